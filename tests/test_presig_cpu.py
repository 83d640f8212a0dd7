"""CPU tests of the presignature pool's contract: the restatement (tests/pyref_presig.py) rejects every illegal slot
transition, its record round-trips, its `phase7_local_sig` + `output_signature` reproduce the oracle's signatures over the
fixture, and the header, the library and the harness agree on the calls and the status codes.  No GPU: the library is only
loaded, never run."""
import os
import re

import numpy as np
import pytest

import fixtures as F
import gg20_fixture as G
import pyref
import pyref_presig as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["pool_create", "pool_destroy", "pool_capacity", "record_words", "deposit", "sign", "complete", "export", "import", "discard",
         "pool_audit"]


@pytest.fixture(autouse=True)
def native():
    """the restatement restates calls that exist: every test here needs the library to export them"""
    from multi_party_ecdsa_amd import _native as N
    for c in CALLS:
        assert hasattr(N.lib, "mpe_gg20_presig_" + c), c
    return N


def _header():
    return open(os.path.join(ROOT, "include", "mpecdsa_hip.h")).read()


def test_header_declares_every_call_the_harness_binds_and_states_the_codes_once(native):
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mpe_gg20_presig_[a-z0-9_]+)\s*\(", code))
    assert declared == {"mpe_gg20_presig_" + c for c in CALLS}
    assert declared <= set(native.EXPORTED)
    engine = open(os.path.join(ROOT, "multi_party_ecdsa_amd", "engine.py")).read()
    assert set(re.findall(r"(?:lib|call)\.(mpe_gg20_presig_\w+)\(", engine)) == declared     # the harness binds them all
    defines = dict(re.findall(r"#define MPE_GG20_PRESIG_(\w+) (\d+)", hdr))
    want = dict(RECORD_VERSION=PP.RECORD_VERSION, DEPOSIT_RANGE=PP.DEPOSIT_RANGE, DEPOSIT_NOT_EMPTY=PP.DEPOSIT_NOT_EMPTY,
                SESSION_FAILED=PP.SESSION_FAILED, SIGN_RANGE=PP.SIGN_RANGE, SIGN_NOT_READY=PP.SIGN_NOT_READY,
                COMPLETE_RANGE=PP.COMPLETE_RANGE, COMPLETE_NOT_SIGNED=PP.COMPLETE_NOT_SIGNED, VERIFY_FAILED=PP.VERIFY_FAILED,
                RECORD_RANGE=PP.RECORD_RANGE, IMPORT_REFUSED=PP.IMPORT_REFUSED, EXPORT_NOT_READY=PP.EXPORT_NOT_READY,
                IMPORT_NOT_EMPTY=PP.IMPORT_NOT_EMPTY)
    assert {k: int(v) for k, v in defines.items()} == want
    for k, v in want.items():
        assert getattr(native, "PRESIG_" + k) == v, k
    assert (PP.DEPOSIT_RANGE, PP.DEPOSIT_NOT_EMPTY, PP.SESSION_FAILED, PP.SIGN_RANGE, PP.SIGN_NOT_READY, PP.COMPLETE_NOT_SIGNED,
            PP.IMPORT_REFUSED, PP.VERIFY_FAILED) == (801, 802, 803, 811, 812, 822, 832, 701)
    # the layout is this library's own and the header says so; the abort comment names deposit instead of "stops after the offline stage"
    assert "no byte parity" in hdr and "Serialize" in hdr
    abort = hdr[hdr.index("/* Gives the running batch up"):hdr.index("int mpe_gg20_session_abort")]
    assert "the caller stops after the offline stage" not in abort and "mpe_gg20_presig_deposit" in abort


def test_argument_errors_without_gpu(native):
    lib = native.lib
    assert lib.mpe_gg20_presig_pool_create(None, None, 1, None, 4, None) == native.MPE_E_ARG
    assert lib.mpe_gg20_presig_pool_capacity(None) == native.MPE_E_ARG
    assert lib.mpe_gg20_presig_deposit(None, None, None, None, None) == native.MPE_E_ARG
    assert lib.mpe_gg20_presig_sign(None, 1, None, None, None, None, None) == native.MPE_E_ARG
    assert lib.mpe_gg20_presig_complete(None, 1, None, None, None, None, None, None, None, None) == native.MPE_E_ARG
    assert lib.mpe_gg20_presig_pool_audit(None, None, None) == native.MPE_E_ARG


def _presig(seed, L=2, keyset=0):
    r = F.Rng(seed)
    sc = lambda: r.below(PP.Q - 1) + 1
    return dict(keyset=keyset, parties=[dict(k=sc(), sigma=sc(), R=pyref.ec_mul(sc(), pyref.G)) for _ in range(L)])


def _pool(capacity=3):
    y = pyref.ec_mul(0x1234567, pyref.G)
    return PP.Pool([0, 2], [0, 1], [y], capacity)


def _put(pool, slot, state):
    """brings an EMPTY slot into `state` by legal transitions only"""
    if state >= PP.READY:
        assert pool.deposit(slot, _presig(f"put-{slot}")) == 0
    if state == PP.SIGNED:
        assert pool.sign(slot, 99)[0] == 0


def test_state_machine_rejects_every_illegal_transition():
    # (call, state the slot must be in, status otherwise)
    rules = [("deposit", PP.EMPTY, PP.DEPOSIT_NOT_EMPTY), ("sign", PP.READY, PP.SIGN_NOT_READY), ("complete", PP.SIGNED, PP.COMPLETE_NOT_SIGNED),
             ("export", PP.READY, PP.EXPORT_NOT_READY), ("import_", PP.EMPTY, PP.IMPORT_NOT_EMPTY)]
    rec = PP.record_pack(PP.signer_mask([0, 2]), [0, 1], 0, pyref.ec_mul(0x1234567, pyref.G), _presig("rec")["parties"])
    args = dict(deposit=(_presig("x"),), sign=(7,), complete=([1, 2],), export=(), import_=(rec,))
    for call, legal, code in rules:
        for state in (PP.EMPTY, PP.READY, PP.SIGNED):
            pool = _pool()
            _put(pool, 1, state)
            before = (list(pool.state), [None if s is None else repr(s) for s in pool.slot])
            out = getattr(pool, call)(1, *args[call])
            got = out if isinstance(out, int) else (out[0][0] if call == "complete" else out[0])
            if state == legal:
                assert got in (0, PP.VERIFY_FAILED), (call, state)
                with_strict = _pool(); _put(with_strict, 1, state); with_strict.strict(call, 1, *args[call])
            else:
                assert got == code, (call, state)
                assert (list(pool.state), [None if s is None else repr(s) for s in pool.slot]) == before     # the loser touches nothing
                with pytest.raises(PP.IllegalTransition):
                    pool.strict(call, 1, *args[call])
            # out of range: the range code of the call, nothing touched
            for bad in (-1, pool.capacity):
                o = getattr(pool, call)(bad, *args[call])
                g = o if isinstance(o, int) else (o[0][0] if call == "complete" else o[0])
                assert g == dict(deposit=801, sign=811, complete=821, export=831, import_=831)[call]
    pool = _pool()
    assert pool.deposit(0, _presig("f"), healthy=False) == PP.SESSION_FAILED and pool.state[0] == PP.EMPTY
    # single use: READY -> SIGNED once, and the signed slot holds no k_i / sigma_i
    _put(pool, 0, PP.READY)
    assert pool.sign(0, 5)[0] == 0 and pool.sign(0, 5) == (PP.SIGN_NOT_READY, [0, 0])
    assert pool.audit() == ([2, 0, 1, 0], 0)
    for state in (PP.EMPTY, PP.READY, PP.SIGNED):                     # discard: any state -> EMPTY
        p2 = _pool(); _put(p2, 2, state); p2.discard(2)
        assert p2.audit() == ([3, 0, 0, 0], 0)


def test_record_round_trips_and_tampered_records_are_refused():
    pool = _pool()
    ps = _presig("roundtrip")
    assert pool.deposit(2, ps) == 0
    code, rec = pool.export(2)
    assert code == 0 and pool.state[2] == PP.EMPTY and len(rec) == 28 + 32 * 2 and all(0 <= w < 2 ** 32 for w in rec)
    u = PP.record_unpack(rec)
    assert u["parties"] == ps["parties"] and (u["version"], u["mask"], u["L"], u["local"], u["keyset"]) == (1, 0b101, 2, [0, 1, 0, 0, 0, 0, 0, 0], 0)
    assert PP.record_pack(u["mask"], u["local"][:2], u["keyset"], u["y"], u["parties"]) == rec
    assert pool.import_(0, rec) == 0 and pool.slot[0]["parties"] == ps["parties"]
    q8 = [(PP.Q >> (32 * j)) & 0xFFFFFFFF for j in range(8)]

    def tampered(at, words):
        t = list(rec)
        t[at:at + len(words)] = words
        return t
    bad = dict(version=tampered(0, [2]), mask=tampered(1, [0b011]), L=tampered(2, [1]), ordinals=tampered(4, [2]), keyset=tampered(11, [1]),
               y=tampered(12, [rec[12] ^ 1]), k_zero=tampered(28, [0] * 8), k_q=tampered(28, q8), sigma_q=tampered(36 + 32, q8),
               R_off_curve=tampered(44, [rec[44] ^ 1]), R_neutral=tampered(44, [0] * 16))
    for name, t in bad.items():
        assert pool.import_(1, t) == PP.IMPORT_REFUSED and pool.state[1] == PP.EMPTY, name
    assert pool.import_(1, tampered(36, [0] * 8)) == 0                     # sigma_i = 0 is in [0, q)


def test_phase7_and_output_signature_reproduce_the_oracle(keys):
    """the fixture's sessions through rounds 0-6 of the GG20 restatement, then the pool's restatement online: the oracle's bytes"""
    import pyref_gg20 as PG
    lk = G.make_local_keys(keys, 1, 3, [0, 2])
    B = 2
    nonces = G.make_nonces(lk, B, seed="presig-cpu")
    wr, ws, wrecid, wR, wstatus = G.oracle_sign(lk, nonces, B)
    assert list(wstatus) == [0] * B
    pool = PP.Pool([0, 2], [0, 1], [lk["y"]], 4)
    slots = [3, 1]
    msgs = F.ints(nonces["msg"])
    presigs, m6 = [], []
    for b in range(B):
        parties = G.py_parties(lk, nonces, b)
        m6.append(PG.simulate(parties, msgs[b])[0][6])                     # the fused path's partial signatures
        assert all(p.status == 0 for p in parties)
        presigs.append(dict(keyset=0, parties=[dict(k=p.k, sigma=p.sigma_i, R=p.R) for p in parties]))
        assert pool.deposit(slots[b], presigs[b]) == 0
    for b in reversed(range(B)):                                           # online, in another order than the offline stage ran
        code, s_i = pool.sign(slots[b], msgs[b])
        assert code == 0 and s_i == m6[b]
        want = (0, F.ints(wr[b:b + 1])[0], F.ints(ws[b:b + 1])[0], int(wrecid[b]))
        assert pool.complete(slots[b], s_i) == [want] * 2
    assert pool.complete(slots[0], [1, 2])[0][0] == PP.COMPLETE_NOT_SIGNED
    assert pool.audit() == ([4, 0, 0, 0], 0)
    # a doubled partial signature of signer 1 (the reference's step-7 corruption, gg_2020/test.rs:679-686) among the incoming ones:
    # 701 and zero outputs at the party that reads it (a party takes its OWN s_i from the slot), the slot freed
    pool.deposit(0, presigs[0])
    _, s_i = pool.sign(0, msgs[0])
    want = (0, F.ints(wr[0:1])[0], F.ints(ws[0:1])[0], int(wrecid[0]))
    assert pool.complete(0, [s_i[0], 2 * s_i[1] % PP.Q]) == [(701, 0, 0, 0), want] and pool.state[0] == PP.EMPTY
    assert np.array_equal(F.words([PP.phase7_local_sig(msgs[0], 3, 5, (7, 9))[2]], 8), F.words([(msgs[0] % PP.Q * 3 + 7 * 5) % PP.Q], 8))
