"""GPU: round 5 verifies a party's OWN PDL proofs through the halves p^2 | q^2 of its Paillier key (mpe_proofs.h PdlOwn, mpe_paillier.h
modexp_nn2_holder) and everybody else's on the public key, wherever the verification runs on one stream: large batches, and any batch
on a context without forks (conftest's gpu_ctx_serial, which the cases below use so that small shapes take that route).  The context
option no_r5_self_crt sends them all to the public key again; a small batch on a default context keeps its forked, public schedule.
Whatever the option says, `mpe_gg20_sign` and the per-round API must give the same bytes, and the oracle's; the profiler's launch
records say which route ran:
 a. lock-step signing and the round view with every signer local: (t=1, n=3, signers {0,1}) and (t=2, n=5, three signers), B = 5 (a
    partial wave) and B = 17 (at t = 1: 34 own items, 68 half-items, two 32-item boundaries of a 1024-bit wave), two wallets with a
    per-session key set so that the own-key index differs from the public-key index; the same on a default context, where the
    records must show no holder's ladder
 b. ONE local party per object (L = 1), named by slot and by party index
 c. a party's own proof tampered on its way back to that party (s2, u2, s1, z; the stored c): status 501 and the bad_actors of the
    oracle and of the option-off run; the untampered sessions of the batch still sign"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import gg20_fixture as G
import sigset_cases as SC

pytestmark = pytest.mark.gpu

SHAPES = {"1of3": (1, 3, [0, 1]), "2of5": (2, 5, [0, 2, 4])}


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _i32(ctx, vals):
    return torch.tensor([int(v) for v in vals], dtype=torch.int32, device=ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _oracle(lk, nonces, keyset, B):
    """orc_gg20_sign_ex over the batch, the sessions spread over host threads (each call writes its own sessions' rows).
    (gg20_fixture.oracle_sign is the same oracle without a per-session key set and without the round messages, which these cases need.)"""
    import orc
    S, n = lk["S"], lk["n"]
    slabs = {rnd: np.zeros((S, B, G.msg_words(S, n, rnd)), dtype=np.uint32) for rnd in G.ROUNDS}
    ptrs = (C.c_void_p * 7)(*[slabs[rnd].ctypes.data for rnd in G.ROUNDS])
    r, s = np.zeros((B, 8), dtype=np.uint32), np.zeros((B, 8), dtype=np.uint32)
    recid, status = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    R = np.zeros((B, 16), dtype=np.uint32)
    pst, pbad = np.zeros((S, B), dtype=np.int32), np.zeros((S, B), dtype=np.uint32)
    ks, ns = G.keys_struct(lk), G.nonces_struct(nonces)
    kset = np.ascontiguousarray(keyset, dtype=np.int32)

    def one(b):
        orc.lib.orc_gg20_sign_ex(C.byref(ks), C.byref(ns), orc._p(kset), B, b, 1, ptrs, orc._p(r), orc._p(s), orc._p(recid), orc._p(R),
                                 orc._p(status), orc._p(pst), orc._p(pbad))
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, range(B)))
    return dict(slabs=slabs, r=r, s=s, recid=recid, R=R, status=status, party_status=pst, party_bad=pbad)


class Case:
    """two wallets, session b on wallet keyset[b]; one signer set"""

    def __init__(self, keys, name, B):
        self.t, self.n, self.signers = SHAPES[name]
        self.S, self.B = len(self.signers), B
        self.keyset = [(b * b + b // 3) % 2 for b in range(B)]
        lks, per_wallet = SC.wallet(keys, self.t, self.n, [self.signers], nwallets=2)
        self.lk = lks[0]
        self.nonces = SC.mixed_nonces(per_wallet, [0] * B, seed=f"r5-self-{name}-{B}", keyset=self.keyset)
        self.want = _oracle(self.lk, self.nonces, self.keyset, B)
        assert not self.want["status"].any()


_cases = {}


@pytest.fixture(scope="module")
def case_of(keys):
    def get(name, B):
        if (name, B) not in _cases:
            _cases[(name, B)] = Case(keys, name, B)
        return _cases[(name, B)]
    return get


@pytest.fixture(scope="module")
def ctx_off():
    """gpu_ctx_serial's code paths with the option off"""
    from multi_party_ecdsa_amd import engine as E
    return E.Context(0, options={"no_par": 1, "no_adaptive_lanes": 1, "no_r5_self_crt": 1})


def _holder_launches(recs, half_items):
    """how many times modexp_nn2_holder ran, by the launch records of its second ladder a^p (c^-1)^e mod p^2 over `half_items` half-items:
    nothing else launches a two-base ladder on the 1024-bit pair engine (kind 3, 2048 bits, exp2_words 8).  Its first ladder, half mode
    (kind 4) with a 32-word exponent over the same items, must be there as often at least (the provers' beta^N has the same shape)."""
    second = [r for r in recs if r["kind"] == 3 and r["bits"] == 2048 and r["exp_words"] == 32 and r["exp2_words"] == 8]
    assert all(r["batch"] == half_items for r in second), second
    first = [r for r in recs if r["kind"] == 4 and r["bits"] == 1024 and r["exp_words"] == 32 and r["batch"] == half_items]
    assert len(first) >= len(second)
    return len(second)


def _profiled(ctx, fn):
    ctx.prof_enable(True)
    try:
        out = fn()
        ctx.sync()
        return out, ctx.prof_collect(4096)
    finally:
        ctx.prof_enable(False)


def _lockstep(ctx, c):
    """(mpe_gg20_sign's outputs, {round: [S, B, W]} and the result of the round view with every signer local)"""
    from multi_party_ecdsa_amd import engine as E
    gk = E.Gg20Keys(ctx, c.t, c.n, c.signers, c.lk["arrays"], nkeysets=2)
    dn, dk = {f: _dev(ctx, v) for f, v in c.nonces.items()}, _i32(ctx, c.keyset)
    sign = [o.cpu().numpy() for o in E.gg20_sign(ctx, gk, dn, c.B, want_R=True, keyset=dk)]
    sess = E.Gg20Session(ctx, gk, c.B, list(range(c.S)), dn, keyset=dk)
    slabs, prev = {}, None
    for rnd in range(9):
        out = sess.round(rnd, d_in=prev, msg=dn["msg"] if rnd == 7 else None)
        if rnd in G.ROUNDS:
            slabs[rnd] = _u32(out)
            prev = out
    res = sess.result()
    ctx.sync()
    res = {f: (_u32(v) if f in ("r", "s", "R", "bad_actors") else v.cpu().numpy()) for f, v in res.items()}
    sess.close()
    gk.close()
    return sign, slabs, res


def _check_lockstep(got, c):
    (r, s, recid, status, R), slabs, res = got
    w = c.want
    assert not status.any()
    assert np.array_equal(r.view(np.uint32), w["r"]) and np.array_equal(s.view(np.uint32), w["s"]) and list(recid) == list(w["recid"])
    assert np.array_equal(R.view(np.uint32), w["R"])
    for rnd in G.ROUNDS:
        assert np.array_equal(slabs[rnd], w["slabs"][rnd]), f"round {rnd}"
    assert not res["status"].any() and not res["bad_actors"].any()
    for i in range(c.S):
        assert np.array_equal(res["r"][i], w["r"]) and np.array_equal(res["s"][i], w["s"]) and list(res["recid"][i]) == list(w["recid"])


# ---- a. every signer local ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("1of3", 5), ("1of3", 17), ("2of5", 5), ("2of5", 17)])
def test_a_sign_and_round_view_are_the_same_with_the_option_on_and_off(gpu_ctx_serial, ctx_off, case_of, name, B):
    c = case_of(name, B)
    assert gpu_ctx_serial.get_option("no_r5_self_crt") == 0 and ctx_off.get_option("no_r5_self_crt") == 1
    (on, recs_on), (off, recs_off) = _profiled(gpu_ctx_serial, lambda: _lockstep(gpu_ctx_serial, c)), _profiled(ctx_off, lambda: _lockstep(ctx_off, c))
    # mpe_gg20_sign and the round view each ran round 5 once: two holder's ladder pairs over 2 B S (S-1) half-items, none with the option off
    assert _holder_launches(recs_on, 2 * c.B * c.S * (c.S - 1)) == 2
    assert _holder_launches(recs_off, 2 * c.B * c.S * (c.S - 1)) == 0
    for a, b in zip(on[0], off[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(on[1][5], off[1][5]), "the round-5 slab"
    for f in on[2]:
        assert np.array_equal(on[2][f], off[2][f]), f
    _check_lockstep(on, c)
    _check_lockstep(off, c)


@pytest.mark.parametrize("name,B", [("1of3", 17), ("2of5", 5)])
def test_a_small_batches_on_a_default_context_keep_the_public_route(gpu_ctx, case_of, name, B):
    """up to par_items (32 768) verification items a default context forks its composites: the split is not applied there"""
    assert gpu_ctx.get_option("no_r5_self_crt") == 0 and gpu_ctx.get_option("no_par") == 0
    c = case_of(name, B)
    got, recs = _profiled(gpu_ctx, lambda: _lockstep(gpu_ctx, c))
    assert _holder_launches(recs, 2 * c.B * c.S * (c.S - 1)) == 0
    _check_lockstep(got, c)


# ---- b. one local party per object -------------------------------------------------------------------------------------------------
def _one_party_objects(ctx, c, by_party):
    from multi_party_ecdsa_amd import engine as E
    dk = _i32(ctx, c.keyset)
    out = []
    for i, p in enumerate(c.signers):
        dn = {f: _dev(ctx, v) for f, v in G.party_nonces(c.nonces, c.lk, i).items()}
        if by_party:
            gk = E.Gg20Keys(ctx, c.t, c.n, None, c.lk["arrays"], own=[p], nkeysets=2, signer_sets=[c.signers])
            sess = E.Gg20Session(ctx, gk, c.B, None, dn, keyset=dk, sigset=_i32(ctx, [0] * c.B), local_party=p)
        else:
            gk = E.Gg20Keys(ctx, c.t, c.n, c.signers, c.lk["arrays"], own=[p], nkeysets=2)
            sess = E.Gg20Session(ctx, gk, c.B, [i], dn, keyset=dk)
        out.append(dict(gk=gk, dn=dn, sess=sess))
    return out


def _relay(ctx, parties, c, tamper=None):
    """every party's rounds over a relay; tamper(rnd, slab, receiver) may change what ONE receiver is handed.
    Returns ({round: [S, B, W]}, [result dict per party])"""
    slabs, prev = {}, None
    for rnd in range(9):
        outs = []
        for i, q in enumerate(parties):
            d_in = None
            if prev is not None and rnd != 7:
                mine = prev.copy()
                if tamper:
                    tamper(rnd - 1 if rnd != 8 else 7, mine, i)
                d_in = _dev(ctx, mine)
            outs.append(q["sess"].round(rnd, d_in=d_in, msg=q["dn"]["msg"] if rnd == 7 else None))
        if rnd in G.ROUNDS:
            slabs[rnd] = prev = np.ascontiguousarray(np.stack([_u32(o)[0] for o in outs]))
    res = []
    for q in parties:
        o = q["sess"].result()
        ctx.sync()
        res.append({f: (_u32(v)[0] if f in ("r", "s", "R", "bad_actors") else v.cpu().numpy()[0]) for f, v in o.items()})
        q["sess"].close()
        q["gk"].close()
    return slabs, res


@pytest.mark.parametrize("by_party", [False, True], ids=["by_slot", "by_party_index"])
@pytest.mark.parametrize("name", ["1of3", "2of5"])
def test_b_one_local_party_per_object(gpu_ctx_serial, ctx_off, case_of, name, by_party):
    c = case_of(name, 5)
    (on, recs), off = _profiled(gpu_ctx_serial, lambda: _relay(gpu_ctx_serial, _one_party_objects(gpu_ctx_serial, c, by_party), c)), \
        _relay(ctx_off, _one_party_objects(ctx_off, c, by_party), c)
    assert _holder_launches(recs, 2 * c.B * (c.S - 1)) == c.S          # every party's round 5: its S-1 own proofs per session
    got = [on, off]
    for slabs, res in got:
        for rnd in G.ROUNDS:
            assert np.array_equal(slabs[rnd], c.want["slabs"][rnd]), f"round {rnd}"
        for o in res:
            assert not o["status"].any() and not o["bad_actors"].any()
            assert np.array_equal(o["r"], c.want["r"]) and np.array_equal(o["s"], c.want["s"]) and list(o["recid"]) == list(c.want["recid"])
    assert np.array_equal(got[0][0][5], got[1][0][5]), "the round-5 slab"


# ---- c. a party's own proof, tampered on its way back to it ------------------------------------------------------------------------
# session -> (round of the message, word offset in the sender's record): fields of M4P sub-record 0 (include/mpecdsa_hip.h), and the
# ciphertext of the last M0 sub-record, which the receiver stores and reads again in round 5
def _tampers(n):
    return {1: (4, 297), 2: (4, 80), 3: (4, 272), 4: (4, 0), 5: (0, n * 256)}


def _oracle_relay(c, tamper):
    parties = [G.OracleParty(c.lk, i, c.B, G.party_nonces(c.nonces, c.lk, i), keyset=c.keyset) for i in range(c.S)]
    prev = None
    for rnd in range(9):
        outs = []
        for i, p in enumerate(parties):
            d_in = None
            if rnd == 7:
                d_in = c.nonces["msg"]
            elif prev is not None:
                d_in = prev.copy()
                tamper(rnd - 1 if rnd != 8 else 7, d_in, i)
            outs.append(p.round(rnd, d_in))
        if rnd in G.ROUNDS:
            prev = np.ascontiguousarray(np.stack(outs))
    res = [p.result() for p in parties]
    for p in parties:
        p.close()
    return res


def test_c_tampered_own_proofs_are_rejected_like_the_oracle_rejects_them(gpu_ctx_serial, ctx_off, keys):
    victim = 1                                                   # signer ordinal whose own proof (and stored c) is corrupted on its way home
    c = Case(keys, "1of3", 7)
    tampers = _tampers(c.n)

    def tamper(rnd, slab, receiver):
        if receiver != victim:
            return
        for b, (r, word) in tampers.items():
            if r == rnd:
                slab[victim, b, word] ^= 4
    want = _oracle_relay(c, tamper)
    clean = [b for b in range(c.B) if b not in tampers]
    for b in tampers:
        assert want[victim]["status"][b] == 501 and want[victim]["bad_actors"][b] == 1 << victim, b
    got = [_relay(ctx, _one_party_objects(ctx, c, False), c, tamper)[1] for ctx in (gpu_ctx_serial, ctx_off)]
    for res in got:
        for i in range(c.S):
            print("party", i, "status", list(res[i]["status"]), "bad_actors", list(res[i]["bad_actors"]), "oracle", list(want[i]["status"]))
            assert list(res[i]["status"]) == list(want[i]["status"])
            assert list(res[i]["bad_actors"]) == list(want[i]["bad_actors"])
            assert not res[i]["status"][clean].any()
            assert np.array_equal(res[i]["r"][clean], c.want["r"][clean]) and np.array_equal(res[i]["s"][clean], c.want["s"][clean])
