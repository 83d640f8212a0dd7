"""The context workspace grows while a composite runs (csrc/mpe_ws.h): a call that needs more than the block an earlier, smaller call
left chains further blocks under the arrays the composite keeps (WsKeep) or beside the composites it runs concurrently (WsHold), gives
the same bytes, and the workspace settles into ONE block that later calls of that size reuse; wipe and audit see every block.
Every test makes contexts of its own: what the shared one holds depends on the tests that ran before."""
import numpy as np
import pytest
import torch

import fixtures as F
import gg20_fixture as G
import lindell_fixture as L
import orc
import pyref

pytestmark = pytest.mark.gpu

ROWS, NST = 8, 3


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32) if t.dtype == torch.int32 else t.cpu().numpy()


def _flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        out.update(_flat(v, prefix + k + ".") if isinstance(v, dict) else {prefix + k: v})
    return out


# ---- the three composites: (inputs as arrays with ROWS or ROWS * NST rows, the oracle's outputs, objects of a context, the call) ---------
def _mta_tables(keys):
    alice, st = keys[:2], keys[4:4 + NST]
    kidx = [i % 2 for i in range(ROWS)]
    N = F.words([k.N for k in alice], 64)
    tabs = [F.words([getattr(k, f) for k in st], 64) for f in ("Nt", "h1", "h2")]
    return alice, st, kidx, N, tabs


def _mta_objs(ctx, keys):
    from multi_party_ecdsa_amd import engine as E
    alice, st, _, _, _ = _mta_tables(keys)
    return (E.PaillierKeys(ctx, p=[k.p for k in alice], q=[k.q for k in alice]),           # the key holder: x^N through the CRT
            E.Statements(ctx, [k.Nt for k in st], [k.h1 for k in st], [k.h2 for k in st]))


def _mta_message_a_case(keys):
    """tests/test_mta_gpu.py's MessageA on 8 rows and 3 statements"""
    from multi_party_ecdsa_amd import engine as E
    alice, st, kidx, N, tabs = _mta_tables(keys)
    r = F.Rng("gpu-ws-growth-mta")
    a = [r.below(pyref.Q) for _ in range(ROWS)]
    ra = [r.below(alice[k].N) for k in kidx]
    nn = [F.alice_nonces(r, alice[kidx[i]], st[s]) for i in range(ROWS) for s in range(NST)]
    nw = {f: F.words([n[f] for n in nn], w) for f, w in E.ALICE_NONCE_WORDS.items()}
    c_a = orc.paillier_encrypt(N, F.words(a, 64), F.words(ra, 64), kidx)
    kit, sit, bit = [kidx[i] for i in range(ROWS) for _ in range(NST)], [s for _ in range(ROWS) for s in range(NST)], [i for i in range(ROWS) for _ in range(NST)]
    proofs = orc.alice_generate(N, *tabs, kit, sit, F.words([a[i] for i in bit], 8), c_a[bit], F.words([ra[i] for i in bit], 64),
                                nw["alpha"], nw["beta"], nw["gamma"], nw["rho"])
    x = dict(a=F.words(a, 8), ra=F.words(ra, 64), kidx=np.array(kidx, dtype=np.int32), **{"n." + f: v for f, v in nw.items()})
    want = dict(c=c_a, **{"proofs." + f: v for f, v in proofs.items()})

    def call(ctx, o, x):
        c, pr = E.mta_message_a(ctx, o[0], o[1], _dev(ctx, x["a"]), _dev(ctx, x["ra"]), {f: _dev(ctx, x["n." + f]) for f in nw}, _dev(ctx, x["kidx"]))
        return dict(c=c, proofs=pr)
    return x, want, _mta_objs, call


def _mta_message_b_case(keys):
    """tests/test_mta_gpu.py's MessageB on the MessageA above, row 2 with one tampered range proof"""
    from multi_party_ecdsa_amd import engine as E
    alice, st, kidx, N, tabs = _mta_tables(keys)
    xa, wa, _, _ = _mta_message_a_case(keys)
    r = F.Rng("gpu-ws-growth-mta-b")
    b = [r.below(pyref.Q) for _ in range(ROWS)]
    bt = [r.below(alice[k].N) for k in kidx]
    rb = [r.below(alice[k].N) for k in kidx]
    nb, nbt = [r.below(pyref.Q - 1) + 1 for _ in range(ROWS)], [r.below(pyref.Q - 1) + 1 for _ in range(ROWS)]
    proofs = {f: wa["proofs." + f].copy() for f in E.ALICE_PROOF_WORDS}
    proofs["s"][2 * NST + 1, 3] ^= 1
    c_a = wa["c"]
    ok = np.ones(ROWS, dtype=np.uint8)
    ok[2] = 0                                                            # Err(InvalidKey)  (mta/mod.rs:123-131)
    cbt = orc.paillier_encrypt(N, F.words(bt, 64), F.words(rb, 64), kidx)
    cb = orc.paillier_add(N, orc.paillier_mul(N, c_a, F.words(b, 64), kidx), cbt, kidx)
    wp = orc.dlog_prove(F.words(b, 8), F.words(nb, 8))
    wt = orc.dlog_prove(F.words([v % pyref.Q for v in bt], 8), F.words(nbt, 8))
    x = dict(b=F.words(b, 8), c_a=c_a, rb=F.words(rb, 64), bt=F.words(bt, 64), nb=F.words(nb, 8), nbt=F.words(nbt, 8), kidx=np.array(kidx, dtype=np.int32),
             **{"p." + f: v for f, v in proofs.items()})
    want = {"c": cb, "beta": F.words([(-v) % pyref.Q for v in bt], 8), "ok": ok,
            "b_proof.pk": wp[0], "b_proof.R": wp[1], "b_proof.z": wp[2], "beta_tag_proof.pk": wt[0], "beta_tag_proof.R": wt[1], "beta_tag_proof.z": wt[2]}

    def call(ctx, o, x):
        d = lambda f: _dev(ctx, x[f])
        return E.mta_message_b(ctx, o[0], o[1], d("b"), d("c_a"), {f: d("p." + f) for f in proofs}, d("rb"), d("bt"), d("nb"), d("nbt"), d("kidx"))
    return x, want, _mta_objs, call


def _lindell_sign_case(keys):
    """tests/test_lindell_gpu.py's party one on 8 rows: decrypt c3, finish the signature"""
    from multi_party_ecdsa_amd import engine as E
    fx = L.make(keys, ROWS, seed="gpu-ws-growth-lindell")
    c3, r, s, recid = L.oracle_run(fx)
    x = dict(c3=c3, k1=fx["k1"], R2=fx["R2"], kidx=np.array(fx["kidx"], dtype=np.int32))
    want = dict(r=r, s=s, recid=np.asarray(recid))

    def objs(ctx, keys):
        return (E.PaillierKeys(ctx, p=[k.p for k in keys], q=[k.q for k in keys]),)

    def call(ctx, o, x):
        r, s, recid = E.lindell_sign(ctx, o[0], _dev(ctx, x["c3"]), _dev(ctx, x["k1"]), _dev(ctx, x["R2"]), _dev(ctx, x["kidx"]))
        return dict(r=r, s=s, recid=recid)
    return x, want, objs, call


CASES = {"mta_message_a": _mta_message_a_case, "mta_message_b": _mta_message_b_case, "lindell_sign": _lindell_sign_case}
# B1: the smallest multiple of 8 rows at which the call chains a block behind the one the 8-row call left (read off the audit totals of
# runs at neighbouring sizes: the total behind the SECOND run of a size differs from the one behind the first exactly when the first chained)
GROWS_AT = {"mta_message_a": 64, "mta_message_b": 56, "lindell_sign": 512}      # 56, 48 and 504 rows still fit the block the 8 rows left


def grow(keys, name, B1, runs=3):
    """On a fresh context: 8 rows against the oracle, then `runs` times the same rows tiled to B1.  Asserts every byte; returns the
    context and the audit totals behind each call."""
    from multi_party_ecdsa_amd import engine as E
    x, want, objs, call = CASES[name](keys)
    ctx = E.Context(0)
    o = objs(ctx, keys)

    def run(x):
        out = _flat(call(ctx, o, x))
        ctx.sync()
        return {f: _u32(t) for f, t in out.items()}, ctx.scratch_audit()[1]
    got, t0 = run(x)
    assert sorted(got) == sorted(want)
    for f in want:
        assert np.array_equal(got[f].reshape(-1), np.asarray(want[f]).reshape(-1).astype(got[f].dtype)), f
    reps = B1 // ROWS
    big = {f: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for f, v in x.items()}
    totals, first = [t0], None
    for _ in range(runs):
        g, t = run(big)
        totals.append(t)
        for f in want:                                                   # every tile: the 8-row answer
            assert np.array_equal(g[f].reshape(reps, -1), np.broadcast_to(got[f].reshape(1, -1), (reps, got[f].size))), f
        first = first or g
        for f in want:                                                   # ... and every run: the same bytes
            assert np.array_equal(g[f], first[f]), f
    return ctx, totals


@pytest.mark.parametrize("name", sorted(CASES))
def test_growth_inside_a_composite_changes_nothing(keys, name):
    _, (t0, t1, t2, t3) = grow(keys, name, GROWS_AT[name])
    print(f"{name}: audit totals {t0} -> {t1} -> {t2} -> {t3} bytes at {GROWS_AT[name]} rows")
    assert t1 > t0                     # the shape is large enough to test growth at all
    assert t2 != t1                    # ... of the WORKSPACE: the chain the first large call left was replaced by one block
    assert t3 == t2                    # one block, no further growth


def test_wipe_and_audit_see_every_block(keys):
    ctx, _ = grow(keys, "mta_message_b", GROWS_AT["mta_message_b"], runs=1)
    assert ctx.scratch_audit()[0] > 0
    ctx.wipe()
    ctx.sync()
    assert ctx.scratch_audit()[0] == 0


def test_held_begins_grow_too(keys):
    """round0 / round1 of a small batch run their composites side by side out of one begin (WsHold, forks): 2 sessions, then 16 on the
    same context"""
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    lk = G.make_local_keys(keys, 1, 3, [0, 1])
    gk = E.Gg20Keys(ctx, 1, 3, [0, 1], lk["arrays"])
    for B in (2, 16):
        nonces = G.make_nonces(lk, B, seed="wipe")
        r, s, recid, status = E.gg20_sign(ctx, gk, {f: _dev(ctx, v) for f, v in nonces.items()}, B)
        ctx.sync()
        wr, ws, wrecid, _, wstatus = G.oracle_sign(lk, nonces, B)
        assert list(status.cpu().numpy()) == [0] * B == list(wstatus)
        assert np.array_equal(_u32(r), wr) and np.array_equal(_u32(s), ws) and list(recid.cpu().numpy()) == list(wrecid)
        assert ctx.scratch_audit()[0] == 0
