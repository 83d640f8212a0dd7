"""GPU: the stand-alone C-ABI verifiers on hostile points, scalars and residues (the table of tests/hostile_cases.py, proved on the CPU by
tests/test_hostile_cases_cpu.py).  Every entry point that takes a curve point from a peer must refuse the neutral element, an off-curve point
and a coordinate >= p through `ec::aff_valid` BEFORE a secret or a challenge touches it: the table's DECISIVE rows are proofs an unguarded
verifier accepts, so only that guard stands between them and a 1.  One batch of 70 per call (one item per lane in 64-thread blocks: hostile
rows in lanes 0, 63, 64 and spread between, at least a third honest), every verdict compared with the table's row by row, and every honest
row 1: a lane's early return disturbs no neighbour.  The calls that use a secret fail closed: mpe_lindell_partial_sig returns Enc(0; r) and
mpe_lindell_sign no signature for an invalid R1 / R2, mpe_mta_verify_get_alpha still returns alpha = share mod q.  Bob's range proof on
hostile residues at B = 12 (lane-serial inversions) and 44 (the batched route), under the public and the private key object, with and
without the (X, u) extension: the oracle's verdicts.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import fixtures as F
import hostile_cases as H
import lindell_fixture as L
import orc
import pyref
from test_hostile_cases_cpu import blame7_opened

pytestmark = pytest.mark.gpu


def E():
    from multi_party_ecdsa_amd import engine
    return engine


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy().view(np.uint32))


def _di(ctx, v):
    return torch.tensor(v, dtype=torch.int32, device=ctx.device)


def _check(case, got):
    """row by row against the table, no row left out; then the honest rows on their own"""
    got = [int(v) for v in got]
    assert len(got) == H.B
    assert [(i, case.labels[i], got[i]) for i in range(H.B) if got[i] != case.want[i]] == []
    assert all(got[i] == case.honest_value for i in case.honest) and 3 * len(case.honest) >= H.B


def test_dlog_verify_on_hostile_rows(gpu_ctx):
    c = H.dlog_case()
    d = lambda f: _dev(gpu_ctx, H.words(c, f))
    _check(c, E().dlog_verify(gpu_ctx, d("pk"), d("R"), d("z")).cpu().numpy())


def test_pedersen_verify_on_hostile_rows(gpu_ctx):
    c = H.pedersen_case()
    _check(c, E().pedersen_verify(gpu_ctx, {f: _dev(gpu_ctx, H.words(c, f)) for f in ("com", "e", "a1", "a2", "z1", "z2")}).cpu().numpy())


def test_heg_verify_on_hostile_rows(gpu_ctx):
    c = H.heg_case()
    d = lambda fs: {f: _dev(gpu_ctx, H.words(c, f)) for f in fs}
    _check(c, E().heg_verify(gpu_ctx, d(("G", "H", "Y", "D", "E")), d(("T", "A3", "z1", "z2"))).cpu().numpy())


def test_ecddh_verify_on_hostile_rows(gpu_ctx):
    c = H.ecddh_case()
    d = lambda fs: {f: _dev(gpu_ctx, H.words(c, f)) for f in fs}
    _check(c, E().ecddh_verify(gpu_ctx, d(("g1", "h1", "g2", "h2")), d(("a1", "a2", "z"))).cpu().numpy())


def test_pdl_verify_on_hostile_points(gpu_ctx, keys):
    e = E()
    c = H.pdl_case()
    pk = e.PaillierKeys(gpu_ctx, N=[k.N for k in keys[:H.PDL_KEYS]])
    st = keys[4:4 + H.PDL_STATEMENTS]
    stm = e.Statements(gpu_ctx, [k.Nt for k in st], [k.h1 for k in st], [k.h2 for k in st])
    d = lambda f: _dev(gpu_ctx, H.words(c, f))
    ok = e.pdl_verify(gpu_ctx, pk, stm, d("c"), d("Q"), d("G"), {f: d(f) for f in e.PDL_PROOF_WORDS}, _di(gpu_ctx, c.col("kidx")), _di(gpu_ctx, c.col("sidx")))
    _check(c, ok.cpu().numpy())


def test_mta_verify_get_alpha_on_hostile_points(gpu_ctx, keys):
    """ok follows the table; alpha = share mod q on EVERY row (it is the decryption and does not depend on the points), share = a b + beta_tag"""
    e = E()
    c = H.mta_case()
    sk = e.PaillierKeys(gpu_ctx, p=[k.p for k in keys[:H.MTA_KEYS]], q=[k.q for k in keys[:H.MTA_KEYS]])
    d = lambda f: _dev(gpu_ctx, H.words(c, f))
    alpha, share, ok = e.mta_verify_get_alpha(gpu_ctx, sk, d("cb"), dict(pk=d("pk"), R=d("R"), z=d("z")), dict(pk=d("tpk"), R=d("tR"), z=d("tz")),
                                              d("a"), _di(gpu_ctx, c.col("kidx")))
    gpu_ctx.sync()
    _check(c, ok.cpu().numpy())
    assert [int(ok[i]) for i in sorted(c.decisive)] == [0] * len(c.decisive)
    assert e.host(share) == c.col("share")
    assert e.host(alpha) == [s % pyref.Q for s in c.col("share")]


def test_blame7_on_hostile_points(gpu_ctx):
    """70 sessions of two signers: the bad-actor mask names signer i when R, R_dash_i or S_i is no valid point (an invalid R: both)"""
    c = H.blame7_case()
    got = E().gg20_blame7(gpu_ctx, H.BLAME7_S, H.B, {f: _dev(gpu_ctx, v) for f, v in blame7_opened(c).items()})
    gpu_ctx.sync()
    _check(c, _u32(got))


def _lindell(keys):
    fx = L.make(keys, H.B, seed="gpu-hostile-lindell")
    return fx, L.oracle_run(fx)


def _with_kinds(honest_words):
    """the column with the rows of H.lindell_rows replaced; -> (words, the lanes whose point is now invalid)"""
    pts, invalid = [H.raw(p) for p in F.points(honest_words)], []
    for lane, kind in H.lindell_rows():
        pts[lane] = H.kind_point(kind, pts[lane], lane)
        assert H.kind_holds(kind, pts[lane])
        if not H.valid(pts[lane]):
            invalid.append(lane)
    assert len(invalid) == len(H.INVALID_KINDS)
    return H.point_words(pts), invalid


def test_lindell_partial_sig_fails_closed_on_invalid_R1(gpu_ctx, keys):
    """an invalid R1: c3 = r^N mod N^2 = Enc(0; r) — nothing of k2 or x2 is in it; every other row (the negated R1 included) is the oracle's c3"""
    e = E()
    fx, _ = _lindell(keys)
    R1, invalid = _with_kinds(fx["R1"])
    pk = e.PaillierKeys(gpu_ctx, N=[k.N for k in keys])
    d = lambda name: _dev(gpu_ctx, fx[name])
    c3 = e.lindell_partial_sig(gpu_ctx, pk, d("c_key"), d("x2"), d("k2"), _dev(gpu_ctx, R1), d("msg"), d("rho"), d("r"), _di(gpu_ctx, fx["kidx"]))
    gpu_ctx.sync()
    got = F.ints(_u32(c3))
    want = F.ints(orc.lindell_partial_sig(fx["N"], fx["c_key"], fx["x2"], fx["k2"], R1, fx["msg"], fx["rho"], fx["r"], fx["kidx"]))
    rr = F.ints(fx["r"])
    for i in invalid:
        N = keys[fx["kidx"][i]].N
        want[i] = pow(rr[i], N, N * N)
    assert [i for i in range(H.B) if got[i] != want[i]] == []


def test_lindell_sign_fails_closed_on_invalid_R2(gpu_ctx, keys):
    """an invalid R2: r = s = 0 and recid = -1 — no signature leaves and k1 never touches the point; every other row is the oracle's"""
    e = E()
    fx, (c3, _, _, _) = _lindell(keys)
    R2, invalid = _with_kinds(fx["R2"])
    sk = e.PaillierKeys(gpu_ctx, p=[k.p for k in keys], q=[k.q for k in keys])
    r, s, recid = e.lindell_sign(gpu_ctx, sk, _dev(gpu_ctx, c3), _dev(gpu_ctx, fx["k1"]), _dev(gpu_ctx, R2), _di(gpu_ctx, fx["kidx"]))
    gpu_ctx.sync()
    wr, ws, wrecid = orc.lindell_sign(fx["p"], fx["q"], c3, fx["k1"], R2, fx["kidx"])
    wr[invalid], ws[invalid], wrecid[invalid] = 0, 0, -1
    gr, gs = _u32(r), _u32(s)
    assert [i for i in range(H.B) if not (np.array_equal(gr[i], wr[i]) and np.array_equal(gs[i], ws[i]))] == []
    assert list(recid.cpu().numpy()) == list(wrecid)
    assert not gr[invalid].any() and not gs[invalid].any() and list(recid.cpu().numpy()[invalid]) == [-1] * len(invalid)


# ---- Bob's range proof ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bob_env(gpu_ctx, keys):
    e = E()
    objs = dict(public=e.PaillierKeys(gpu_ctx, N=[k.N for k in keys[:4]]), holder=e.PaillierKeys(gpu_ctx, p=[k.p for k in keys[:4]], q=[k.q for k in keys[:4]]))
    stm = e.Statements(gpu_ctx, [k.Nt for k in keys[4:7]], [k.h1 for k in keys[4:7]], [k.h2 for k in keys[4:7]])
    tabs = [F.words([k.N for k in keys[:4]], 64)] + [F.words([getattr(k, f) for k in keys[4:7]], 64) for f in ("Nt", "h1", "h2")]
    return objs, stm, tabs, {}


@pytest.mark.parametrize("check", [False, True])
@pytest.mark.parametrize("key_object", ["public", "holder"])
@pytest.mark.parametrize("B", H.BOB_BATCHES)
def test_bob_verify_on_hostile_values(gpu_ctx, keys, bob_env, B, key_object, check):
    """The rows of hostile_cases.BOB_ROWS on proofs from mpe_bob_generate: s = N, 0, N - 1, 2^2048 - 1; z, t = N~, 0; mta_enc = 0, 7 N, 11 p,
    unreduced; a_enc = 7 N; s1 at the range bound; s2, t2, t1 all ones; e = 0; three FORGED transcripts (hostile_cases.bob_forge) that only
    the flag of one of the three inversions refuses — and with `check` X and u of every point kind, the two
    decisive ones (b = 0, alpha = q: honest proofs whose X / u is the neutral row) included.  B = 12 inverts on the lane-serial kernel;
    at B = 44 the three inversions take the batched route (mpe_modinv.h) and the non-units share chunks with honest proofs.  `holder`: the
    verifier owns the key (Alice, the normal case) and her exponentiations go through p^2 | q^2.  The verdicts equal the oracle's (and the
    validity rule on X, u), the rows the table marks rejected are 0, the honest tail is 1, and both key objects give the same verdicts."""
    e = E()
    objs, stm, tabs, seen = bob_env
    inp = H.bob_inputs(B)
    kidx, sidx = inp["kidx"], inp["sidx"]
    nw = {f: F.words([n[f] for n in inp["nonces"]], w) for f, w in e.BOB_NONCE_WORDS.items()}
    dA, dM = e.dev(gpu_ctx, inp["a_enc"], 128), e.dev(gpu_ctx, inp["mta_enc"], 128)
    pr, u = e.bob_generate(gpu_ctx, objs["public"], stm, dA, dM, e.dev(gpu_ctx, inp["b"], 8), e.dev(gpu_ctx, inp["beta_prim"], 64),
                           e.dev(gpu_ctx, inp["r"], 64), {f: _dev(gpu_ctx, v) for f, v in nw.items()}, check, _di(gpu_ctx, kidx), _di(gpu_ctx, sidx))
    gpu_ctx.sync()
    cols = {f: e.host(v) for f, v in pr.items()}
    cols.update(a_enc=list(inp["a_enc"]), mta_enc=list(inp["mta_enc"]))
    X = [H.raw(pyref.ec_mul(b, H.G)) for b in inp["b"]] if check else None
    uu = [H.raw(p) for p in F.points(_u32(u))] if check else None
    H.bob_tamper(B, check, cols, X, uu)
    pw = {f: F.words(cols[f], w) for f, w in e.BOB_PROOF_WORDS.items()}
    aw, mw = F.words(cols["a_enc"], 128), F.words(cols["mta_enc"], 128)
    Xw, uw = (H.point_words(X), H.point_words(uu)) if check else (None, None)
    ok = e.bob_verify(gpu_ctx, objs[key_object], stm, _dev(gpu_ctx, aw), _dev(gpu_ctx, mw), {f: _dev(gpu_ctx, v) for f, v in pw.items()},
                      _dev(gpu_ctx, Xw) if check else None, _dev(gpu_ctx, uw) if check else None, _di(gpu_ctx, kidx), _di(gpu_ctx, sidx))
    got = [int(v) for v in ok.cpu().numpy()]
    w_ok = [int(v) for v in orc.bob_verify(*tabs, kidx, sidx, aw, mw, pw, Xw, uw)]
    rule = [int(H.valid(X[i]) and H.valid(uu[i])) if check else 1 for i in range(B)]
    assert got == [a & b for a, b in zip(w_ok, rule)]
    layout, marks = H.bob_layout(B, check), H.bob_rejected(B, check)
    nh = len(layout)
    assert [layout[i][0] for i in range(nh) if marks[i] and got[i] != 0] == []
    assert nh < B and got[nh:] == [1] * (B - nh) == w_ok[nh:]
    for i, (label, field, what) in enumerate(layout):
        if what == "DECISIVE":                                   # the oracle (no rule) accepts, the device must not
            assert (w_ok[i], rule[i], got[i]) == (1, 0, 0), label
    other = seen.setdefault((B, check), got)                     # the second key object to run finds the verdicts of the first
    assert other == got
