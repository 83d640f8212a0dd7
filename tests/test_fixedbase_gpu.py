"""The fixed-base ladder of h1 / h2 (`fb_modexp_kernel`, multi_party_ecdsa_amd/csrc/mpe_fixedbase.h) at every window width and
lane split, on the case table of tests/fb_cases.py: proofs byte-equal to the GMP oracle's field by field, z (and Bob's t) equal to
Python's pow, verdicts equal to the oracle's on the GPU's proofs AND on the oracle's (an error of the tables that prover and verifier
share would cancel in the first alone).  Then the three scheduler modes of the launch, the suite's ordinary route on the same rows,
and the width `mpe_gg20_keys_create` gives a key object under a memory budget, signing included.  Exact equality, no tolerance.
(tests/test_fb_cases_cpu.py proves the table reaches what it is named for.)"""
import functools

import numpy as np
import pytest
import torch

import fixtures as F
import fb_cases as FB
import gg20_fixture as G

pytestmark = pytest.mark.gpu


def E():
    from multi_party_ecdsa_amd import engine
    return engine


def npw(t):
    return np.ascontiguousarray(t.cpu().numpy().view(np.uint32))


def to_dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


@pytest.fixture(scope="module")
def pk(gpu_ctx):
    p = E().PaillierKeys(gpu_ctx, N=[k.N for k in F.load_keys()[:FB.PAILLIER_KEYS]])
    yield p
    p.close()


@pytest.fixture(scope="module")
def tables(request, gpu_ctx):
    """the statements of one window width with their tables, shared by every split (a statement set belongs to no context) and
    freed before the next width is built"""
    wb = request.param
    assert gpu_ctx.get_option("no_fixed_base") == 0               # else mpe_statements_create_wb builds no tables
    Nt, h1, h2 = FB.alice_case(wb).statements()
    stm = E().Statements(gpu_ctx, Nt, h1, h2, wb=wb)
    gpu_ctx.sync()
    yield wb, stm
    stm.close()


@pytest.fixture(scope="module")
def split_ctx():
    """contexts pinned to a lane split (option fb_split), made on first use and closed with the module"""
    made = {}

    def get(S):
        if S not in made:
            made[S] = E().Context(0, options={"fb_split": S})
            assert made[S].get_option("fb_split") == S == FB.split_of(1, S)
            assert made[S].get_option("no_fixed_base") == 0      # else every power would run on the variable-base ladder
        return made[S]
    yield get
    for c in made.values():
        c.close()


def differing_rows(got, want):
    return np.flatnonzero((got != want).any(axis=1)).tolist()


def alice_batch(ctx, pk, stm, case, B, what, oracle=True):
    """the first B rows of the case through alice_generate and alice_verify on `ctx`; oracle = False: z against Python alone and
    every proof accepted (honest rows whose reference proof nobody computed)"""
    e = E()
    i = {f: v[:B] for f, v in case.inputs().items()}
    di = lambda v: torch.tensor(v[:B], dtype=torch.int32, device=ctx.device)
    d_c = to_dev(ctx, i["c"])
    pr = e.alice_generate(ctx, pk, stm, to_dev(ctx, i["a"]), d_c, to_dev(ctx, i["r"]),
                          {f: to_dev(ctx, i[f]) for f in e.ALICE_NONCE_WORDS}, di(case.kidx), di(case.sidx))
    ctx.sync()
    got = {f: npw(v) for f, v in pr.items()}
    bad = [k for k, (g, w) in enumerate(zip(F.ints(got["z"]), case.python_z()[:B])) if g != w]
    assert not bad, f"{what}: z != h1^a h2^rho mod N~ (Python) on rows " + str([(k, case.rows[k].name, case.sidx[k]) for k in bad[:8]])
    if oracle:
        want = {f: v[:B] for f, v in case.expected().items()}
        for f in want:
            bad = differing_rows(got[f], want[f])
            assert not bad, f"{what}: field {f} differs from the oracle on rows " + str([(k, case.rows[k].name, case.sidx[k]) for k in bad[:8]])
        # the GPU's proofs, then the oracle's, each with the hostile rows' fields written in
        verdicts = list(case.expected_verdicts()[:B])
        proofs = [("its own", case.hostile(got)), ("the oracle's", case.hostile(want))]
    else:
        verdicts, proofs = [1] * B, [("its own", got)]               # honest rows only: accepted by design
    for whose, proof in proofs:
        ok = e.alice_verify(ctx, pk, stm, d_c, {f: to_dev(ctx, v) for f, v in proof.items()}, di(case.kidx), di(case.sidx))
        ctx.sync()
        ok = ok.cpu().numpy().tolist()
        bad = [k for k in range(B) if ok[k] != verdicts[k]]
        assert not bad, f"{what}: alice_verify on {whose} proofs differs from the oracle's verdict on rows " + \
            str([(k, case.rows[k].name, case.sidx[k], ok[k]) for k in bad[:8]])


@pytest.mark.parametrize("S", FB.SPLITS)
@pytest.mark.parametrize("tables", FB.WIDTHS, indirect=True)
def test_alice_proofs_at_every_width_and_split(pk, tables, split_ctx, S):
    """batches of one item, a full wave, a wave and one item, 37 rows: the planted digits of every exponent width (8, 24, 72, 88 words
    in the prover, 25 and 89 in the verifier) on S lane groups per item"""
    wb, stm = tables
    case = FB.alice_case(wb)
    ctx = split_ctx(S)
    for B in FB.batch_sizes(S):
        alice_batch(ctx, pk, stm, case, B, f"wb = {wb}, S = {S}, B = {B}")


@pytest.mark.parametrize("S", FB.BOB_SPLITS)
@pytest.mark.parametrize("tables", FB.BOB_WIDTHS, indirect=True)
def test_bob_proofs_add_the_64_80_and_81_word_exponents(pk, tables, split_ctx, S):
    """BobProof launches the ladder with beta' (64 words) and gamma (80 words) and, in the verifier, t1 (81 words): a wave and one
    item, then all 18 rows; t = h1^beta' h2^sigma against Python, every field against the oracle, both sides' proofs accepted"""
    e = E()
    wb, stm = tables
    case = FB.bob_case(wb)
    ctx = split_ctx(S)
    want, verdicts = case.expected(), case.expected_verdicts()
    for B in (FB.GROUPS // S + 1, case.B):
        what = f"wb = {wb}, S = {S}, B = {B}"
        i = {f: to_dev(ctx, v[:B]) for f, v in case.inputs().items()}
        di = lambda v: torch.tensor(v[:B], dtype=torch.int32, device=ctx.device)
        pr, _ = e.bob_generate(ctx, pk, stm, i["a_enc"], i["mta"], i["b"], i["beta_prim"], i["r"], {f: i[f] for f in e.BOB_NONCE_WORDS},
                               False, di(case.kidx), di(case.sidx))
        ctx.sync()
        got = {f: npw(v) for f, v in pr.items()}
        bad = [k for k, (g, w) in enumerate(zip(F.ints(got["t"]), case.python_t()[:B])) if g != w]
        assert not bad, f"{what}: t != h1^beta' h2^sigma mod N~ (Python) on rows " + str([(k, case.names[k]) for k in bad[:8]])
        for f in want:
            bad = differing_rows(got[f], want[f][:B])
            assert not bad, f"{what}: field {f} differs from the oracle on rows " + str([(k, case.names[k], case.sidx[k]) for k in bad[:8]])
        for whose, proof in (("its own", got), ("the oracle's", {f: v[:B] for f, v in want.items()})):
            ok = e.bob_verify(ctx, pk, stm, i["a_enc"], i["mta"], {f: to_dev(ctx, v) for f, v in proof.items()}, None, None,
                              di(case.kidx), di(case.sidx))
            ctx.sync()
            assert ok.cpu().numpy().tolist() == list(verdicts[:B]) == [1] * B, f"{what}: bob_verify on {whose} proofs"


@pytest.mark.parametrize("tables", [FB.SCHED_WB], indirect=True)
def test_every_scheduler_mode_hands_out_every_unit(pk, tables):
    """one item per wave and one wave per compute unit: cap // 2 items elect primaries, one more runs static units, cap + 3 pull
    every unit from the queue.  z against Python on EVERY row: a scheduling bug lives in particular units."""
    wb, stm = tables
    cap = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = FB.sched_sizes(cap)
    assert [FB.sched_mode(FB.units_of(B, 16), cap)[0] for B in sizes] == ["primaries", "static", "queue"]
    case = FB.sched_case(sizes[-1])
    ctx = E().Context(0, options=FB.SCHED_OPTIONS)
    try:
        assert (ctx.get_option("fb_split"), ctx.get_option("waves_per_cu"), ctx.get_option("no_fixed_base")) == (16, 1, 0)
        for B in sizes:
            alice_batch(ctx, pk, stm, case, B, f"scheduler mode {FB.sched_mode(FB.units_of(B, 16), cap)[0]}, B = {B}", oracle=False)
    finally:
        ctx.close()


def test_the_ordinary_route_gives_the_same_bytes(gpu_ctx, pk):
    """statements made the way the rest of the suite makes them (the context's width, the split chosen per launch) on the 13-bit
    rows: the oracle's bytes again, so the cases above are tied to the route the other tests pin"""
    case = FB.alice_case(FB.FB_WINDOW_BITS)
    assert gpu_ctx.get_option("fb_window_bits") == FB.FB_WINDOW_BITS and gpu_ctx.get_option("fb_split") == 0
    assert gpu_ctx.get_option("no_fixed_base") == 0
    stm = E().Statements(gpu_ctx, *case.statements())
    try:
        alice_batch(gpu_ctx, pk, stm, case, case.B, "the ordinary route")
    finally:
        stm.close()


@functools.lru_cache(maxsize=None)
def _gg20_reference():
    lk = G.make_local_keys(F.load_keys(), 1, 3, [0, 2])
    nonces = G.make_nonces(lk, 3, seed="fb-budget")
    return lk, nonces, G.oracle_sign(lk, nonces, 3)


@pytest.mark.parametrize("options", [{"fb_budget_mb": mb} for mb in FB.BUDGETS_MB] + [{"no_fixed_base": 1}], ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_gg20_keys_pick_the_width_the_budget_allows_and_sign(options):
    """t = 1, n = 3: budgets of 1, 20 and 200 MB give no tables (the variable-base ladder inside GG20 signing), 4-bit and 8-bit tables;
    option no_fixed_base gives none either.  Three sessions signed at each: the oracle's r, s, recid, R and status byte for byte."""
    e = E()
    lk, nonces, (wr, ws, wrecid, wR, wstatus) = _gg20_reference()
    ctx = e.Context(0, options=options)
    gk = None
    try:
        gk = e.Gg20Keys(ctx, 1, 3, [0, 2], lk["arrays"])
        budget = ctx.get_option("fb_budget_mb") << 20             # 0: a quarter of the free memory, which three statements fit at any width
        want_wb = FB.select_width(3, budget if budget else 1 << 62, start=ctx.get_option("fb_window_bits"),
                                  fixed_base=not ctx.get_option("no_fixed_base"))
        assert want_wb == (FB.BUDGETS_MB[options["fb_budget_mb"]] if "fb_budget_mb" in options else 0)
        assert gk.fb_window_bits() == want_wb
        r, s, recid, status, R = [o.cpu().numpy() for o in e.gg20_sign(ctx, gk, {f: to_dev(ctx, v) for f, v in nonces.items()}, 3, want_R=True)]
        ctx.sync()
        assert list(status) == [0] * 3 == list(wstatus)
        assert np.array_equal(r.view(np.uint32), wr) and np.array_equal(s.view(np.uint32), ws) and list(recid) == list(wrecid)
        assert np.array_equal(R.view(np.uint32), wR)
    finally:
        if gk is not None:
            gk.close()
        ctx.close()
