"""-m gpu: the PRODUCT's own copies of the one-item-per-lane layer, through the C-ABI, on the case tables of tests/fe_cases.py.
tests/hip/libec_dev.so (tests/test_fe_gpu.py) is a compile of its own; the out-of-line ladders, the scalar reduction and the SHA-256
inside libmpecdsa_hip.so see the same edge tables here: the GLV and scalar edge lists against G, base_point2, a random point and
infinity as the base; the comb scalars and every reduction width the ABI takes, the crafted inputs of the three endings of
sc_reduce512 included; every ordered pair of {inf, P, -P, 2P, Q}; the sc_mul edge table; the hash commitment at every pair of byte
lengths, which drives the SHA-256 through every one-block and two-block padding edge under both zero_bytes profiles."""
import hashlib
import random

import pytest

import fe_cases as T
import pyref as R

pytestmark = pytest.mark.gpu
ABI_REDUCE_WIDTHS = [1, 5, 8, 9, 16, 24, 25, 64, 72, 88, 89]


def E():
    from multi_party_ecdsa_amd import engine
    return engine


def points_dev(ctx, pts):
    return E().dev(ctx, [T.words_value(T.pt_words(p)) for p in pts], 16)


def points_host(t):
    return [T.words_pt(T.to_words(v, 16)) for v in E().host(t)]


def test_ec_mul_glv_and_edge_scalars_on_four_bases_infinity_included(gpu_ctx):
    pts, ks = T.glv_tables()[1]
    ks = ks + [k % R.Q for k in T.point_tables()["ks"]]
    assert pts[:2] == [R.G, R.H2] and pts[3] is None
    cases = [(k, pt) for k in ks for pt in pts]                                     # the bases alternate inside every wave
    got = E().ec_mul(gpu_ctx, E().dev(gpu_ctx, [k for k, _ in cases], 8), points_dev(gpu_ctx, [p for _, p in cases]))
    for (k, pt), g in zip(cases, points_host(got)):
        assert g == T.ec_mul(k, pt), (hex(k), pt)


def test_ec_mul_base_comb_scalars_and_every_reduction_width(gpu_ctx):
    ks = [k for g, k in T.comb_table() if g == 0]
    got = points_host(E().ec_mul_base(gpu_ctx, E().dev(gpu_ctx, ks, 8)))
    assert got == [T.ec_mul(k, R.G) for k in ks]
    red = T.scalar_tables()["reduce"]
    ends = {T.reduce16_model(x)[1] for x in red[16]}
    assert ends == {"carry", "ge", "lt"}
    for n in ABI_REDUCE_WIDTHS:
        got = points_host(E().ec_mul_base(gpu_ctx, E().dev(gpu_ctx, red[n], n)))
        assert got == [T.ec_mul(v % R.Q, R.G) for v in red[n]], n
    N = E().N_
    k, out = E().dev(gpu_ctx, [1] * 4, 90), E().dev(gpu_ctx, [0] * 4, 16)
    for bad in (90, 0):
        assert N.lib.mpe_ec_mul_base(gpu_ctx.h, 4, E()._ptr(k), bad, E()._ptr(out), gpu_ctx.stream()) == N.MPE_E_ARG


def test_ec_add_every_ordered_pair_of_special_operands(gpu_ctx):
    pts = T.point_tables()["pts"]
    pairs = []
    for P, Q in [(R.G, pts[4]), (pts[2], R.H2), (pts[3], pts[5])]:
        ops = [None, P, R.ec_neg(P), T.ec_mul(2, P), Q]
        pairs += [(a, b) for a in ops for b in ops]                                 # every pair in both orders, the diagonal too
    got = points_host(E().ec_add(gpu_ctx, points_dev(gpu_ctx, [a for a, _ in pairs]), points_dev(gpu_ctx, [b for _, b in pairs])))
    assert got == [R.ec_add(a, b) for a, b in pairs]


def test_scalar_mul_edge_table(gpu_ctx):
    mul = T.scalar_tables()["mul"]
    got = E().host(E().scalar_mul(gpu_ctx, E().dev(gpu_ctx, [a for a, _ in mul], 8), E().dev(gpu_ctx, [b for _, b in mul], 8)))
    assert got == [a * b % R.Q for a, b in mul]
    # the ABI reduces both factors as it reads them: the crafted products of all three endings have factors below q and stay as they are
    assert {T.fold_model((a % R.Q) * (b % R.Q))[1] for a, b in mul} == {"carry", "ge", "lt"}


def test_hash_commit_bigint_at_every_pair_of_byte_lengths(gpu_ctx):
    rng = random.Random(17)
    val = lambda nbytes: rng.randrange(1 << (8 * nbytes - 8), 1 << (8 * nbytes)) if nbytes else 0
    rows = [(val(i), val(j)) for i in range(33) for j in range(33)]                 # 1089 rows, one launch per profile
    m, blind = E().dev(gpu_ctx, [a for a, _ in rows], 8), E().dev(gpu_ctx, [b for _, b in rows], 8)
    default = gpu_ctx.encoding()
    try:
        for zb in (0, 1):
            gpu_ctx.set_encoding(dict(default, zero_bytes=zb))
            got = E().host(E().hash_commit_bigint(gpu_ctx, m, blind))
            with R.use_encoding(R.Encoding(zero_bytes=zb)):
                msgs = [R.to_bytes(a) + R.to_bytes(b) for a, b in rows]
            assert {0 if zb else 2, 55, 56, 63, 64} <= {len(x) for x in msgs}
            assert got == [int.from_bytes(hashlib.sha256(x).digest(), "big") for x in msgs], zb
    finally:
        gpu_ctx.set_encoding(default)
