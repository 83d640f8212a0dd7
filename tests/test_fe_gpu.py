"""-m gpu: the case tables of tests/fe_cases.py on the device.  tests/test_fe_cpu.py runs them through a g++ build of the headers;
here the same tables and the same checks go through tests/hip/libec_dev.so, which hipcc compiles from the same headers with the
product's flags -- ladders, inversions and the GLV split as out-of-line callees under amdgpu_waves_per_eu(2), the loops under
`#pragma unroll 1`: the code the product's kernels run, which the host build is not.  One launch per operation and table; every launch
has at least 65 rows (lanes 0, 63 and 64), the exceptional rows (infinity, P + P, P + (-P), k = 0, digit-0 windows, the three endings
of sc_reduce512) sit between ordinary ones in the same wave, and each exceptional kind is also launched as 64 identical rows (and
the same row once more in lane 64), where the branch is uniform across the wave.
Device-only parts -- the SHA-256 of mpe_ec.h, the word helpers of mpe_small.h, what ec_comb_build_kernel builds -- are compared
with hashlib, Python integers and pyref here and nowhere else."""
import ctypes
import hashlib
import shutil

import numpy as np
import pytest
import torch

import fe_cases as T
import hip_build
import pyref as R

pytestmark = pytest.mark.gpu
PTR = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib(gpu_ctx, tmp_path_factory):
    try:
        path = hip_build.build(str(tmp_path_factory.mktemp("ec_dev")))
    except Exception as e:
        pytest.fail(f"tests/hip/libec_dev.so is missing or stale and could not be built (hipcc: {shutil.which('hipcc')}): {e}")
    lib = ctypes.CDLL(path)
    for op in T.OPS:
        getattr(lib, "ecd_" + op).argtypes = [ctypes.c_int] + [PTR] * 8 + [ctypes.c_int]
    lib.ecd_comb_copy.argtypes = [PTR]
    lib.ecd_sha_bigints.argtypes = [ctypes.c_int, PTR, ctypes.c_uint32, PTR, PTR, ctypes.c_int]
    lib.ecd_sha_points.argtypes = [ctypes.c_int, PTR, ctypes.c_int, PTR, PTR, PTR, ctypes.c_int]
    lib.ecd_sm.argtypes = [ctypes.c_int, ctypes.c_int, PTR, ctypes.c_int, PTR, ctypes.c_int, PTR, ctypes.c_int, PTR, PTR, PTR]
    assert lib.ecd_comb_build() == 0                               # this library's own COMB, by its own ec_comb_build_kernel
    return lib


def to_dev(gpu_ctx, rows, width):
    """rows of `width` words -> device tensor [n, width]"""
    a = np.array(rows, dtype=np.uint32).reshape(len(rows), width)
    return torch.from_numpy(a.view(np.int32)).to(gpu_ctx.device)


def new(gpu_ctx, n, width):
    return torch.zeros((n, width), dtype=torch.int32, device=gpu_ctx.device)


def to_host(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def ptr(t):
    return PTR(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def run(gpu_ctx, lib):
    def run(op, rows, arg=0):
        wi, wo = T.OPS[op]
        rows = list(rows)
        n = max(len(rows), 65)
        padded = [rows[i % len(rows)] for i in range(n)]            # at least 65 rows: lanes 0, 63 and 64 of two waves
        ins = [to_dev(gpu_ctx, [r[k] for r in padded], w if w is not None else arg) for k, w in enumerate(wi)]
        outs = [new(gpu_ctx, n, w) for w in wo]
        torch.cuda.synchronize()
        rc = getattr(lib, "ecd_" + op)(n, *[ptr(t) for t in ins + [None] * (5 - len(ins)) + outs + [None] * (3 - len(outs))], arg)
        assert rc == 0, f"ecd_{op}: HIP error {rc}"
        host = [to_host(o) for o in outs]
        res = [tuple(h[i] for h in host) for i in range(n)]
        for i in range(len(rows), n):                              # the padding computes what its original did
            assert res[i] == res[i % len(rows)], (op, i)
        return res[:len(rows)]
    return run


def test_mul_sqr_all_magnitudes(run):
    T.check_mul_sqr(run)


def test_normalize_weak_zero_neg(run):
    T.check_normalize_weak_zero_neg(run)


def test_words_roundtrip_and_inverse(run):
    T.check_words_roundtrip_and_inverse(run)


def test_add_sub_mul_int_eq_at_the_magnitudes_of_the_point_formulas(run):
    T.check_fe_helpers(run)


def test_scalar_multiplication_and_additions(run):
    T.check_scalar_multiplication_and_additions(run)


def test_negation_and_projective_equality(run):
    T.check_neg_and_eq(run)


def test_comb_table_entries_and_products(gpu_ctx, lib, run):
    tab = new(gpu_ctx, 2, 64 * 15 * 20)
    torch.cuda.synchronize()
    assert lib.ecd_comb_copy(ptr(tab)) == 0
    tab = to_host(tab)
    for g in (0, 1):
        T.check_comb_entries(tab[g], g, T.COMB_ENTRIES_DEVICE)
    T.check_comb_mul(run)


def test_scalar_field(run):
    T.check_scalar_field(run)


def test_scalar_add_sub_neg(run):
    T.check_scalar_add_sub_neg(run)


def test_glv_split(run):
    T.check_glv_split(run)


def test_glv_ladder_matches_plain_ladder(run):
    T.check_glv_ladder_matches_plain_ladder(run)


def test_exceptional_kinds_as_uniform_batches(run):
    T.check_uniform(run)


def test_entry_points_refuse_bad_arguments(lib):
    assert lib.ecd_sch_reduce(65, None, None, None, None, None, None, None, None, 0) != 0
    assert lib.ecd_sch_reduce(65, None, None, None, None, None, None, None, None, 91) != 0
    assert lib.ecd_ech_mul_comb(65, None, None, None, None, None, None, None, None, 2) != 0
    assert lib.ecd_sm(0, 65, None, 129, None, 129, None, 257, None, None, None) != 0


# ---- SHA-256 ---------------------------------------------------------------------------------------------------------------------------
def test_sha256_of_bigint_chains_at_every_length(gpu_ctx, lib):
    rows = T.sha_bigint_rows()
    assert len(rows) >= 65
    data, desc = [], []
    for fields in rows:
        d = [len(fields)]
        for v, nw, p1 in fields:
            d += [len(data), nw, p1]
            data += T.to_words(v, nw)
        desc.append(d + [0] * (43 - len(d)))
    d_data, d_desc, out = to_dev(gpu_ctx, [data], len(data)), to_dev(gpu_ctx, desc, 43), new(gpu_ctx, len(rows), 8)
    for zb in (0, 1):
        torch.cuda.synchronize()
        assert lib.ecd_sha_bigints(len(rows), ptr(d_data), len(data), ptr(d_desc), ptr(out), zb) == 0
        for fields, got in zip(rows, to_host(out)):
            msg = T.sha_message(fields, zb)
            assert T.words_value(got) == T.sha_ref(msg), (zb, len(msg), [(nw, p1) for _, nw, p1 in fields])


def test_sha256_of_points_in_both_chain_forms_and_compressed(gpu_ctx, lib):
    rows = T.sha_point_rows()
    flat = [sum((T.pt_words(p) for p in r), []) + [0] * (16 * (3 - len(r))) for r in rows]
    pts, cnt = to_dev(gpu_ctx, flat, 48), to_dev(gpu_ctx, [[len(r)] for r in rows], 1)
    chain, comp = new(gpu_ctx, len(rows), 8), new(gpu_ctx, len(rows), 8)
    sha = lambda r, c: int.from_bytes(hashlib.sha256(b"".join(R.pt_bytes(p, c) for p in r)).digest(), "big")
    for form in (0, 1):
        torch.cuda.synchronize()
        assert lib.ecd_sha_points(len(rows), ptr(pts), 3, ptr(cnt), ptr(chain), ptr(comp), form) == 0
        for r, a, b in zip(rows, to_host(chain), to_host(comp)):
            assert T.words_value(a) == sha(r, bool(form)) and T.words_value(b) == sha(r, True), (form, len(r))


# ---- sm:: ------------------------------------------------------------------------------------------------------------------------------
def sm_call(gpu_ctx, lib, op, a, na, b, nb, nr, scratch=False):
    """(rows of r as integers, flags): one launch over the rows a[i], b[i]"""
    n = len(a)
    assert n >= 65
    d_a, d_b = to_dev(gpu_ctx, [T.to_words(v, na) for v in a], na), to_dev(gpu_ctx, [T.to_words(v, nb) for v in b], nb)
    r, flag = new(gpu_ctx, n, nr), new(gpu_ctx, n, 1)
    t1, t2 = (new(gpu_ctx, n, nr), new(gpu_ctx, n, nr)) if scratch else (None, None)
    torch.cuda.synchronize()
    assert lib.ecd_sm(op, n, ptr(d_a), na, ptr(d_b), nb, ptr(r), nr, ptr(flag), ptr(t1), ptr(t2)) == 0
    return [T.words_value(w) for w in to_host(r)], [f[0] for f in to_host(flag)]


@pytest.mark.parametrize("na, nb", [(n, n) for n in T.SM_WIDTHS] + [(16, 8), (8, 16), (65, 64), (128, 129), (24, 1)])
def test_sm_mul_mullo_add_sub_cmp(gpu_ctx, lib, na, nb):
    """the widths of the call sites in mpe_paillier.h, mpe_proofs.h, mpe_keygen.h and mpe_primes.h; all-ones, zero, a single top bit, random"""
    vals = T.sm_values()
    pairs = [(a, b) for a in vals[na] for b in vals[nb]]                            # 81 rows
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    n = max(na, nb)
    got, _ = sm_call(gpu_ctx, lib, 0, a, na, b, nb, na + nb)
    assert got == [x * y for x, y in pairs]
    got, carry = sm_call(gpu_ctx, lib, 2, a, na, b, nb, n)
    assert got == [(x + y) % (1 << 32 * n) for x, y in pairs] and carry == [(x + y) >> (32 * n) for x, y in pairs]
    got, borrow = sm_call(gpu_ctx, lib, 3, a, na, b, nb, n)
    assert got == [(x - y) % (1 << 32 * n) for x, y in pairs] and borrow == [1 if x < y else 0 for x, y in pairs]
    _, c = sm_call(gpu_ctx, lib, 4, a, na, b, nb, 1)
    assert c == [(x > y) - (x < y) & 0xFFFFFFFF for x, y in pairs]
    if na == nb:
        got, _ = sm_call(gpu_ctx, lib, 1, a, na, b, nb, n)
        assert got == [x * y % (1 << 32 * n) for x, y in pairs]
        assert {0, 1} <= set(carry) and {0, 1} <= set(borrow) and {0, 1, 0xFFFFFFFF} <= set(c)


@pytest.mark.parametrize("n", T.SM_INV_WIDTHS)
def test_sm_inv2adic(gpu_ctx, lib, n):
    """a inv2adic(a) = 1 mod 2^(32 n) for odd a, a = 1 and a = 2^(32 n) - 1 included; 3 and 33 words: the precision doubles past n"""
    import random
    rng = random.Random(16 + n)
    m = 1 << 32 * n
    a = [1, m - 1, 3 % m, (m >> 1) + 1] + [v | 1 for v in T.sm_values()[n]] + [rng.randrange(m) | 1 for _ in range(56)]
    got, _ = sm_call(gpu_ctx, lib, 5, a, n, a, n, n, scratch=True)
    for x, inv in zip(a, got):
        assert x * inv % m == 1, (n, hex(x))
