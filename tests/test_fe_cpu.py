"""The device field / scalar / point code (csrc/mpe_fe.h, mpe_sc.h, mpe_jac.h) compiled for the HOST and run over the case tables of
tests/fe_cases.py against Python integers and tests/pyref.py: the 10 x 26-bit lazy-reduction limb algorithms at every magnitude the
point formulas use and at the worst-case limb patterns, the scalar field at every ending of its reduction, and whole scalar
multiplications (variable base, comb table, exceptional additions, negation, projective equality).  No GPU involved: this is the same
header text hipcc compiles for gfx950, NOT the same code — tests/test_fe_gpu.py runs the same tables and the same checks on the device."""
import ctypes
import os
import subprocess

import pytest

import fe_cases as T
import pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
LAMBDA, BETA = T.LAMBDA, T.BETA

# how fe_host.cpp takes each operation of fe_cases.OPS: i<n> an input column (pointer), v<n> an input column of one word by value,
# o<n> an output column (pointer), r the int it returns (the only output column), n the call's arg (sch_reduce's width), t the comb table
HOST_CALLS = {
    "feh_mul": "i0 i1 o0 o1", "feh_sqr": "i0 o0 o1", "feh_weak": "i0 o0", "feh_normalize": "i0 o0", "feh_is_zero": "i0 r",
    "feh_neg": "i0 v1 o0", "feh_from_words": "i0 o0", "feh_inv": "i0 o0", "feh_add": "i0 i1 o0", "feh_sub": "i0 i1 v2 o0",
    "feh_mul_int": "i0 v1 o0", "feh_eq": "i0 i1 v2 r", "ech_mul": "i0 i1 o0", "ech_mul_w4": "i0 i1 o0", "ech_add": "i0 i1 o0",
    "ech_add_jac": "i0 i1 i2 i3 o0", "ech_eq": "i0 i1 i2 r", "ech_eq_jac": "i0 i1 i2 i3 v4 r", "ech_on_curve": "i0 r",
    "ech_neg": "i0 i1 v2 o0 o1", "ech_mul_comb": "i0 t o0", "sch_split": "i0 o0 o1 o2", "sch_reduce": "i0 n o0", "sch_mul": "i0 i1 o0",
    "sch_inv": "i0 o0", "sch_add": "i0 i1 o0", "sch_sub": "i0 i1 o0", "sch_neg": "i0 o0",
}


def arr(vals, n):
    return (ctypes.c_uint32 * n)(*vals)


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(ROOT, "build", "libfe_host.so")
    src = os.path.join(ROOT, "tools", "model", "fe_host.cpp")
    inc = os.path.join(ROOT, "multi_party_ecdsa_amd", "csrc")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [src, os.path.join(inc, "mpe_fe.h"), os.path.join(inc, "mpe_jac.h"), os.path.join(inc, "mpe_sc.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-DMPE_FE_HOST", "-I", inc, src, "-o", out])
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def comb(lib):
    """the comb tables of G and base_point2, built by the host twin of ec_comb_build_kernel"""
    tabs = []
    for base in (R.G, R.H2):
        tab = (ctypes.c_uint32 * (64 * 15 * 20))()
        lib.ech_comb_build(arr(T.pt_words(base), 16), tab)
        tabs.append(tab)
    return tabs


@pytest.fixture(scope="module")
def run(lib, comb):
    assert set(HOST_CALLS) == set(T.OPS)

    def run(op, rows, arg=0):
        wi, wo = T.OPS[op]
        fn, spec, res = getattr(lib, op), HOST_CALLS[op].split(), []
        for row in rows:
            outs = [arr([0] * w, w) for w in wo]
            args = []
            for s in spec:
                k = int(s[1:]) if len(s) > 1 else 0
                if s[0] == "i":
                    args.append(arr(row[k], len(row[k])))
                    assert len(row[k]) == (wi[k] if wi[k] is not None else arg)
                elif s[0] == "v":
                    args.append(ctypes.c_uint32(row[k][0]))
                elif s[0] == "o":
                    args.append(outs[k])
                elif s[0] == "n":
                    args.append(ctypes.c_int(arg))
                elif s[0] == "t":
                    args.append(comb[arg])
            ret = fn(*args)
            res.append(([ret],) if "r" in spec else tuple(list(o) for o in outs))
        return res
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


def test_comb_tables(run, comb):
    for g in (0, 1):
        T.check_comb_entries(list(comb[g]), g)
    T.check_comb_mul(run)


def test_fold_model_reaches_every_ending_of_sc_reduce512():
    T.check_fold_model()


def test_scalar_field(run):
    T.check_scalar_field(run)


def test_scalar_add_sub_neg(run):
    T.check_scalar_add_sub_neg(run)


def test_glv_constants_and_split(run):
    """the endomorphism constants are re-derived here from the lattice basis; the device split is exact and 128-bit"""
    n, p = R.Q, R.P
    assert pow(LAMBDA, 3, n) == 1 and LAMBDA != 1 and pow(BETA, 3, p) == 1 and BETA != 1
    assert R.ec_mul(LAMBDA, R.G) == (BETA * R.G[0] % p, R.G[1])
    a1, b1 = 0x3086D221A7D46BCDE86C90E49284EB15, -0xE4437ED6010E88286F547FA90ABFE4C3
    a2, b2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8, a1
    assert (a1 + b1 * LAMBDA) % n == 0 and (a2 + b2 * LAMBDA) % n == 0
    g1, g2 = (2 * (b2 << 384) + n) // (2 * n), (2 * ((-b1) << 384) + n) // (2 * n)
    src = open(os.path.join(ROOT, "multi_party_ecdsa_amd", "csrc", "mpe_sc.h")).read()

    def const(name):
        body = src[src.index(name + "[8] = {") + len(name) + 7:]
        return T.words_value([int(t.strip().rstrip("u"), 16) for t in body[:body.index("}")].split(",")])
    assert const("GLV_LAMBDA") == LAMBDA and const("GLV_BETA") == BETA
    assert const("GLV_G1") == g1 and const("GLV_G2") == g2
    assert const("GLV_MB1") == (-b1) % n and const("GLV_MB2") == (-b2) % n
    T.check_glv_split(run)


def test_glv_ladder_matches_plain_ladder(run):
    T.check_glv_ladder_matches_plain_ladder(run)


def test_exceptional_kinds_one_call_each(run):
    T.check_uniform(run, rows=1)                                  # (the device launches each as a whole wave of identical rows)


def test_sha_rows_cover_every_length_and_field_shape():
    T.check_sha_bigint_rows_cover_every_length()
