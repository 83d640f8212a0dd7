"""The case tables of the one-item-per-lane layer (csrc/mpe_fe.h, mpe_sc.h, mpe_jac.h, and the device-only SHA-256 of mpe_ec.h and word
helpers of mpe_small.h), and the checks that run over them.  Pure Python: no ctypes, no GPU.  A check takes `run(op, rows, arg=0)`, which
hands every row (a tuple of word lists) to one operation and returns one tuple of word lists per row; tests/test_fe_cpu.py runs the checks
through the host build (tools/model/fe_host.cpp, one call per row), tests/test_fe_gpu.py through the test-only device library
(tests/hip/ec_dev.hip, one launch per table).  The references are Python integers, hashlib and tests/pyref.py.
Tables are seeded and built once (functools.lru_cache); nothing mutates them."""
import functools
import hashlib
import random

import pyref as R

P, Q = R.P, R.Q
M26 = (1 << 26) - 1
QC = (1 << 256) - Q
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE

# operation -> (words per input column, words per output column).  None: the width is the call's `arg` (sch_reduce).  A column of one
# word carries a small integer (a magnitude, a factor, a mode) in, or a verdict out.
OPS = {
    "feh_mul": ((10, 10), (8, 10)), "feh_sqr": ((10,), (8, 10)), "feh_weak": ((10,), (10,)), "feh_normalize": ((10,), (8,)),
    "feh_is_zero": ((10,), (1,)), "feh_neg": ((10, 1), (10,)), "feh_from_words": ((8,), (10,)), "feh_inv": ((10,), (8,)),
    "feh_add": ((10, 10), (10,)), "feh_sub": ((10, 10, 1), (10,)), "feh_mul_int": ((10, 1), (10,)), "feh_eq": ((10, 10, 1), (1,)),
    "ech_mul": ((8, 16), (16,)), "ech_mul_w4": ((8, 16), (16,)), "ech_add": ((16, 16), (16,)), "ech_add_jac": ((8, 16, 8, 16), (16,)),
    "ech_eq": ((8, 16, 16), (1,)), "ech_eq_jac": ((8, 16, 8, 16, 1), (1,)), "ech_on_curve": ((16,), (1,)),
    "ech_neg": ((8, 16, 1), (16, 16)), "ech_mul_comb": ((8,), (16,)),                 # ech_mul_comb: arg = 0 (table of G) | 1 (of H2)
    "sch_split": ((8,), (8, 8, 2)), "sch_reduce": ((None,), (8,)), "sch_mul": ((8, 8), (8,)), "sch_inv": ((8,), (8,)),
    "sch_add": ((8, 8), (8,)), "sch_sub": ((8, 8), (8,)), "sch_neg": ((8,), (8,)),
}


def limbs_value(l):
    return sum(int(v) << (26 * i) for i, v in enumerate(l))


def words_value(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def to_words(x, n=8):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def canon_limbs(v):
    """v spread over 26-bit limbs, whatever is left in the top one"""
    return [(v >> (26 * i)) & M26 for i in range(9)] + [v >> 234]


def limb_bound(m):
    """an element of magnitude m: n[0..8] <= 2 m (2^26 - 1), n[9] <= 2 m (2^22 - 1)"""
    return [2 * m * M26] * 9 + [2 * m * ((1 << 22) - 1)]


def within(l, m):
    return all(0 <= int(v) <= h for v, h in zip(l, limb_bound(m)))


def rand_limbs(rng, m, mode):
    hi = limb_bound(m)
    if mode == "max":
        return hi
    if mode == "edge":
        return [rng.choice([0, 1, h - 1, h, h // 2]) for h in hi]
    return [rng.randrange(h + 1) for h in hi]


def pt_words(pt):
    return [0] * 16 if pt is None else to_words(pt[0]) + to_words(pt[1])


def words_pt(w):
    x, y = words_value(w[:8]), words_value(w[8:])
    return None if x == 0 and y == 0 else (x, y)


table = functools.lru_cache(maxsize=None)
ec_mul = table(R.ec_mul)          # a reference product is computed once, whichever test asks for it


# ---- base field ----------------------------------------------------------------------------------------------------------------------
MUL_PAIRS = [(1, 1), (1, 3), (3, 3), (3, 6), (2, 6), (5, 5), (5, 3), (1, 32), (4, 8), (2, 16), (3, 2)]


@table
def mul_sqr_tables():
    """(fe_mul rows (m1, m2, mode, a, b) for every magnitude pair the formulas use, fe_sqr rows (m, mode, a))"""
    rng = random.Random(1)
    mul, sqr = [], []
    for m1, m2 in MUL_PAIRS:
        for mode in ["max", "edge", "rand", "rand", "rand", "edge", "rand"] * 6:
            mul.append((m1, m2, mode, rand_limbs(rng, m1, mode), rand_limbs(rng, m2, mode if mode != "edge" else "rand")))
    for m in [1, 2, 3, 5]:
        for mode in ["max", "edge", "rand", "rand", "edge", "rand"] * 8:
            sqr.append((m, mode, rand_limbs(rng, m, mode)))
    return mul, sqr


def check_mul_sqr(run):
    mul, sqr = mul_sqr_tables()
    for (m1, m2, mode, a, b), (out, ol) in zip(mul, run("feh_mul", [(a, b) for _, _, _, a, b in mul])):
        assert words_value(out) == limbs_value(a) * limbs_value(b) % P, (m1, m2, mode)
        assert within(ol, 1), (m1, m2, mode)                       # the raw result is of magnitude 1 and congruent
        assert limbs_value(ol) % P == words_value(out)
    for (m, mode, a), (out, ol) in zip(sqr, run("feh_sqr", [(a,) for _, _, a in sqr])):
        assert words_value(out) == limbs_value(a) ** 2 % P, (m, mode)
        assert within(ol, 1), (m, mode)


NORMALIZE_SPECIALS = [0, 1, P - 1, P, P + 1, 2 * P, 2 * P - 1, (1 << 256) - 1, 1 << 256, (1 << 256) + (1 << 32) + 976, 3 * P, 31 * P]


@table
def normalize_tables():
    """(limbs of the special values, rows (m, mode, a) at every magnitude up to 31, limbs of k p for k < 60)"""
    rng = random.Random(2)
    specials = [(v, canon_limbs(v)) for v in NORMALIZE_SPECIALS if max(canon_limbs(v)) < 1 << 32]
    mags = [(m, mode, rand_limbs(rng, m, mode)) for m in [1, 2, 3, 6, 10, 17, 31] for mode in ["max", "edge", "rand", "rand", "rand"] * 10]
    return specials, mags, [canon_limbs(k * P) for k in range(60)]


def check_normalize_weak_zero_neg(run):
    specials, mags, multiples = normalize_tables()
    rows = [(l,) for _, l in specials]
    for (v, _), (out,), (z,) in zip(specials, run("feh_normalize", rows), run("feh_is_zero", rows)):
        assert words_value(out) == v % P, hex(v)
        assert z[0] == (1 if v % P == 0 else 0), hex(v)
    rows = [(a,) for _, _, a in mags]
    for (m, mode, a), (out,), (ol,), (z,) in zip(mags, run("feh_normalize", rows), run("feh_weak", rows), run("feh_is_zero", rows)):
        assert words_value(out) == limbs_value(a) % P
        assert limbs_value(ol) % P == limbs_value(a) % P
        assert all(v <= M26 for v in ol[:9]) and ol[9] <= (1 << 22) + 63
        assert z[0] == (1 if limbs_value(a) % P == 0 else 0)
    neg = [(m, a) for m, _, a in mags if m < 31]
    for (m, a), (ol,) in zip(neg, run("feh_neg", [(a, [m]) for m, a in neg])):
        assert (limbs_value(ol) + limbs_value(a)) % P == 0
        assert within(ol, m + 1)
    for (z,) in run("feh_is_zero", [(l,) for l in multiples]):      # multiples of p at every magnitude are recognised as zero
        assert z[0] == 1


@table
def words_table():
    rng = random.Random(3)
    return [0, 1, P - 1, (1 << 255) + 12345, 0xDEADBEEF << 200] + [rng.randrange(P) for _ in range(50)]


def check_words_roundtrip_and_inverse(run):
    vals = words_table()
    limbs = [ol for (ol,) in run("feh_from_words", [(to_words(v),) for v in vals])]
    for v, ol, (out,) in zip(vals, limbs, run("feh_normalize", [(ol,) for ol in limbs])):
        assert limbs_value(ol) == v and all(x <= M26 for x in ol)
        assert words_value(out) == v
    inv = [(v, k, [x * k for x in ol]) for v, ol in zip(vals, limbs) if v for k in [1, 2, 5]]
    for (v, k, _), (out,) in zip(inv, run("feh_inv", [(lk,) for _, _, lk in inv])):
        assert words_value(out) * v * k % P == 1


# fe_add / fe_sub / fe_mul_int / fe_eq at the magnitudes the comments of mpe_jac.h state:
#   jac_dbl       fe_add(1, 9), fe_add(4, 2), fe_add(1, 9); fe_mul_int(1, k) for k = 3, 8, 4, 8, 2
#   jac_add_tail  fe_add(1, 2) then (3, 3); fe_add(1, 2); fe_add(1, 2); fe_mul_int(1, 2)
#   jac_add[_affl] fe_sub(1, 1, 1), fe_sub(1, 3, 3);  jac_eq[_aff] fe_eq(1, 1, 1), fe_eq(1, 3, 3);  aff_on_curve fe_add(1, 1), fe_eq(1, 2, 2)
FE_ADD_MAGS = [(1, 9), (4, 2), (1, 2), (3, 3), (1, 1)]
FE_SUB_MAGS = [(1, 1), (1, 3), (1, 2)]
FE_MUL_INT = [(1, 3), (1, 8), (1, 4), (1, 2)]
FE_MODES = ["max", "edge", "rand", "rand", "edge", "rand", "max", "rand"]


@table
def fe_helper_tables():
    """(fe_add rows (ma, mb, a, b), fe_sub rows (ma, mb, a, b), fe_mul_int rows (m, k, a), fe_eq rows (mb, a, b, equal?))"""
    rng = random.Random(10)
    add = [(ma, mb, rand_limbs(rng, ma, mode), rand_limbs(rng, mb, mode)) for ma, mb in FE_ADD_MAGS for mode in FE_MODES * 3]
    sub = [(ma, mb, rand_limbs(rng, ma, mode), rand_limbs(rng, mb, mode)) for ma, mb in FE_SUB_MAGS for mode in FE_MODES * 4]
    # "max" both sides is a - a at the limb bound: the smallest results
    mint = [(m, k, rand_limbs(rng, m, mode)) for m, k in FE_MUL_INT for mode in FE_MODES * 3]
    eq = []
    for ma, mb in FE_SUB_MAGS:
        for mode in FE_MODES * 3:
            b = rand_limbs(rng, mb, mode)
            v = limbs_value(b) % P
            eq.append((mb, canon_limbs(v), b, True))                                            # the same value, canonical against lazy
            eq.append((mb, [x + y for x, y in zip(canon_limbs(v), canon_limbs(P))], b, True))   # ... plus p: still magnitude 1
            eq.append((mb, canon_limbs((v + 1) % P), b, False))
            eq.append((mb, canon_limbs((v + (1 << 26 * rng.randrange(10))) % P), b, False))
            a = rand_limbs(rng, ma, mode)
            eq.append((mb, a, b, limbs_value(a) % P == v))
        eq.append((mb, canon_limbs(0), canon_limbs(0), True))
        eq.append((mb, canon_limbs(0), canon_limbs(P), True))
        eq.append((mb, canon_limbs(P), canon_limbs(0), True))
        eq.append((mb, canon_limbs(1), canon_limbs(P), False))
    return add, sub, mint, eq


def check_fe_helpers(run):
    add, sub, mint, eq = fe_helper_tables()
    for (ma, mb, a, b), (ol,) in zip(add, run("feh_add", [(a, b) for _, _, a, b in add])):
        assert limbs_value(ol) % P == (limbs_value(a) + limbs_value(b)) % P and within(ol, ma + mb), (ma, mb)
    for (ma, mb, a, b), (ol,) in zip(sub, run("feh_sub", [(a, b, [mb]) for _, mb, a, b in sub])):
        assert limbs_value(ol) % P == (limbs_value(a) - limbs_value(b)) % P and within(ol, ma + mb + 1), (ma, mb)
    for (m, k, a), (ol,) in zip(mint, run("feh_mul_int", [(a, [k]) for _, k, a in mint])):
        assert limbs_value(ol) % P == limbs_value(a) * k % P and within(ol, m * k), (m, k)
    assert sum(1 for r in eq if r[3]) >= 100 and sum(1 for r in eq if not r[3]) >= 100
    for (mb, a, b, want), (v,) in zip(eq, run("feh_eq", [(a, b, [mb]) for mb, a, b, _ in eq])):
        assert v[0] == (1 if want else 0), (mb, a, b)


# ---- points --------------------------------------------------------------------------------------------------------------------------
@table
def point_tables():
    rng = random.Random(4)
    pts = [R.G, R.H2] + [ec_mul(rng.randrange(1, Q), R.G) for _ in range(6)]
    ks = [0, 1, 2, 3, 15, 16, 17, Q - 1, Q - 2, (1 << 255), (1 << 256) - 1, 0x1111111111111111111111111111111111111111111111111111111111111111,
          0xF0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0 % Q] + [rng.randrange(Q) for _ in range(12)]
    t = {"pts": pts, "ks": ks}
    t["mul"] = [(k % Q, pt) for pt in pts[:4] for k in ks]
    # mixed additions incl. the exceptional cases: P + P, P + (-P), P + inf, inf + P
    t["add"] = [(x, b) for a in pts[:4] for b in [a, R.ec_neg(a), None, pts[5], ec_mul(2, a)] for x in (a, None)]
    # general Jacobian addition of two computed points, incl. equal, opposite and infinite operands
    t["add_jac"] = [(3, pts[2], 5, pts[3]), (7, R.G, 7, R.G), (7, R.G, Q - 7, R.G), (0, R.G, 9, pts[4]), (9, pts[4], 0, R.G), (0, R.G, 0, R.G),
                    (2, R.G, 1, ec_mul(2, R.G))] + [(rng.randrange(Q), pts[2], rng.randrange(Q), pts[6]) for _ in range(6)]
    eq = []                                                        # projective equality: (k, P, Q, jac_eq_aff | jac_eq << 1)
    for k in [1, 2, 5, rng.randrange(Q)]:
        q = ec_mul(k, pts[3])
        eq += [(k, pts[3], q, 3), (k, pts[3], R.ec_neg(q), 0), (k, pts[3], pts[4], 0)]
    t["eq"] = eq + [(0, R.G, None, 3)]
    t["on_curve"] = [(c, w) for pt in pts for c, w in [(pt, 1), ((pt[0], (pt[1] + 1) % P), 0), (((pt[0] + 1) % P, pt[1]), 0)]]
    return t


def ref_mul(row):
    return ec_mul(words_value(row[0]), words_pt(row[1]))


def ref_add(row):
    return R.ec_add(words_pt(row[0]), words_pt(row[1]))


def check_scalar_multiplication_and_additions(run):
    t = point_tables()
    for (k, pt), (out,) in zip(t["mul"], run("ech_mul", [(to_words(k), pt_words(pt)) for k, pt in t["mul"]])):
        assert words_pt(out) == ec_mul(k, pt), hex(k)
    for (a, b), (out,) in zip(t["add"], run("ech_add", [(pt_words(a), pt_words(b)) for a, b in t["add"]])):
        assert words_pt(out) == R.ec_add(a, b)
    rows = [(to_words(ka), pt_words(pa), to_words(kb), pt_words(pb)) for ka, pa, kb, pb in t["add_jac"]]
    for (ka, pa, kb, pb), (out,) in zip(t["add_jac"], run("ech_add_jac", rows)):
        assert words_pt(out) == R.ec_add(ec_mul(ka, pa), ec_mul(kb, pb))
    for (k, p, q, want), (v,) in zip(t["eq"], run("ech_eq", [(to_words(k), pt_words(p), pt_words(q)) for k, p, q, _ in t["eq"]])):
        assert v[0] == want
    for (c, want), (v,) in zip(t["on_curve"], run("ech_on_curve", [(pt_words(c),) for c, _ in t["on_curve"]])):
        assert v[0] == want


@table
def neg_eq_tables():
    """(jac_neg rows (k, P, ladder?): -(k P) of a table entry (Z = 1; k is 1) or of a ladder output (Y of magnitude 3), infinity included;
    jac_eq rows (ka, P, kb, Q, ladder?, equal?))"""
    rng = random.Random(11)
    pts = point_tables()["pts"]
    neg = [(1, pt, 0) for pt in pts] + [(1, None, 0), (0, R.G, 1), (5, None, 1)]
    neg += [(k, pt, 1) for pt in pts[:4] for k in [1, 2, 3, Q - 1, LAMBDA, rng.randrange(Q), rng.randrange(Q), rng.randrange(Q), rng.randrange(Q)]]
    eq = []
    for pt in pts[:4]:
        for k in [1, 2, 7, Q - 1, rng.randrange(1, Q), rng.randrange(1, Q)]:
            j = rng.randrange(1, Q)
            base = ec_mul(j, pt)                                 # k P = (k / j) (j P): the same point through two different ladders
            eq += [(k, pt, k * pow(j, -1, Q) % Q, base, 1, True), (k, pt, k, pt, 1, True), (k, pt, (k + 1) % Q, pt, 1, False),
                   (k, pt, Q - k, pt, 1, False), (k, pt, k, pts[5], 1, False), (k, pt, 0, pt, 1, False)]
        eq += [(0, pt, 0, pts[4], 1, True), (0, pt, 3, None, 1, True), (1, pt, 1, pt, 0, True), (1, pt, 1, R.ec_neg(pt), 0, False),
               (1, pt, 1, pts[6], 0, False), (1, pt, 1, None, 0, False), (1, None, 1, None, 0, True)]
    return neg, eq


def check_neg_and_eq(run):
    neg, eq = neg_eq_tables()
    for (k, pt, lad), (out, zero) in zip(neg, run("ech_neg", [(to_words(k), pt_words(pt), [lad]) for k, pt, lad in neg])):
        assert words_pt(out) == R.ec_neg(ec_mul(k, pt) if lad else pt), (hex(k), lad)      # -(k P) against pyref.ec_neg
        assert words_pt(zero) is None, (hex(k), lad)                                           # k P + (-(k P)) = infinity
    rows = [(to_words(ka), pt_words(p), to_words(kb), pt_words(q), [lad]) for ka, p, kb, q, lad, _ in eq]
    for (ka, p, kb, q, lad, want), (v,) in zip(eq, run("ech_eq_jac", rows)):
        assert want == ((ec_mul(ka, p) == ec_mul(kb, q)) if lad else (p == q))             # the table states what pyref computes
        assert v[0] == (1 if want else 0), (hex(ka), hex(kb), lad)


COMB_ENTRIES = [(0, 1), (0, 15), (1, 1), (63, 15), (31, 7)]
COMB_ENTRIES_DEVICE = COMB_ENTRIES + [(63, 1), (32, 15)]


@table
def comb_table():
    """rows (base index, k): the scalars multiplied through the comb tables of G (0) and base_point2 (1)"""
    rng = random.Random(5)
    return [(g, k % Q) for g in (0, 1)
            for k in [0, 1, 15, 16, Q - 1, 1 << 255, 0x0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F]
            + [rng.randrange(Q) for _ in range(10)]
            # digit-0 windows at either end and all through, every digit value, one digit alone in the top window
            + [16 ** 63, 15 * 16 ** 63, 16 ** 32, 0xFEDCBA9876543210FEDCBA9876543210FEDCBA9876543210FEDCBA9876543210, Q - 16, 1 << 252]]


def check_comb_entries(tab, g, entries=COMB_ENTRIES):
    """tab: the 64 x 15 x 20 limbs of base g's table"""
    base = (R.G, R.H2)[g]
    for w, d in entries:
        e = tab[(w * 15 + d - 1) * 20:(w * 15 + d) * 20]
        assert (limbs_value(e[:10]), limbs_value(e[10:])) == ec_mul(d * 16 ** w, base), (g, w, d)


def ref_mul_comb(row, g):
    return ec_mul(words_value(row[0]), (R.G, R.H2)[g])


def check_comb_mul(run):
    for g in (0, 1):
        ks = [k for b, k in comb_table() if b == g]
        for k, (out,) in zip(ks, run("ech_mul_comb", [(to_words(k),) for k in ks], g)):
            assert words_pt(out) == ec_mul(k, (R.G, R.H2)[g]), hex(k)


GLV_EDGES = [0, 1, 2, 15, 16, 17, 31, 32, 33, Q - 1, Q - 2, LAMBDA, Q - LAMBDA, LAMBDA - 1, LAMBDA + 1, (LAMBDA * 16) % Q, (LAMBDA * 17 + 16) % Q,
             (1 << 128) - 1, 1 << 128, 0x10842108421084210842108421084210 % Q]


@table
def glv_tables():
    """(the scalars of the split check, (points, scalars) of the ladder check)"""
    rng = random.Random(7)
    split = [0, 1, 2, Q - 1, Q - 2, Q // 2, Q // 2 + 1, LAMBDA, Q - LAMBDA, LAMBDA + 1, (1 << 128), (1 << 128) - 1, (1 << 255)]
    split += [rng.randrange(Q) for _ in range(3000)]
    rng = random.Random(8)
    pts = [R.G, R.H2, ec_mul(rng.randrange(1, Q), R.G), None]     # infinity as the base, between the others
    return split, (pts, GLV_EDGES + [rng.randrange(Q) for _ in range(60)])


def check_glv_split(run):
    split, _ = glv_tables()
    for k, (r1, r2, neg) in zip(split, run("sch_split", [(to_words(k),) for k in split])):
        v1, v2 = words_value(r1), words_value(r2)
        assert v1 < 1 << 128 and v2 < 1 << 128
        assert ((-v1 if neg[0] else v1) + (-v2 if neg[1] else v2) * LAMBDA) % Q == k


def check_glv_ladder_matches_plain_ladder(run):
    pts, ks = glv_tables()[1]
    cases = [(k, pt) for pt in pts for k in ks]
    rows = [(to_words(k), pt_words(pt)) for k, pt in cases]
    for (k, pt), (out,), (out2,) in zip(cases, run("ech_mul", rows), run("ech_mul_w4", rows)):
        assert list(out) == list(out2), hex(k)
        assert words_pt(out) == ec_mul(k, pt), hex(k)


# ---- scalar field --------------------------------------------------------------------------------------------------------------------
def fold_model(t):
    """The three folds of sc_reduce512 on a 512-bit t, on Python integers: (result, ending).  ending: "carry" (the third fold leaves
    w[8] = 1), "ge" (w[8] = 0 and the 256 bits are >= q), "lt" (neither)."""
    assert 0 <= t < 1 << 512
    m = (1 << 256) - 1
    y = (t & m) + (t >> 256) * QC
    z = (y & m) + (y >> 256) * QC
    w = (z & m) + (z >> 256) * QC
    assert y < (1 << 385) + (1 << 256) and z < 1 << 260 and w < (1 << 256) + (1 << 134)       # the bounds the code's comments state
    if w >> 256:
        r, end = (w - Q) & m, "carry"
    elif w >= Q:
        r, end = w - Q, "ge"
    else:
        r, end = w, "lt"
    assert r == t % Q
    return r, end


def reduce16_model(x):
    """sc_reduce(x, 16): the top group is brought below q (one subtraction), then one sc_reduce512"""
    h = x >> 256
    return fold_model((x & ((1 << 256) - 1)) | ((h - Q if h >= Q else h) << 256))


def craft_reduce16(z, y_hi):
    """a 16-word x whose first fold gives y = (z - y_hi QC) + y_hi 2^256 and whose second fold gives z; the top group is below q"""
    y_lo = z - y_hi * QC
    h, lo = divmod(y_lo + (y_hi << 256), QC)
    return lo | h << 256 if 0 <= y_lo < 1 << 256 and h < Q else None     # (h < q bounds y_hi by 1.27 2^128 and z by 2.61 2^256)


@table
def reduce_endings():
    """16-word inputs of sc_reduce that take each ending of sc_reduce512, at the boundaries between them: (x, ending)"""
    out = []
    for y_hi in [1 << 128, (1 << 128) + 1, (1 << 128) - 1, (1 << 129) - 1, 3 << 127]:
        for z in [(1 << 257) - 1, (1 << 257) - QC, (1 << 257) - QC + 1, (3 << 256) - 1, (3 << 256) - 2 * QC,          # w[8] = 1, incl. w = 2^256
                  (1 << 257) - QC - 1, (3 << 256) - 2 * QC - 1, (1 << 256) + Q - QC, (1 << 256) - 1 + (1 << 256) - QC - QC,    # w in [q, 2^256)
                  (1 << 256) + Q - QC - 1, (1 << 256) + 12345, (1 << 257) + 99]:                                          # w < q
            x = craft_reduce16(z, y_hi)
            if x is not None:
                out.append((x, None))
    out += [(Q, "ge"), ((1 << 256) - 1, "ge"), (Q - 1, "lt"), (0, "lt"), (Q << 256, "lt"), (((Q - 1) << 256) | (1 << 256) - 1, None)]
    return [(x, end or reduce16_model(x)[1]) for x, end in out]


@table
def mul_endings():
    """(a, b, ending): factors below 2^256 whose product takes each ending of sc_reduce512.  "carry" needs a b = 2^256 + d (mod q) with
    the second fold landing on (k + 1) q + QC + d, k >= 1: b = (QC + d) / a mod q for seeded a, kept when the model says so."""
    rng = random.Random(12)
    out = [(1, Q, "ge"), (1, (1 << 256) - 1, "ge"), (1, Q - 1, "lt"), (0, 5, "lt")]
    want = {"carry": 6, "ge": 6}
    while any(want.values()):
        a = rng.randrange(1 << 255, 1 << 256) | 1
        if a % Q == 0:
            continue
        for end, d in (("carry", QC + rng.choice([0, 1, rng.randrange(1 << 128)])), ("ge", rng.choice([0, 1, QC - 1, rng.randrange(QC)]))):
            b = d * pow(a, -1, Q) % Q
            for bb in (b, b + Q):                                 # an unreduced second factor reaches other multiples of q
                if bb < 1 << 256 and want[end] and fold_model(a * bb)[1] == end:
                    out.append((a, bb, end))
                    want[end] -= 1
    return out


SC_EDGES = [0, 1, 2, Q - 1, Q, Q + 1, (1 << 256) - 1, (1 << 255), (1 << 128) - 1, 1 << 128, Q >> 1]
REDUCE_WIDTHS = [1, 5, 8, 9, 16, 24, 25, 64, 72, 88, 89, 90]


@table
def scalar_tables():
    rng = random.Random(6)
    t = {"reduce": {}}
    # reductions of every width the kernels use (8 .. 90 words), incl. all-ones inputs and multiples of q
    for n in REDUCE_WIDTHS:
        vals = [0, (1 << (32 * n)) - 1, (Q * ((1 << (32 * n)) // Q)) if n >= 8 else 0, ((1 << (32 * n)) // Q) * Q - 1 if n >= 8 else 1]
        t["reduce"][n] = vals + [rng.randrange(1 << (32 * n)) for _ in range(12)]
    mul = [(a % (1 << 256), b % (1 << 256)) for a in SC_EDGES for b in SC_EDGES + [rng.randrange(1 << 256) for _ in range(3)]]
    t["mul"] = mul + [(rng.randrange(1 << 256), rng.randrange(1 << 256)) for _ in range(300)]
    t["inv"] = [1, 2, Q - 1, Q - 2] + [rng.randrange(1, Q) for _ in range(20)]
    # the crafted inputs of the three endings in the low 16 words of every width that has them (zeros above: the last sc_reduce512 sees them)
    for n in REDUCE_WIDTHS:
        if n >= 16:
            t["reduce"][n] = t["reduce"][n] + [x for x, _ in reduce_endings()]
        elif n >= 8:
            t["reduce"][n] = t["reduce"][n] + [Q, Q - 1, Q + 1, (1 << 256) - 1]
    t["mul"] = t["mul"] + [(a, b) for a, b, _ in mul_endings()]
    return t


def ref_reduce(row):
    return words_value(row[0]) % Q


def check_fold_model():
    """every ending of sc_reduce512 is reached by a case of sch_reduce(n = 16) and by a case of sch_mul, and the tables say which"""
    for x, end in reduce_endings():
        assert reduce16_model(x) == (x % Q, end), hex(x)
    for a, b, end in mul_endings():
        assert fold_model(a * b) == (a * b % Q, end), (hex(a), hex(b))
    t = scalar_tables()
    assert {reduce16_model(x)[1] for x in t["reduce"][16]} == {"carry", "ge", "lt"}
    assert {fold_model(a * b)[1] for a, b in t["mul"]} == {"carry", "ge", "lt"}
    x = craft_reduce16((1 << 257) - 1, 1 << 128)                  # the construction this table started from
    assert x in t["reduce"][16] and reduce16_model(x)[1] == "carry"


def check_scalar_field(run):
    t = scalar_tables()
    for n, vals in t["reduce"].items():
        for v, (out,) in zip(vals, run("sch_reduce", [(to_words(v, n),) for v in vals], n)):
            assert words_value(out) == v % Q, (n, hex(v))
    for (a, b), (out,) in zip(t["mul"], run("sch_mul", [(to_words(a), to_words(b)) for a, b in t["mul"]])):
        assert words_value(out) == a * b % Q, (hex(a), hex(b))
    for a, (out,) in zip(t["inv"], run("sch_inv", [(to_words(a),) for a in t["inv"]])):
        assert words_value(out) * a % Q == 1


@table
def add_sub_table():
    """(the (a, b) of sc_add, the (a, b) of sc_sub, the a of sc_neg).  Reduced operands: the sum carries out of 2^256 or not, reaches q
    or not; a - b borrows or not; 0.  The call sites also hand over an operand as it was loaded (a nonce, a share: any 256-bit value)
    -- either operand of sc_add, the minuend of sc_sub (z = k - c sk), never the subtrahend and never sc_neg's -- beside one that is
    reduced: then the result is congruent and fits 256 bits (a + b - q < 2^256), and that is what is asked of those rows."""
    rng = random.Random(13)
    red = [0, 1, 2, QC, QC - 1, QC + 1, Q - QC, Q - 1, Q - 2, Q >> 1, (Q >> 1) + 1, (1 << 255), (1 << 255) + 1, (1 << 128) - 1, 1 << 128]
    red += [rng.randrange(Q) for _ in range(6)]
    raw = [Q, Q + 1, (1 << 256) - 1, (1 << 256) - 2, Q + QC - 1, rng.randrange(Q, 1 << 256), rng.randrange(Q, 1 << 256)]
    pairs = [(a, b) for a in red for b in red]                    # (q - 1) + (q - 1) carries out of 2^256; 2^255 + 2^255 is 2^256 itself
    sub = pairs + [(a, b) for a in raw for b in red[:13]]
    return sub + [(b, a) for a in raw for b in red[:13]], sub, red


def check_scalar_add_sub_neg(run):
    adds, subs, singles = add_sub_table()
    s = [a + b for a, b in adds if a < Q and b < Q]
    assert any(x > 1 << 256 for x in s) and any(Q < x < 1 << 256 for x in s) and any(x < Q for x in s) and Q in s and 1 << 256 in s
    assert any(a < b for a, b in subs) and any(a > b for a, b in subs) and any(a == b for a, b in subs)
    for op, pairs, f in (("sch_add", adds, lambda a, b: a + b), ("sch_sub", subs, lambda a, b: a - b)):
        for (a, b), (out,) in zip(pairs, run(op, [(to_words(a), to_words(b)) for a, b in pairs])):
            assert words_value(out) % Q == f(a, b) % Q, (op, hex(a), hex(b))
            if a < Q and b < Q:
                assert words_value(out) == f(a, b) % Q, (op, hex(a), hex(b))
    for a, (out,) in zip(singles, run("sch_neg", [(to_words(a),) for a in singles])):
        assert words_value(out) == -a % Q, hex(a)


# ---- layout of the device launches -----------------------------------------------------------------------------------------------------
def uniform_cases():
    """(kind, op, row, arg, reference): the exceptional kinds, each to be launched as 64 identical rows (the branch is then uniform
    across the wave; inside the tables the same kinds sit between ordinary rows, where the lanes diverge)"""
    G, w, pw = R.G, to_words, pt_words
    ends = {end: x for x, end in reduce_endings()}
    pt = lambda f: (lambda row: f(row))
    return [("inf + P", "ech_add", (pw(None), pw(G)), 0, pt(ref_add)), ("P + inf", "ech_add", (pw(G), pw(None)), 0, pt(ref_add)),
            ("P + P", "ech_add", (pw(R.H2), pw(R.H2)), 0, pt(ref_add)), ("P + (-P)", "ech_add", (pw(G), pw(R.ec_neg(G))), 0, pt(ref_add)),
            ("k = 0", "ech_mul", (w(0), pw(G)), 0, pt(ref_mul)), ("base at infinity", "ech_mul", (w(5), pw(None)), 0, pt(ref_mul)),
            ("comb k = 0", "ech_mul_comb", (w(0),), 0, lambda row: ref_mul_comb(row, 0)),
            ("digit-0 windows", "ech_mul_comb", (w(16 ** 63),), 1, lambda row: ref_mul_comb(row, 1)),
            ("reduce: carry", "sch_reduce", (w(ends["carry"], 16),), 16, ref_reduce),
            ("reduce: ge", "sch_reduce", (w(ends["ge"], 16),), 16, ref_reduce),
            ("reduce: lt", "sch_reduce", (w(ends["lt"], 16),), 16, ref_reduce)]


def check_uniform(run, rows=64):
    for kind, op, row, arg, ref in uniform_cases():
        want = ref(row)
        for (out,) in run(op, [row] * rows, arg):
            assert (words_value(out) if op == "sch_reduce" else words_pt(out)) == want, kind


# ---- SHA-256 and sm:: (device only) ----------------------------------------------------------------------------------------------------
SHA_NWORDS = [8, 64, 128, 129]


def sha_message(fields, zero_bytes):
    """what the device hashes for a row of fields (value, nwords, plus1): sha_bigint of each value (+ 1: the HF_BIGINT_PLUS1 shape)"""
    with R.use_encoding(R.Encoding(zero_bytes=zero_bytes)):
        return b"".join(R.to_bytes(v + p1) for v, _, p1 in fields)


def sha_ref(msg):
    return int.from_bytes(hashlib.sha256(msg).digest(), "big")


@table
def sha_bigint_rows():
    """rows of up to 14 fields (value, nwords, plus1).  For every L in 0 .. 200 one row of non-zero fields whose bytes add up to L, and
    one with a zero field among them (one more byte, or none under zero_bytes): under either setting every total length 0 .. 200 occurs.
    The fields' top words hold 1, 2, 3 and 4 bytes; they are stored in 8, 64, 128 and 129 words, the words above the value zero."""
    rng = random.Random(14)
    rows = []
    for total in range(201):
        for with_zero in (False, True):
            left, fields = total, []
            while left:
                n = left if len(fields) == 12 else min(left, rng.randrange(1, 21))
                if not fields and not with_zero:
                    n = min(left, total % 4 + 1)                                    # the four top-word lengths lead in turn
                fields.append((rng.randrange(1 << (8 * n - 8), 1 << (8 * n)), rng.choice([w for w in SHA_NWORDS if 4 * w >= n]), 0))
                left -= n
            if with_zero:
                fields.insert(rng.randrange(len(fields) + 1), (0, rng.choice(SHA_NWORDS), 0))
            rows.append(fields)
    rows.append([((1 << 2048) - 1, 64, 1)])                                         # 2^2048 - 1 + 1: 257 bytes out of 65 words
    rows.append([(0, 8, 1), ((1 << 4096) - 1, 128, 1), ((1 << 256) - 1, 8, 0)])
    rows.append([(0, w, 0) for w in SHA_NWORDS * 3] + [(0, 1, 0), (1, 1, 0)])       # 14 fields
    return rows


def check_sha_bigint_rows_cover_every_length():
    rows = sha_bigint_rows()
    for zb in (0, 1):
        lens = {len(sha_message(f, zb)) for f in rows}
        assert set(range(201)) <= lens and 257 in lens
    tops = {(len(R.to_bytes(v)) - 1) % 4 + 1 if v else 0 for f in rows for v, _, _ in f}
    assert tops == {0, 1, 2, 3, 4} and {w for f in rows for _, w, _ in f} >= set(SHA_NWORDS) and max(len(f) for f in rows) == 14


@table
def sha_point_rows():
    pts = point_tables()["pts"]
    return [[pts[(i + j) % 8] for j in range(1 + i % 3)] for i in range(66)]


SM_WIDTHS = [1, 8, 16, 24, 32, 64, 65, 128, 129]
SM_INV_WIDTHS = sorted(set(SM_WIDTHS + [3, 33]))       # the call sites' widths (32 and 64 are inv2adic's own), and two that are no power of two


@table
def sm_values():
    """per width n: all-ones, zero, one, a single top bit, random values"""
    rng = random.Random(15)
    return {n: [(1 << 32 * n) - 1, 0, 1, 1 << (32 * n - 1), (1 << 32 * n) - 2] + [rng.randrange(1 << 32 * n) for _ in range(4)]
            for n in sorted(set(SM_WIDTHS + SM_INV_WIDTHS))}
