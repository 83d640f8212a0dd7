"""The hostile-input table (tests/hostile_cases.py) proved without a GPU: every point is what its kind says, every guarded point argument
of every call has a DECISIVE row (accepted by the unguarded Python verifier, refused by the validity rule alone), the scalar and residue
rows carry the oracle's verdicts, and what the oracle's own stand-alone verifiers answer on the point rows is recorded row by row.  The
oracle's verifiers have no deserialisation rule (by design: pt_in only knows the all-zero row), so on a decisive row the oracle says 1 and
the rule says 0 — asserted here as exactly that, so that the divergence stays explicit.  Points: the Python rule is the anchor; scalars and
residues: the oracle is."""
import ctypes as C

import numpy as np
import pytest

import fixtures as F
import hostile_cases as H
import orc
import pyref

# the guarded point arguments of the calls the GPU test makes (the `aff_valid` sites of mpe_proofs.h, mpe_sigma.h, mpe_blame.h, mpe_mta.h)
GUARDED = dict(dlog=("pk", "R"), pedersen=("com", "a1", "a2"), heg=("G", "H", "Y", "D", "E", "T", "A3"),
               ecddh=("g1", "h1", "g2", "h2", "a1", "a2"), pdl=("G", "Q", "u1"), mta=("pk", "R", "tpk", "tR"),
               blame7=("R", "Rd0", "S0", "Rd1", "S1"))


def _ok(n):
    return np.zeros(n, dtype=np.uint8)


def oracle_verdicts(name):
    """the oracle's stand-alone verifier on every row of the case, from the interface words"""
    c = H.EC_CASES[name]()
    w = lambda f: H.words(c, f)
    ok = _ok(H.B)
    if name == "dlog":
        return list(orc.dlog_verify(w("pk"), w("R"), w("z")))
    if name == "pedersen":
        orc.lib.orc_pedersen_verify(H.B, *[orc._p(a) for a in (w("com"), w("a1"), w("a2"), w("z1"), w("z2"), ok)])
    elif name == "heg":
        orc.lib.orc_heg_verify(H.B, *[orc._p(a) for a in [w(f) for f in ("G", "H", "Y", "D", "E", "T", "A3", "z1", "z2")] + [ok]])
    elif name == "ecddh":
        orc.lib.orc_ecddh_verify(H.B, *[orc._p(a) for a in [w(f) for f in ("g1", "h1", "g2", "h2", "a1", "a2", "z")] + [ok]])
    elif name == "pdl":
        keys = F.load_keys()
        tabs = [F.words([k.N for k in keys[:H.PDL_KEYS]], 64)] + [F.words([getattr(k, f) for k in keys[4:4 + H.PDL_STATEMENTS]], 64) for f in ("Nt", "h1", "h2")]
        return list(orc.pdl_verify(*tabs, c.col("kidx"), c.col("sidx"), w("c"), w("Q"), w("G"), {f: w(f) for f in ("z", "u1", "u2", "u3", "s1", "s2", "s3")}))
    elif name == "mta":
        # MessageB::verify_proofs_get_alpha composed of the oracle's primitives: two DLogProof::verify and a b_pk + beta_tag_pk == alpha G
        alpha = F.words([s % pyref.Q for s in c.col("share")], 8)
        rel = [np.array_equal(x, y) for x, y in zip(orc.ec_add(orc.ec_mul(w("a"), w("pk")), w("tpk")), orc.ec_mul_base(alpha))]
        return [int(a and b and r) for a, b, r in zip(orc.dlog_verify(w("pk"), w("R"), w("z")), orc.dlog_verify(w("tpk"), w("tR"), w("tz")), rel)]
    elif name == "blame7":
        return list(oracle_blame7(c))
    return list(ok)


def blame7_opened(c):
    """the [B S] layout of mpe_gg20_blame7_in from the session rows"""
    both = lambda f0, f1: np.ascontiguousarray(np.stack([H.words(c, f0), H.words(c, f1)], axis=1).reshape(H.B * H.BLAME7_S, -1))
    return dict(s=both("s0", "s1"), r=H.words(c, "r"), R_dash=both("Rd0", "Rd1"), m=H.words(c, "m"), R=H.words(c, "R"), S=both("S0", "S1"))


def oracle_blame7(c):
    o = blame7_opened(c)
    keep = [np.ascontiguousarray(o[f]) for f in ("s", "r", "R_dash", "m", "R", "S")]
    st = (C.c_void_p * 6)(*[a.ctypes.data for a in keep])
    bad = np.zeros(H.B, dtype=np.uint32)
    orc.lib.orc_gg20_blame7(H.BLAME7_S, H.B, st, orc._p(bad))
    return bad


def test_point_kinds_are_what_they_say():
    for x in (1, 2, 3, 4):                                   # x^3 + 7 is a square for each: the NONCANON_X pool exists
        pt = H.lift(x)
        assert pt is not None and H.valid(pt) and x + H.P < 1 << 256
    assert len(set(H.NONCANON)) == 4 and all(H.kind_holds("NONCANON_X", p) for p in H.NONCANON)
    assert H.TWIST_B != 7 and len(set(H.TWIST)) == len(H.TWIST) and all(H.kind_holds("TWIST", p) for p in H.TWIST)
    r = F.Rng("hostile-kinds")
    for i in range(8):
        pt = pyref.ec_mul(r.below(H.Q - 1) + 1, H.G)
        for kind in H.KINDS:
            hp = H.kind_point(kind, pt, i)
            assert H.kind_holds(kind, hp), (kind, hp)
            assert H.valid(hp) == (kind == "NEG")
            assert all(0 <= v < 1 << 256 for v in hp)
    assert H.valid(H.G) and H.valid(H.H2) and not H.valid((0, 0))
    # the raw hash of the neutral row is 04 and 64 zero bytes; of a NONCANON_X row, the bytes of x + p
    import hashlib
    assert H.chain_scalar([(0, 0)]) == int.from_bytes(hashlib.sha256(b"\x04" + bytes(64)).digest(), "big") % H.Q
    assert H.chain_scalar([H.NONCANON[0]]) != H.chain_scalar([H.red(H.NONCANON[0])])


@pytest.mark.parametrize("name", sorted(H.EC_CASES))
def test_table_invariants(name):
    c = H.EC_CASES[name]()
    assert len(c.labels) == H.B and c.points == GUARDED[name]
    hostile = [i for i in range(H.B) if c.labels[i] != "honest"]
    assert set(H.EDGE_LANES) <= set(hostile) and 3 * len(c.honest) >= H.B          # lanes 0, 63, 64 are hostile; a third is honest
    assert len(set(i // 8 for i in hostile)) == 9                                  # ... and spread: every run of eight lanes holds one
    for i in c.honest:
        assert c.want[i] == c.unguarded[i] == c.honest_value and c.invalid_args(i) == ()
    for i in hostile:
        label = c.labels[i]
        if label.startswith("scalar "):
            assert c.invalid_args(i) == () and c.want[i] == c.unguarded[i] != c.honest_value, label      # all rejections, by the algebra
        elif i not in c.decisive:
            words = label.split()
            if words[-1] in H.KINDS:                                                   # a generic substitution: one point of one kind
                arg, kind = words
                assert H.kind_holds(kind, c.fields[i][arg]), label
                assert c.invalid_args(i) == (() if kind == "NEG" else (arg,)), label
            else:
                assert "TWIST" in label and all(H.kind_holds("TWIST", c.fields[i][a]) for a in c.invalid_args(i)) and len(c.invalid_args(i)) == 3
            assert c.want[i] != c.honest_value, label
    # every kind reaches every call, and every point argument gets a NEUTRAL, an off-curve and a coordinate >= p
    for kind in H.KINDS:
        assert any(l.endswith(" " + kind) for l in c.labels), kind
    for arg in c.points:
        got = {l.split()[1] for l in c.labels if l.split()[0] == arg and l.split()[-1] in H.KINDS}
        assert {"NEUTRAL", "OFF"} <= got and got & {"COORD_PX", "COORD_PY"}, arg


@pytest.mark.parametrize("name", sorted(H.EC_CASES))
def test_every_guarded_argument_has_a_decisive_row(name):
    """decisive = the unguarded verifier accepts and the rule alone refuses; the arguments a row is decisive for are exactly its invalid ones"""
    c = H.EC_CASES[name]()
    covered = set()
    for i, args in c.decisive.items():
        assert c.unguarded[i] == c.honest_value != c.want[i], c.labels[i]
        assert c.invalid_args(i) == tuple(a for a in c.points if a in args), c.labels[i]
        for a in args:
            kind = "NEUTRAL" if c.fields[i][a] == (0, 0) else "NONCANON_X"
            assert H.kind_holds(kind, c.fields[i][a]) and kind in c.labels[i]
        covered |= set(args)
    assert covered == set(GUARDED[name])
    # no other row is decisive: whatever else the rule refuses, the algebra refuses as well
    assert [i for i in range(H.B) if c.unguarded[i] == c.honest_value != c.want[i]] == sorted(c.decisive)
    if name == "blame7":                                        # an invalid R blames both signers, an invalid R_dash_i / S_i signer i alone
        for i, args in c.decisive.items():
            assert c.want[i] == (0b11 if args == ("R",) else 1 << int(args[0][-1]))


@pytest.mark.parametrize("name", sorted(H.EC_CASES))
def test_oracle_on_the_table(name):
    """scalar and honest rows: the oracle's verdict IS the table's.  Point rows: the oracle's answers are recorded in
    hostile_cases.ORACLE_RECORD; it never refuses what the rule and the algebra accept, and where it says 1 and the rule says 0 — the
    decisive rows, all of them — that is asserted as the known divergence (the oracle has no deserialisation rule)."""
    c = H.EC_CASES[name]()
    got = oracle_verdicts(name)
    for i in c.scalar_rows() + c.honest:
        assert got[i] == c.want[i], c.labels[i]
    assert "".join(str(int(v)) for v in got) == H.ORACLE_RECORD[name]
    for i in c.point_rows():
        assert got[i] == c.unguarded[i], c.labels[i]                  # the oracle is an unguarded verifier: it agrees with the Python one
    diverge = [i for i in range(H.B) if got[i] == c.honest_value and c.want[i] != c.honest_value]
    assert diverge == sorted(c.decisive)
    if name == "blame7":
        assert all(int(got[i]) & ~c.want[i] == 0 for i in range(H.B))     # the oracle's mask never names a signer the rule clears


def test_lindell_rows():
    rows = H.lindell_rows()
    assert [k for _, k in rows] == list(H.KINDS) and set(H.EDGE_LANES) <= {lane for lane, _ in rows} and len({lane for lane, _ in rows}) == len(H.KINDS)


# ---- Bob's range proof ------------------------------------------------------------------------------------------------------------
def _bob_oracle_batch(Bsz, check):
    keys = F.load_keys()
    inp = H.bob_inputs(Bsz)
    tabs = [F.words([k.N for k in keys[:4]], 64)] + [F.words([getattr(k, f) for k in keys[4:7]], 64) for f in ("Nt", "h1", "h2")]
    widths = dict(alpha=24, beta=64, gamma=80, rho=72, rho_prim=88, sigma=72, tau=88)
    nw = {f: F.words([n[f] for n in inp["nonces"]], w) for f, w in widths.items()}
    pr, u = orc.bob_generate(*tabs, inp["kidx"], inp["sidx"], F.words(inp["a_enc"], 128), F.words(inp["mta_enc"], 128), F.words(inp["b"], 8),
                             F.words(inp["beta_prim"], 64), F.words(inp["r"], 64), nw["alpha"], nw["beta"], nw["gamma"], nw["rho"], nw["rho_prim"],
                             nw["sigma"], nw["tau"], check)
    cols = {f: F.ints(v) for f, v in pr.items()}
    cols.update(a_enc=list(inp["a_enc"]), mta_enc=list(inp["mta_enc"]))
    X = [H.raw(pyref.ec_mul(b, H.G)) for b in inp["b"]] if check else None
    uu = [H.raw(p) for p in F.points(u)] if check else None
    H.bob_tamper(Bsz, check, cols, X, uu)
    pw = {f: F.words(cols[f], v.shape[1]) for f, v in pr.items()}
    ok = orc.bob_verify(*tabs, inp["kidx"], inp["sidx"], F.words(cols["a_enc"], 128), F.words(cols["mta_enc"], 128), pw,
                        H.point_words(X) if check else None, H.point_words(uu) if check else None)
    return inp, cols, X, uu, list(ok)


@pytest.mark.parametrize("check", [False, True])
@pytest.mark.parametrize("Bsz", H.BOB_BATCHES)
def test_bob_rows_oracle_parity(Bsz, check):
    """orc.bob_verify on the tampered batch: the rows marked rejected are refused (a sample of rows is checked against pyref.bob_verify too), the honest tail accepted, and the two decisive rows (X = b G with b = 0, u = alpha G
    with alpha = q) are accepted by the oracle — Bob's transcript hashes coordinates as integers, so the oracle is its unguarded verifier —
    and refused by the rule."""
    keys = F.load_keys()
    inp, cols, X, uu, ok = _bob_oracle_batch(Bsz, check)
    layout, marks = H.bob_layout(Bsz, check), H.bob_rejected(Bsz, check)
    assert len(layout) < Bsz and ok[len(layout):] == [1] * (Bsz - len(layout))
    assert len(layout) == (H.BOB_SMALL if Bsz == 12 else len(H.BOB_ROWS) + (16 if check else 0))
    for i, (label, field, what) in enumerate(layout):
        if marks[i] and what != "DECISIVE":
            assert ok[i] == 0, label
    sample = ([0, 1, 2, 4, 8, Bsz - 1] if Bsz == 12 else [15, 17]) if not check else ([16] if Bsz > 12 else [])      # pyref is slow: a few rows
    for i in sample:
        ek, st = keys[inp["kidx"][i]], keys[4 + inp["sidx"][i]]
        pr = {f: cols[f][i] for f in ("t", "z", "e", "s", "s1", "s2", "t1", "t2")}
        Xi, ui = (X[i], uu[i]) if check else (None, None)
        assert ok[i] == int(pyref.bob_verify(ek.N, st.Nt, st.h1, st.h2, cols["a_enc"][i], cols["mta_enc"][i], pr, Xi, ui)), i
    if check and Bsz > 12:
        dec = [i for i, l in enumerate(layout) if l[2] == "DECISIVE"]
        assert [layout[i][1] for i in dec] == list(H.BOB_POINT_ARGS)
        for i in dec:
            pts = dict(X=X[i], u=uu[i])
            assert ok[i] == 1 and pts[layout[i][1]] == (0, 0) and H.valid(pts["X" if layout[i][1] == "u" else "u"])
        for i, (label, field, what) in enumerate(layout):
            if what in H.KINDS:
                assert H.kind_holds(what, dict(X=X[i], u=uu[i])[field]), label


def _bob_verify_flagless(N, Nt, h1, h2, a_enc, mta_enc, pr):
    """pyref.bob_verify with the inversions' verdicts dropped: the inverse of a non-unit is 0, as the device's inversion writes it"""
    def inv0(x, m):
        try:
            return pow(x, -1, m)
        except ValueError:
            return 0
    NN = N * N
    if pr["s1"] > pyref.Q ** 3:
        return False
    z_prim = pow(h1, pr["s1"], Nt) * pow(h2, pr["s2"], Nt) * inv0(pow(pr["z"], pr["e"], Nt), Nt) % Nt
    v = pow(a_enc, pr["s1"], NN) * pow(pr["s"], N, NN) * (pr["t1"] * N + 1) * inv0(pow(mta_enc, pr["e"], NN), NN) % NN
    w = pow(h1, pr["t1"], Nt) * pow(h2, pr["t2"], Nt) * inv0(pow(pr["t"], pr["e"], Nt), Nt) % Nt
    return pyref.hash_bigints([N, N + 1, a_enc, mta_enc, pr["z"], z_prim, pr["t"], v, w]) == pr["e"]


def test_bob_forged_rows_are_decisive_for_the_inversion_flags():
    """the three FORGED transcripts verify when the flag of the inversion they aim at is dropped (its output for a non-unit is 0), and only
    that flag refuses them: the reference (pyref, the oracle) fails the inversion.  One row per flag of bob_verify: z, mta_enc, t."""
    keys = F.load_keys()
    inp, cols, _, _, ok = _bob_oracle_batch(12, False)
    forged = [(i, l[2]) for i, l in enumerate(H.bob_layout(12, False)) if l[1] == "FORGED"]
    assert [w for _, w in forged] == ["z", "mta_enc", "t"]
    for i, which in forged:
        ek, st = keys[inp["kidx"][i]], keys[4 + inp["sidx"][i]]
        pr = {f: cols[f][i] for f in ("t", "z", "e", "s", "s1", "s2", "t1", "t2")}
        args = (ek.N, st.Nt, st.h1, st.h2, cols["a_enc"][i], cols["mta_enc"][i], pr)
        assert _bob_verify_flagless(*args) and not pyref.bob_verify(*args) and ok[i] == 0, which
        units = dict(z=pr["z"], t=pr["t"], mta_enc=cols["mta_enc"][i])
        assert [f for f, v in units.items() if v != 1] == [which]
