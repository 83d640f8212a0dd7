"""Hostile inputs for the stand-alone verifiers: points that `ec::aff_valid` must refuse, scalars at the edges of their field and
(for Bob's range proof) residues a prover may send, with the verdict every row must get.  Pure Python over tests/pyref.py; shared by
tests/test_hostile_cases_cpu.py (which proves the table) and tests/test_hostile_gpu.py (which runs it through the C-ABI).

A point is carried RAW: the pair (x, y) of 256-bit integers the 16 interface words hold, (0, 0) = the neutral element.  The kinds:
  NEUTRAL     all zero
  OFF         a curve point with y ^ 1
  TWIST       a point of y^2 = x^3 + TWIST_B (TWIST_B != 7); pyref.ec_add never uses b, so pyref.ec_mul gives its multiples there
  NONCANON_X  (x + p, y) for a curve point with x + p < 2^256 (x = 1, 2, 3, 4: the discrete log of such a point is unknown)
  COORD_PX / COORD_PY   x = p / y = p
  NEG         -P: valid but wrong, the control that the ALGEBRA refuses and not the guard
Validity is one rule, keygen_deal_cases.pt_valid.  Every proof system has an UNGUARDED verifier here: it hashes the 64 interface bytes
as they stand (what sha_chain_point would absorb under the default encoding profile: 04 and 64 zero bytes for NEUTRAL, the bytes of
x + p for NONCANON_X) and computes with pyref.ec_add / pyref.ec_mul on the coordinates reduced mod p.  A row's verdict is
    want = pt_valid(every point) and unguarded verdict.
A row is DECISIVE when the unguarded verifier accepts it: only the guard stands between it and a 1.  Every guarded point argument of
every call has one (Case.decisive); they are made by a prover that hashes raw bytes too: NEUTRAL where the algebra allows it (a zero
secret or nonce), NONCANON_X for a base whose discrete log the proof does not need.  TWIST statements (the prover chooses the base) are
verdict rows only: the device's ladder is GLV, whose split holds in the group of order q alone, so they say nothing about a device
without the guard.  Scalar rows (0, q, 2^256 - 1 in a proof's scalar field) and residues are anchored on the oracle instead: the CPU
test compares them with it.  Every expected value is exact.  Test infrastructure: nothing here is imported by the product."""
import functools
import hashlib

import fixtures as F
import pyref
from keygen_deal_cases import pt_valid

P, Q, G, H2 = pyref.P, pyref.Q, pyref.G, pyref.H2
B = 70                                   # one full wave and a ragged one: these kernels run one item per lane in 64-thread blocks
EDGE_LANES = (0, 63, 64)                 # the first lane, the last lane of block 0, the first lane of block 1
KINDS = ("NEUTRAL", "OFF", "TWIST", "NONCANON_X", "COORD_PX", "COORD_PY", "NEG")
INVALID_KINDS = KINDS[:-1]
TWIST_B = 2
MAX256 = (1 << 256) - 1
SCALAR_EDGES = (("0", 0), ("q", Q), ("max", MAX256))


# ---- raw points ---------------------------------------------------------------------------------------------------------------------
def lift(x, b=7):
    """the point (x, y) of y^2 = x^3 + b with the square root p = 3 (mod 4) gives, or None"""
    y2 = (x ** 3 + b) % P
    y = pow(y2, (P + 1) // 4, P)
    return (x, y) if y * y % P == y2 else None


def raw(pt):
    return (0, 0) if pt is None else pt


def red(rp):
    """what the arithmetic sees: None for the neutral row, else the coordinates mod p"""
    return None if rp == (0, 0) else (rp[0] % P, rp[1] % P)


def valid(rp):
    return pt_valid(None if rp == (0, 0) else rp)


def on_curve(pt, b=7):
    return pt is not None and (pt[1] * pt[1] - pt[0] ** 3 - b) % P == 0


def point_words(raws):
    return F.words([x | (y << 256) for x, y in raws], 16)


NONCANON = [(x + P, lift(x)[1]) for x in (1, 2, 3, 4)]                                      # lift(x) exists for each: asserted by the CPU test
TWIST_BASE = next(lift(x, TWIST_B) for x in range(1, 64) if lift(x, TWIST_B))
TWIST = [pyref.ec_mul(k, TWIST_BASE) for k in (1, 2, 3, 5, 7, 11)]


def kind_point(kind, pt, salt=0):
    """the hostile stand-in of kind `kind` for the honest curve point pt"""
    x, y = pt
    return {"NEUTRAL": (0, 0), "OFF": (x, y ^ 1), "NEG": (x, P - y), "COORD_PX": (P, y), "COORD_PY": (x, P),
            "NONCANON_X": NONCANON[salt % len(NONCANON)], "TWIST": TWIST[salt % len(TWIST)]}[kind]


def kind_holds(kind, rp):
    """is rp what its kind says?"""
    x, y = rp
    canon = x < P and y < P
    return {"NEUTRAL": rp == (0, 0),
            "OFF": canon and not on_curve(rp) and on_curve((x, y ^ 1)),
            "TWIST": canon and on_curve(rp, TWIST_B) and not on_curve(rp),
            "NONCANON_X": P <= x <= MAX256 and y < P and on_curve(red(rp)) and not valid(rp),
            "COORD_PX": x == P and not valid(rp), "COORD_PY": y == P and not valid(rp),
            "NEG": valid(rp)}[kind]


# ---- hashing of raw bytes (default encoding profile) ----------------------------------------------------------------------------------
def chain_scalar(raws):
    """Sha256::new().chain_points(..).result_scalar(): 04 | x | y of every point as its words stand"""
    h = hashlib.sha256()
    for x, y in raws:
        h.update(b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big"))
    return int.from_bytes(h.digest(), "big") % Q


def compressed_int(rp):
    """BigInt::from_bytes(P.to_bytes(true)) of the raw words (how PDLwSlack hashes its points)"""
    return int.from_bytes(bytes([2 + (rp[1] & 1)]) + rp[0].to_bytes(32, "big"), "big")


def _mul(k, rp):
    return pyref.ec_mul(k, red(rp))


def _sum(*pts):
    acc = None
    for p in pts:
        acc = pyref.ec_add(acc, p)
    return acc


def _safe(f, *a):
    """a verdict; an inversion of 0 mod p inside pyref.ec_add (a doubling of y = 0, off the curve) is a refusal"""
    try:
        return bool(f(*a))
    except ValueError:
        return False


# ---- the proof systems: prover and unguarded verifier on raw points ----------------------------------------------------------------
def dlog_prove(sk, nonce):
    pk, R = raw(pyref.ec_mul(sk, G)), raw(pyref.ec_mul(nonce, G))
    return dict(pk=pk, R=R, z=(nonce - chain_scalar([R, G, pk]) * sk) % Q)


def dlog_verify(f):
    c = chain_scalar([f["R"], G, f["pk"]])
    return _sum(pyref.ec_mul(f["z"], G), _mul(c, f["pk"])) == red(f["R"])


def pedersen_prove(m, r, s1, s2):
    com = raw(_sum(pyref.ec_mul(m, G), pyref.ec_mul(r, H2)))
    a1, a2 = raw(pyref.ec_mul(s1, G)), raw(pyref.ec_mul(s2, H2))
    e = chain_scalar([G, H2, com, a1, a2])
    return dict(com=com, e=e, a1=a1, a2=a2, z1=(s1 + e * m) % Q, z2=(s2 + e * r) % Q)


def pedersen_verify(f):
    e = chain_scalar([G, H2, f["com"], f["a1"], f["a2"]])
    return _sum(pyref.ec_mul(f["z1"], G), pyref.ec_mul(f["z2"], H2)) == _sum(red(f["a1"]), red(f["a2"]), _mul(e, f["com"]))


def heg_prove(x, r, s1, s2, Gp, H, Y):
    """HomoELGamalProof over the raw bases Gp, H, Y: D = x H + r Y, E = r Gp"""
    D, E = raw(_sum(_mul(x, H), _mul(r, Y))), raw(_mul(r, Gp))
    T, A3 = raw(_sum(_mul(s1, H), _mul(s2, Y))), raw(_mul(s2, Gp))
    e = chain_scalar([T, A3, Gp, H, Y, D, E])
    return dict(G=Gp, H=H, Y=Y, D=D, E=E, T=T, A3=A3, z1=(s1 + e * x) % Q, z2=(s2 + e * r) % Q)


def heg_verify(f):
    e = chain_scalar([f[k] for k in ("T", "A3", "G", "H", "Y", "D", "E")])
    return (_sum(_mul(f["z1"], f["H"]), _mul(f["z2"], f["Y"])) == _sum(red(f["T"]), _mul(e, f["D"])) and
            _mul(f["z2"], f["G"]) == _sum(red(f["A3"]), _mul(e, f["E"])))


def ecddh_prove(x, s, g1, g2):
    h1, h2, a1, a2 = raw(_mul(x, g1)), raw(_mul(x, g2)), raw(_mul(s, g1)), raw(_mul(s, g2))
    return dict(g1=g1, h1=h1, g2=g2, h2=h2, a1=a1, a2=a2, z=(s + chain_scalar([g1, h1, g2, h2, a1, a2]) * x) % Q)


def ecddh_verify(f):
    e = chain_scalar([f[k] for k in ("g1", "h1", "g2", "h2", "a1", "a2")])
    return (_mul(f["z"], f["g1"]) == _sum(red(f["a1"]), _mul(e, f["h1"])) and
            _mul(f["z"], f["g2"]) == _sum(red(f["a2"]), _mul(e, f["h2"])))


def _pdl_e(f):
    return pyref.hash_bigints([compressed_int(f["G"]), compressed_int(f["Q"]), f["c"], f["z"], compressed_int(f["u1"]), f["u2"], f["u3"]])


def pdl_prove(ek, st, Gp, x, r, nn):
    """pyref.pdl_prove over the raw base Gp (zk_pdl_with_slack/mod.rs:68-122): Q = x Gp, c = Enc(x; r)"""
    N, NN, Nt, h1, h2 = ek.N, ek.NN, st.Nt, st.h1, st.h2
    f = dict(G=Gp, Q=raw(_mul(x, Gp)), c=pyref.paillier_encrypt(N, x, r), z=pyref.commit(h1, h2, Nt, x, nn["rho"]),
             u1=raw(_mul(nn["alpha"], Gp)), u2=pyref.commit(N + 1, nn["beta"], NN, nn["alpha"], N),
             u3=pyref.commit(h1, h2, Nt, nn["alpha"], nn["gamma"]))
    e = _pdl_e(f)
    f.update(s1=e * x + nn["alpha"], s2=pyref.commit(r, nn["beta"], N, e, 1), s3=e * nn["rho"] + nn["gamma"])
    return f


def pdl_verify(f, ek, st):
    N, NN, Nt, h1, h2 = ek.N, ek.NN, st.Nt, st.h1, st.h2
    e = _pdl_e(f)
    if _sum(_mul(f["s1"], f["G"]), _mul(-e, f["Q"])) != red(f["u1"]):
        return False
    u2 = pyref.commit(pyref.commit(N + 1, f["s2"], NN, f["s1"], N), f["c"], NN, 1, -e)
    u3 = pyref.commit(pyref.commit(h1, h2, Nt, f["s1"], f["s3"]), f["z"], Nt, 1, -e)
    return u2 == f["u2"] and u3 == f["u3"]


def mta_verify(f):
    """MessageB::verify_proofs_get_alpha (mta/mod.rs:166-178) given alpha = Dec(c_b) mod q"""
    return (_sum(_mul(f["a"], f["pk"]), red(f["tpk"])) == pyref.ec_mul(f["share"] % Q, G) and
            dlog_verify(dict(pk=f["pk"], R=f["R"], z=f["z"])) and dlog_verify(dict(pk=f["tpk"], R=f["tR"], z=f["tz"])))


def blame7_signer_ok(f, i):
    """phase7_blame (blame.rs:434-454): R s_i == m R_dash_i + r S_i"""
    return _mul(f["s%d" % i], f["R"]) == _sum(_mul(f["m"], f["Rd%d" % i]), _mul(f["r"], f["S%d" % i]))


# ---- the case tables --------------------------------------------------------------------------------------------------------------
def hostile_slots(n):
    """n distinct lanes of a B-row batch: the edge lanes first, the others spread evenly over the rest"""
    rest = [i for i in range(B) if i not in EDGE_LANES]
    assert 3 <= n and 3 * n <= 2 * B, n                             # at least a third of the rows stays honest
    return list(EDGE_LANES) + [rest[k * len(rest) // (n - 3)] for k in range(n - 3)]


def kinds_for(arg_index, nargs):
    """the generic substitutions one point argument gets: every kind when the call has few point arguments, else NEUTRAL, OFF, one
    coordinate = p and one of the remaining kinds in rotation (a 70-row batch keeps a third of its rows honest)"""
    if nargs <= 4:
        return KINDS
    return ("NEUTRAL", "OFF", ("COORD_PX", "COORD_PY")[arg_index % 2], ("TWIST", "NONCANON_X", "NEG")[arg_index % 3])


class Case:
    """rows[i] = (label, fields); guarded / unguarded = the verdict with and without the validity rule; want = guarded"""

    def __init__(self, name, points, scalars, rows, decisive, verdicts, honest_value):
        self.name, self.points, self.scalars, self.honest_value = name, points, scalars, honest_value
        self.labels, self.fields = [r[0] for r in rows], [r[1] for r in rows]
        self.decisive = decisive                                         # {row: the point arguments whose guard alone refuses it}
        self.want, self.unguarded = [v[0] for v in verdicts], [v[1] for v in verdicts]
        self.honest = [i for i, l in enumerate(self.labels) if l == "honest"]

    def col(self, f):
        return [row[f] for row in self.fields]

    def invalid_args(self, i):
        return tuple(a for a in self.points if not valid(self.fields[i][a]))

    def point_rows(self):
        return [i for i, l in enumerate(self.labels) if l != "honest" and not l.startswith("scalar ")]

    def scalar_rows(self):
        return [i for i, l in enumerate(self.labels) if l.startswith("scalar ")]


def _verdict(points, verify):
    def both(f):
        ung = _safe(verify, f)
        return int(all(valid(f[a]) for a in points) and ung), int(ung)
    return both


HONEST_POOL = 12                         # distinct honest proofs per case (the wide ones, PDL and MtA: 6); the honest lanes and the substitutions cycle them


def _build(name, points, scalars, honest, specials, verdict, honest_value=1, pool=HONEST_POOL):
    """specials: [(label, fields, decisive arguments)] made by the raw-hashing prover; then every point argument under its generic kinds
    (an honest proof with that one point replaced), then every scalar field at 0, q, 2^256 - 1; honest proofs fill the other lanes"""
    r = F.Rng("hostile-" + name)
    rows = list(specials(r))
    made, turn = [honest(r) for _ in range(pool)], [0]

    def take():
        turn[0] += 1
        return dict(made[turn[0] % pool])
    for ai, arg in enumerate(points):
        for kind in kinds_for(ai, len(points)):
            f = take()
            f[arg] = kind_point(kind, f[arg], ai)
            rows.append(("%s %s" % (arg, kind), f, ()))
    for s in scalars:
        for label, v in SCALAR_EDGES:
            f = take()
            f[s] = v
            rows.append(("scalar %s=%s" % (s, label), f, ()))
    slots = hostile_slots(len(rows))
    out, decisive = [None] * B, {}
    for slot, (label, f, dec) in zip(slots, rows):
        out[slot] = (label, f)
        if dec:
            decisive[slot] = tuple(dec)
    out = [o if o is not None else ("honest", take()) for o in out]
    seen = {}

    def once(f):
        key = tuple(sorted(f.items()))
        if key not in seen:
            seen[key] = verdict(f)
        return seen[key]
    return Case(name, points, scalars, out, decisive, [once(f) for _, f in out], honest_value)


def _sc(r):
    return r.below(Q - 1) + 1


@functools.lru_cache(maxsize=None)
def dlog_case():
    honest = lambda r: dlog_prove(_sc(r), _sc(r))
    specials = lambda r: [("pk NEUTRAL (sk = 0)", dlog_prove(0, _sc(r)), ("pk",)), ("R NEUTRAL (nonce = 0)", dlog_prove(_sc(r), 0), ("R",))]
    return _build("dlog", ("pk", "R"), ("z",), honest, specials, _verdict(("pk", "R"), dlog_verify))


@functools.lru_cache(maxsize=None)
def pedersen_case():
    pts = ("com", "a1", "a2")
    honest = lambda r: pedersen_prove(_sc(r), _sc(r), _sc(r), _sc(r))
    specials = lambda r: [("com NEUTRAL (m = r = 0)", pedersen_prove(0, 0, _sc(r), _sc(r)), ("com",)),
                          ("a1 NEUTRAL (s1 = 0)", pedersen_prove(_sc(r), _sc(r), 0, _sc(r)), ("a1",)),
                          ("a2 NEUTRAL (s2 = 0)", pedersen_prove(_sc(r), _sc(r), _sc(r), 0), ("a2",))]
    return _build("pedersen", pts, ("z1", "z2"), honest, specials, _verdict(pts, pedersen_verify))


@functools.lru_cache(maxsize=None)
def heg_case():
    pts = ("G", "H", "Y", "D", "E", "T", "A3")
    base = lambda r: raw(pyref.ec_mul(_sc(r), G))

    def honest(r):
        return heg_prove(_sc(r), _sc(r), _sc(r), _sc(r), base(r), base(r), base(r))

    def specials(r):
        out = [("%s NONCANON_X (a base)" % a, heg_prove(_sc(r), _sc(r), _sc(r), _sc(r), *[NONCANON[j] if j == i else base(r) for j in range(3)]), (a,))
               for i, a in enumerate(("G", "H", "Y"))]
        # H = h Gen, Y = y Gen: x h + r y = 0 makes D neutral, s1 h + s2 y = 0 makes T neutral
        h, y, rr, s2 = _sc(r), _sc(r), _sc(r), _sc(r)
        Hh, Yy = raw(pyref.ec_mul(h, G)), raw(pyref.ec_mul(y, G))
        out.append(("D NEUTRAL (x H = -r Y)", heg_prove(-rr * y * pow(h, -1, Q) % Q, rr, _sc(r), _sc(r), base(r), Hh, Yy), ("D",)))
        out.append(("E NEUTRAL (r = 0)", heg_prove(_sc(r), 0, _sc(r), _sc(r), base(r), base(r), base(r)), ("E",)))
        out.append(("T NEUTRAL (s1 H = -s2 Y)", heg_prove(_sc(r), _sc(r), -s2 * y * pow(h, -1, Q) % Q, s2, base(r), Hh, Yy), ("T",)))
        out.append(("A3 NEUTRAL (s2 = 0)", heg_prove(_sc(r), _sc(r), _sc(r), 0, base(r), base(r), base(r)), ("A3",)))
        out.append(("G E A3 TWIST (a statement on the twist)", heg_prove(_sc(r), _sc(r), _sc(r), _sc(r), TWIST[0], base(r), base(r)), ()))
        return out
    return _build("heg", pts, ("z1", "z2"), honest, specials, _verdict(pts, heg_verify))


@functools.lru_cache(maxsize=None)
def ecddh_case():
    pts = ("g1", "h1", "g2", "h2", "a1", "a2")
    base = lambda r: raw(pyref.ec_mul(_sc(r), G))
    honest = lambda r: ecddh_prove(_sc(r), _sc(r), base(r), base(r))
    specials = lambda r: [("g1 NONCANON_X (a base)", ecddh_prove(_sc(r), _sc(r), NONCANON[0], base(r)), ("g1",)),
                          ("g2 NONCANON_X (a base)", ecddh_prove(_sc(r), _sc(r), base(r), NONCANON[3]), ("g2",)),
                          ("h1 h2 NEUTRAL (x = 0)", ecddh_prove(0, _sc(r), base(r), base(r)), ("h1", "h2")),
                          ("a1 a2 NEUTRAL (s = 0)", ecddh_prove(_sc(r), 0, base(r), base(r)), ("a1", "a2")),
                          ("g2 h2 a2 TWIST (a statement on the twist)", ecddh_prove(_sc(r), _sc(r), base(r), TWIST[1]), ())]
    return _build("ecddh", pts, ("z",), honest, specials, _verdict(pts, ecddh_verify))


PDL_KEYS, PDL_STATEMENTS = 2, 2          # Paillier keys 0..1 and statements 4..5 of tests/golden/keys16.json, item i -> (i % 2, (i // 2) % 2)


@functools.lru_cache(maxsize=None)
def pdl_case():
    keys = F.load_keys()
    pts = ("G", "Q", "u1")
    count = [0]

    def prove(r, Gp=None, x=None, alpha=None):
        i = count[0]
        count[0] += 1
        ek, st = keys[i % PDL_KEYS], keys[4 + (i // 2) % PDL_STATEMENTS]
        nn = F.pdl_nonces(r, ek, st)
        if alpha is not None:
            nn["alpha"] = alpha
        f = pdl_prove(ek, st, raw(pyref.ec_mul(_sc(r), G)) if Gp is None else Gp, _sc(r) if x is None else x, r.below(ek.N), nn)
        f.update(kidx=i % PDL_KEYS, sidx=(i // 2) % PDL_STATEMENTS)
        return f

    specials = lambda r: [("G NONCANON_X (a base)", prove(r, Gp=NONCANON[1]), ("G",)), ("Q NEUTRAL (x = 0)", prove(r, x=0), ("Q",)),
                          ("u1 NEUTRAL (alpha = q)", prove(r, alpha=Q), ("u1",)),
                          ("G Q u1 TWIST (a statement on the twist)", prove(r, Gp=TWIST[2]), ())]
    verify = lambda f: pdl_verify(f, keys[f["kidx"]], keys[4 + f["sidx"]])
    return _build("pdl", pts, (), prove, specials, _verdict(pts, verify), pool=6)


MTA_KEYS = 2                             # Alice's Paillier keys 0..1, item i -> key i % 2


@functools.lru_cache(maxsize=None)
def mta_case():
    """MessageB as Bob sends it: c_b = Enc(a b + beta_tag) under Alice's key, DLogProof(b), DLogProof(beta_tag mod q); `share` = the
    decryption a b + beta_tag (beta_tag < N / 2: no wrap mod N), which alpha = share mod q must equal whatever the points are"""
    keys = F.load_keys()
    pts = ("pk", "R", "tpk", "tR")
    count = [0]

    def make(r, b=None, bt=None, nb=None, nbt=None):
        i = count[0]
        count[0] += 1
        ek = keys[i % MTA_KEYS]
        a = _sc(r)
        b = _sc(r) if b is None else b
        bt = r.below(ek.N >> 1) if bt is None else bt
        p1, p2 = dlog_prove(b, _sc(r) if nb is None else nb), dlog_prove(bt % Q, _sc(r) if nbt is None else nbt)
        share = a * b + bt
        return dict(a=a, share=share, cb=pyref.paillier_encrypt(ek.N, share, r.coprime_below(ek.N)), kidx=i % MTA_KEYS,
                    pk=p1["pk"], R=p1["R"], z=p1["z"], tpk=p2["pk"], tR=p2["R"], tz=p2["z"])

    specials = lambda r: [("pk NEUTRAL (b = 0)", make(r, b=0), ("pk",)), ("R NEUTRAL (nonce = 0)", make(r, nb=0), ("R",)),
                          ("tpk NEUTRAL (beta_tag = 5 q)", make(r, bt=5 * Q), ("tpk",)), ("tR NEUTRAL (nonce = 0)", make(r, nbt=0), ("tR",))]
    return _build("mta", pts, ("z", "tz"), make, specials, _verdict(pts, mta_verify), pool=6)


BLAME7_S = 2                             # signers per session: 70 sessions are 140 lanes of blame7_kernel


@functools.lru_cache(maxsize=None)
def blame7_case():
    """one row = one session of two signers: R, m, r and per signer i (s_i, R_dash_i, S_i).  The verdict is the bad-actor MASK: bit i is set
    when R, R_dash_i or S_i is no valid point or R s_i != m R_dash_i + r S_i.  Honest and decisive-unguarded value: 0."""
    pts = ("R", "Rd0", "S0", "Rd1", "S1")

    def session(r, R=None, rho=None):
        """R = rho Gen (or a raw base of unknown log: then everything is a multiple of R itself)"""
        Rr = raw(pyref.ec_mul(rho, G)) if R is None else R
        f = dict(R=Rr, m=_sc(r), r=_sc(r))
        for i in range(BLAME7_S):
            d, sg = _sc(r), _sc(r)
            f.update({"Rd%d" % i: raw(_mul(d, Rr)), "S%d" % i: raw(_mul(sg, Rr)), "s%d" % i: (f["m"] * d + f["r"] * sg) % Q})
        return f

    honest = lambda r: session(r, rho=_sc(r))

    def specials(r):
        out = [("R NONCANON_X (a base)", session(r, R=NONCANON[2]), ("R",))]
        f = honest(r)                                       # R neutral: m R_dash_i + r S_i = 0 for both signers
        f["R"] = (0, 0)
        for i in range(BLAME7_S):
            d = _sc(r)
            f.update({"Rd%d" % i: raw(pyref.ec_mul(d, G)), "S%d" % i: raw(pyref.ec_mul(-f["m"] * d * pow(f["r"], -1, Q) % Q, G))})
        out.append(("R NEUTRAL (m R_dash = -r S)", f, ("R",)))
        for i in range(BLAME7_S):
            rho, sg = _sc(r), _sc(r)                        # R_dash_i neutral: s_i R = r S_i
            f = session(r, rho=rho)
            f.update({"Rd%d" % i: (0, 0), "S%d" % i: raw(pyref.ec_mul(sg * rho, G)), "s%d" % i: f["r"] * sg % Q})
            out.append(("Rd%d NEUTRAL (s R = r S)" % i, f, ("Rd%d" % i,)))
            rho, d = _sc(r), _sc(r)                         # S_i neutral: s_i R = m R_dash_i
            f = session(r, rho=rho)
            f.update({"S%d" % i: (0, 0), "Rd%d" % i: raw(pyref.ec_mul(d * rho, G)), "s%d" % i: f["m"] * d % Q})
            out.append(("S%d NEUTRAL (s R = m R_dash)" % i, f, ("S%d" % i,)))
        return out

    def verdict(f):
        ung = [_safe(blame7_signer_ok, f, i) for i in range(BLAME7_S)]
        grd = [ung[i] and valid(f["R"]) and valid(f["Rd%d" % i]) and valid(f["S%d" % i]) for i in range(BLAME7_S)]
        mask = lambda oks: sum((0 if o else 1) << i for i, o in enumerate(oks))
        return mask(grd), mask(ung)
    return _build("blame7", pts, ("s0", "s1"), honest, specials, verdict, honest_value=0)


WIDTHS = dict(pdl=dict(c=128, z=64, u2=128, u3=64, s1=25, s2=64, s3=89), mta=dict(cb=128, share=64))


def words(case, field):
    """one column of a case as interface words [B, w]: points 16, scalars 8, the wide fields by WIDTHS"""
    col = case.col(field)
    return point_words(col) if field in case.points else F.words(col, WIDTHS.get(case.name, {}).get(field, 8))


EC_CASES = dict(dlog=dlog_case, pedersen=pedersen_case, heg=heg_case, ecddh=ecddh_case, pdl=pdl_case, mta=mta_case, blame7=blame7_case)

# What the ORACLE's stand-alone verifiers answer on every row of the tables above ("0" / "1" per row; blame7: the mask as a digit),
# recorded by tests/test_hostile_cases_cpu.py.  They carry no deserialisation rule by design (pt_in only knows the all-zero row), so on
# the rows where the unguarded Python verifier says 1 the oracle says 1 as well: that divergence from the device is KNOWN and stays.
ORACLE_RECORD = dict(
    blame7="0000000300303030010101001010100101020200202020020202001010100200020200",
    dlog="1011101110111011101110111101110111011101110111101110111011101111001111",
    ecddh="1110101011010101101010110101011010101011010101101010110101011011101011",
    heg="1111111010101001010010101001010010101001010010101001010010101001110101",
    mta="1101010101010101010101001010101010101010101010010101010101010101110101",
    pdl="1011011011011011011011011011011011011011011011011011011011011011110111",
    pedersen="1010101101011010110101101011010110101101011010110101101011010111101011")


# ---- Lindell'17 signing: the peer's ephemeral point --------------------------------------------------------------------------------
def lindell_rows():
    """[(lane, kind)]: which rows of a 70-session batch (tests/lindell_fixture.py) get their R1 (party two's call) or R2 (party one's call)
    replaced by kind_point(kind, the honest point, lane).  NEG stays valid: that row must still equal the oracle on the negated point."""
    return list(zip(hostile_slots(len(KINDS)), KINDS))


# ---- Bob's range proof: residues and scalars a prover may send ------------------------------------------------------------------------
# (label, field, value(k), rejected) — k: N, NN, p (Alice's key), Nt, h1, h2 (the statement), a_enc, cur (the honest value of the field).
# `rejected` None: the row may verify (an unreduced ciphertext that no longer fits falls back to the honest one); every other row must be
# refused.  A FORGED row replaces the whole proof (bob_forge): a transcript that verifies if the verifier takes 0 for the inverse of a
# non-unit and forgets the inversion's flag — the rows that make the three `ok` flags of bob_verify decisive.
# The first BOB_SMALL rows are the forged ones and those whose value reaches one of the three inversions: the B = 12 batch holds them and
# two honest proofs, the B = 44 batch holds every row.
_fits = lambda v: v if v.bit_length() <= 4096 else None
BOB_ROWS = [
    ("forged on z = 0", "FORGED", "z", True), ("forged on mta_enc = 7 N", "FORGED", "mta_enc", True), ("forged on t = 0", "FORGED", "t", True),
    ("z = N~", "z", lambda k: k.Nt, True), ("z = 0", "z", lambda k: 0, True),
    ("t = N~", "t", lambda k: k.Nt, True), ("t = 0", "t", lambda k: 0, True),
    ("mta_enc = 0", "mta_enc", lambda k: 0, True), ("mta_enc = 7 N", "mta_enc", lambda k: 7 * k.N, True),
    ("mta_enc = 11 p", "mta_enc", lambda k: 11 * k.p, True),
    ("mta_enc + N^2", "mta_enc", lambda k: _fits(k.cur + k.NN), None),
    ("s = N", "s", lambda k: k.N, True), ("s = 0", "s", lambda k: 0, True),
    ("s = N - 1", "s", lambda k: k.N - 1, True), ("s = 2^2048 - 1", "s", lambda k: (1 << 2048) - 1, True),
    ("a_enc = 7 N", "a_enc", lambda k: 7 * k.N, True),
    ("s1 = q^3", "s1", lambda k: Q ** 3, True), ("s1 = q^3 + 1", "s1", lambda k: Q ** 3 + 1, True),
    ("s2 all ones", "s2", lambda k: (1 << (89 * 32)) - 1, True), ("t2 all ones", "t2", lambda k: (1 << (89 * 32)) - 1, True),
    ("t1 all ones", "t1", lambda k: (1 << (81 * 32)) - 1, True),
    ("e = 0", "e", lambda k: 0, True),
]
BOB_SMALL = 10
BOB_POINT_ARGS = ("X", "u")              # with check: each under every kind, after the numeric rows
BOB_BATCHES = (12, 44)


def bob_layout(Bsz, check):
    """-> [(label, field, value function or kind)] for the leading hostile rows of a batch; the rows after them are honest"""
    if Bsz < len(BOB_ROWS) + 2:
        return [r[:3] for r in BOB_ROWS[:BOB_SMALL]]
    rows = [r[:3] for r in BOB_ROWS]
    if check:
        rows += [("X NEUTRAL (b = 0)", "X", "DECISIVE"), ("u NEUTRAL (alpha = q)", "u", "DECISIVE")]
        rows += [("%s %s" % (a, kind), a, kind) for a in BOB_POINT_ARGS for kind in KINDS]
    return rows


def bob_rejected(Bsz, check):
    """row -> True (must be refused) / None (may verify), for the hostile rows of bob_layout"""
    marks = {r[0]: r[3] for r in BOB_ROWS}
    return [marks.get(label, True) for label, _, _ in bob_layout(Bsz, check)]


@functools.lru_cache(maxsize=None)
def _bob_inputs_full():
    keys = F.load_keys()
    r = F.Rng("hostile-bob")
    Bsz = max(BOB_BATCHES)
    layout = bob_layout(Bsz, True)
    kidx, sidx = [i % 4 for i in range(Bsz)], [(i // 2) % 3 for i in range(Bsz)]
    o = dict(kidx=kidx, sidx=sidx, a_enc=[], mta_enc=[], b=[], beta_prim=[], r=[], nonces=[])
    for i, (k, s) in enumerate(zip(kidx, sidx)):
        ek, st = keys[k], keys[4 + s]
        b, bp, rr = r.below(Q), r.below(ek.N), r.below(ek.N)
        nn = F.bob_nonces(r, ek, st)
        if i < len(layout) and layout[i][2] == "DECISIVE":
            if layout[i][1] == "X":
                b = 0                                                     # X = b G is the neutral row
            else:
                nn["alpha"] = Q                                           # u = alpha G is the neutral row
        ae = r.coprime_below(ek.NN)                                       # a unit mod N^2: a ciphertext of something, which is all Bob knows of it
        o["a_enc"].append(ae); o["b"].append(b); o["beta_prim"].append(bp); o["r"].append(rr); o["nonces"].append(nn)
        o["mta_enc"].append(pow(ae, b, ek.NN) * pyref.paillier_encrypt(ek.N, bp, rr) % ek.NN)
    return o


def bob_inputs(Bsz):
    """what BobProof::generate takes, as Python ints: keys 0..3, statements 4..6.  The B = 44 batch is laid out by bob_layout(44, True) (its
    two DECISIVE rows, b = 0 and alpha = q, are honest inputs without `check` as well); the B = 12 batch is its rows 0..9 and its last two"""
    full = _bob_inputs_full()
    take = list(range(max(BOB_BATCHES))) if Bsz == max(BOB_BATCHES) else list(range(BOB_SMALL)) + list(range(max(BOB_BATCHES) - (Bsz - BOB_SMALL), max(BOB_BATCHES)))
    return {f: [v[i] for i in take] for f, v in full.items()}


class BobKey:
    def __init__(self, ek, st, a_enc, cur):
        self.N, self.NN, self.p, self.Nt, self.h1, self.h2, self.a_enc, self.cur = ek.N, ek.NN, ek.p, st.Nt, st.h1, st.h2, a_enc, cur


def bob_forge(which, k):
    """BobProof::verify (range_proofs.rs:321-412) recomputes z' = h1^s1 h2^s2 (z^e)^-1, v = a_enc^s1 s^N (t1 N + 1) (mta_enc^e)^-1 and
    w = h1^t1 h2^t2 (t^e)^-1 and compares H(.., z', .., v, w) with e: Fiat-Shamir binds the prover because these depend on e.  With z = t =
    mta_enc = 1 they do not — and if ONE of the three is a non-unit instead (0, or a multiple of N) whose "inverse" the verifier takes to
    be 0 (what the batched inversion writes beside its cleared flag), that product is 0 whatever e is.  So the prover computes e himself:
    the transcript below verifies on a verifier that drops the flag of inversion `which`, without any witness.  (Without `check`: the
    extension's equation s1 G = e X + u binds e again.)  The reference refuses: mod_inv fails."""
    z, t, mta = (0 if which == "z" else 1), (0 if which == "t" else 1), (7 * k.N if which == "mta_enc" else 1)
    s, s1, s2, t1, t2 = 1, 5, 7, 3, 11
    zp = 0 if which == "z" else pow(k.h1, s1, k.Nt) * pow(k.h2, s2, k.Nt) % k.Nt
    w = 0 if which == "t" else pow(k.h1, t1, k.Nt) * pow(k.h2, t2, k.Nt) % k.Nt
    v = 0 if which == "mta_enc" else pow(k.a_enc, s1, k.NN) * pow(s, k.N, k.NN) * (t1 * k.N + 1) % k.NN
    e = pyref.hash_bigints([k.N, k.N + 1, k.a_enc, mta, z, zp, t, v, w])
    return dict(z=z, t=t, mta_enc=mta, e=e, s=s, s1=s1, s2=s2, t1=t1, t2=t2)


def bob_tamper(Bsz, check, cols, X=None, u=None):
    """applies bob_layout to honest columns (dict field -> list of ints: the proof fields, a_enc, mta_enc) and raw point lists X, u, in place"""
    keys = F.load_keys()
    inp = bob_inputs(Bsz)
    for i, (label, field, what) in enumerate(bob_layout(Bsz, check)):
        if field in BOB_POINT_ARGS:
            if what != "DECISIVE":
                pts = X if field == "X" else u
                pts[i] = kind_point(what, pts[i], i)
            continue
        k = BobKey(keys[inp["kidx"][i]], keys[4 + inp["sidx"][i]], cols["a_enc"][i], cols.get(field, [None] * Bsz)[i])
        if field == "FORGED":
            for f, v in bob_forge(what, k).items():
                cols[f][i] = v
            continue
        v = what(k)
        if v is not None:
            cols[field][i] = v
