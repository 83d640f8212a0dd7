"""Launches of the fixed-base ladder of h1 / h2 (`fb_modexp_kernel`, multi_party_ecdsa_amd/csrc/mpe_fixedbase.h, launched by
`launch_fb_modexp` of mpe_proofs.h from the tables `mpe_statements_create_wb` builds) at every window width and lane split, with the
exponents and batch shapes where a row index, a run boundary, a tree partner or a scheduler unit can go wrong.  Pure Python: values,
expected results and the geometry the device derives from them; nothing here touches the product.

The route to the kernel is the range proof, whose nonces are inputs (there is no call for a bare h^e mod N~):
    alice_generate   z = h1^a h2^rho leaves the prover verbatim (a = 0: h2^rho alone; rho = 0: h1^a alone), w = h1^alpha h2^gamma
                     enters e and through it s, s1, s2                                              exponent words 8, 72, 24, 88
    alice_verify     h1^s1 h2^s2; with a = 0 and rho = 0 the exponents are chosen: s1 = alpha, s2 = gamma             words 25, 89
    bob_generate     t = h1^beta' h2^sigma leaves the prover verbatim, w = h1^gamma h2^tau enters e              adds words 64, 80
    bob_verify       h1^t1 h2^t2 with t1 = e beta' + gamma                                                          adds words 81
What a verifier can SHOW of an exponent is limited by the protocol: an accepted s1 is at most q^3 < 2^768 and an honest s2 is below
2^2817, while the top window of a 25-word (89-word) exponent starts at bit 784 (2832) or above at every width.  A non-zero digit there exists
only in a proof both sides reject, so those digits are compared by verdict (`Hostile` rows); every other planted digit reaches a byte
that is compared.

`alice_case(wb)` / `bob_case(wb)` -> the rows of a window width, `Case.expected()` -> the oracle's proof, cached on the case;
tests/test_fb_cases_cpu.py checks that the table is not vacuous, tests/test_fixedbase_gpu.py runs it on the GPU."""
import functools

import fixtures as F
import pyref

Q = pyref.Q
Q3 = Q ** 3

# ---- the geometry of the device, mirrored (tests/test_fb_cases_cpu.py pins these to the source text) -----------------------------------
FB_EXP_BITS = 89 * 32      # mpe_fixedbase.h: `constexpr int FB_EXP_BITS = 89 * 32;`
GROUPS = 16                # mpe_bigint.h: Cfg2048 has 4 threads per integer, 16 lane groups per wave
ROW_WORDS = 72             # Cfg2048::K: a table row is 72 words, 288 bytes
CUS = 256                  # compute units of an MI355X (the GPU test takes the device's own count)
WAVES_PER_CU = 8           # mpe_internal.h, mpe_ctx: `modexp_waves_per_cu = 8`
FB_WINDOW_BITS = 13        # mpe_internal.h, mpe_ctx: `fb_window_bits = 13`

WIDTHS = (2, 4, 5, 8, 11, 13, 16)                                   # 2, 4, 8, 16 divide 32 (no window straddles two words); 5, 11, 13 do not
STATEMENTS = {2: 3, 4: 3, 5: 3, 8: 3, 11: 3, 13: 2, 16: 1}          # 16-bit tables are 3.4 GB per base
SPLITS = (1, 2, 4, 8, 16)
ALICE_GENERATE_WORDS = dict(a=8, alpha=24, rho=72, gamma=88)
ALICE_VERIFY_WORDS = dict(s1=25, s2=89)
BOB_GENERATE_WORDS = dict(b=8, alpha=24, beta_prim=64, rho=72, sigma=72, gamma=80, rho_prim=88, tau=88)
BOB_VERIFY_WORDS = dict(s1=25, s2=89, t1=81, t2=89)
EXP_WORDS = (8, 24, 25, 64, 72, 80, 81, 88, 89)                     # every exponent width the kernel is launched with
BOB_WIDTHS, BOB_SPLITS = (5, 16), (2, 8)
SCHED_WB = 8
SCHED_OPTIONS = {"fb_split": 16, "waves_per_cu": 1}                 # one item per wave: an item is a unit, cap = the compute units
BUDGETS_MB = {1: 0, 20: 4, 200: 8}                                  # option fb_budget_mb -> the width 3 statements get (select_width)
ROWS = 37


def fb_windows(wb):
    """windows of a table: `(FB_EXP_BITS + wb - 1) / wb`"""
    return (FB_EXP_BITS + wb - 1) // wb


def nwin(exp_words, wb):
    """windows of a launch: `(exp_words * 32 + FB_WB - 1) / FB_WB`"""
    return (exp_words * 32 + wb - 1) // wb


def run_of(part, exp_words, wb, S):
    """(first window, rows) of lane group `part`: `lo = part * nwin / S, cnt = (part + 1) * nwin / S - lo`"""
    n = nwin(exp_words, wb)
    lo = part * n // S
    return lo, (part + 1) * n // S - lo


def longest_run(exp_words, wb, S):
    """`cmax = (nwin + S - 1) / S`: every group multiplies this many factors, a short run pads with the form of 1"""
    return (nwin(exp_words, wb) + S - 1) // S


def chain_length(exp_words, wb, S):
    """multiplications one item's chain takes: `total = cmax - 1 + lg + 1`"""
    return longest_run(exp_words, wb, S) - 1 + S.bit_length() - 1 + 1


def fb_digit(ex, exp_words, i, wb):
    """`fb_digit` on a list of 32-bit words, shift for shift"""
    bitpos = i * wb
    word, sh = bitpos >> 5, bitpos & 31
    v = ex[word] >> sh
    if sh + wb > 32 and word + 1 < exp_words:
        v |= (ex[word + 1] << (32 - sh)) & 0xFFFFFFFF
    return v & ((1 << wb) - 1)


def to_words(v, exp_words):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(exp_words)]


def digits(v, exp_words, wb):
    ex = to_words(v, exp_words)
    return [fb_digit(ex, exp_words, i, wb) for i in range(nwin(exp_words, wb))]


def straddlers(exp_words, wb):
    """the windows that take the word-straddle branch of fb_digit (bits of two words)"""
    return [i for i in range(nwin(exp_words, wb)) if (i * wb & 31) + wb > 32 and (i * wb >> 5) + 1 < exp_words]


def top_digit_max(exp_words, wb):
    """the largest digit of the top window, which may be partial: the exponent ends at bit 32 * exp_words"""
    return (1 << min(wb, 32 * exp_words - (nwin(exp_words, wb) - 1) * wb)) - 1


def split_of(B, fb_split=0, cap=CUS * WAVES_PER_CU, adaptive=True):
    """the lane groups per item `launch_fb_modexp` picks: option fb_split rounded down to a power of two, else the widest split
    that still leaves one wave per SIMD"""
    split = 1
    if fb_split > 0:
        while split * 2 <= fb_split and split * 2 <= GROUPS:
            split *= 2
    elif adaptive:
        while split * 2 <= GROUPS and (B * split * 2 + GROUPS - 1) // GROUPS <= cap // 2:
            split *= 2
    return split


def units_of(B, S):
    per_wave = GROUPS // S
    return (B + per_wave - 1) // per_wave


def sched_mode(units, cap):
    """`ladder_sched` / `ladder_grid`: (mode, workgroups)"""
    if 2 * units <= cap:
        return "primaries", 2 * units
    if units <= cap:
        return "static", units
    return "queue", cap


def table_bytes(count, wb):
    """`mpe_statements_table_bytes`"""
    return 2 * count * fb_windows(wb) * (1 << wb) * ROW_WORDS * 4


def select_width(count, budget_bytes, start=FB_WINDOW_BITS, fixed_base=True):
    """the width `mpe_gg20_keys_create` builds `count` statements' tables with under an explicit budget (option fb_budget_mb), as
    `mpe_gg20_keys_fb_window_bits` reports it"""
    wb = start
    while wb > 4 and table_bytes(count, wb) > budget_bytes:
        wb -= 1
    if table_bytes(count, wb) > budget_bytes:
        wb = 0
    return wb if fixed_base else 0


def batch_sizes(S):
    per_wave = GROUPS // S
    return sorted({1, per_wave, per_wave + 1, ROWS})


def sched_sizes(cap):
    """one batch per scheduler mode under SCHED_OPTIONS"""
    return [cap // 2, cap // 2 + 1, cap + 3]


def statement_index(i, nst):
    """repeats and skips: 0 0 2 2 1 1 0 0 ... over three statements"""
    return (2 * (i // 2)) % nst if nst == 3 else (i // 2) % nst


# ---- exponents -------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("zero", "one", "all ones", "top bit", "planted 0", "planted max", "random")


def planted_windows(exp_words, wb, top_bits=None):
    """the windows a planted exponent fixes: the lowest, the top one (of a value of `top_bits` bits, default the full width) and the
    straddling window nearest the middle, where the width has one"""
    n = nwin(exp_words, wb) if top_bits is None else (top_bits + wb - 1) // wb
    st = [i for i in straddlers(exp_words, wb) if 0 < i < n - 1]
    return [0, n - 1] + ([min(st, key=lambda i: abs(i - n // 2))] if st else [])


def planted(r, exp_words, wb, fill, top_bits=None):
    """random, with digit 0 (fill = 0) or the maximal digit (fill = 1) in planted_windows(); their neighbours get a digit that is neither"""
    bits = 32 * exp_words if top_bits is None else top_bits
    v = r.bits(bits)
    mask = (1 << wb) - 1
    wins = planted_windows(exp_words, wb, top_bits)
    for i in wins:
        for j in (i - 1, i + 1):
            if j >= 0 and j not in wins and (j + 1) * wb <= bits and wb > 1:
                v = v & ~(mask << (j * wb)) | ((1 + r.below(mask - 1)) << (j * wb))
        v = v & ~(mask << (i * wb)) | ((mask if fill else 0) << (i * wb))
    return v & ((1 << bits) - 1)


def family(r, exp_words, wb):
    """{family name: value} for one exponent width"""
    bits = 32 * exp_words
    return {"zero": 0, "one": 1, "all ones": (1 << bits) - 1, "top bit": 1 << (bits - 1), "planted 0": planted(r, exp_words, wb, 0),
            "planted max": planted(r, exp_words, wb, 1), "random": r.bits(bits)}


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
PAILLIER_KEYS = 4          # keys[0:4] encrypt, keys[4:4 + STATEMENTS[wb]] are the statements


@functools.lru_cache(maxsize=None)
def _keys():
    return F.load_keys()


@functools.lru_cache(maxsize=None)
def _r_to_the_N(k, r):
    return pow(r, _keys()[k].N, _keys()[k].NN)


def _encrypt(k, m, r):
    """pyref.paillier_encrypt with r^N mod N^2 kept: the rows of every width share their r"""
    key = _keys()[k]
    return (1 + m * key.N) % key.NN * _r_to_the_N(k, r) % key.NN


class Hostile:
    """what a verifier's copy of a row's proof carries instead of the honest field: {"s1" / "s2": value}"""

    def __init__(self, **fields):
        self.fields = fields


class AliceRow:
    def __init__(self, name, a, rho, alpha, gamma, accept, hostile=None):
        self.name, self.a, self.rho, self.alpha, self.gamma, self.accept, self.hostile = name, a, rho, alpha, gamma, accept, hostile


def _sure_verdict(a, alpha):
    """s1 = e a + alpha with e < 2^256: accepted when even the largest e keeps it at most q^3, rejected when alpha alone exceeds q^3.
    Rows are built so that one of the two holds."""
    if alpha + ((1 << 256) - 1) * a <= Q3:
        return True
    assert alpha > Q3, "a row whose verdict depends on the challenge"
    return False


class AliceCase:
    """37 rows of AliceProof inputs for one window width; batch(B) = the first B rows"""

    def __init__(self, wb):
        self.wb, self.nst = wb, STATEMENTS[wb]
        keys = _keys()
        r = F.Rng(f"fb-alice-{wb}")
        fam = {w: family(r, w, wb) for w in (8, 24, 72, 88)}
        small = lambda: r.bits(700)                               # an alpha that keeps s1 <= q^3 whatever a < 2^256 and e are
        rows = [
            # the boundaries of the verifier's range: s1 = q^3 exactly (accepted), all-ones rho alone, ones beside a lone top bit, and
            # an s1 of 769 bits beside an s2 of 2817 bits, which the reference rejects
            AliceRow("s1 = q^3, s2 = 2^2816 - 1", 0, 0, Q3, (1 << 2816) - 1, True),
            AliceRow("rho all ones alone", 0, (1 << 2304) - 1, 0, 0, True),
            AliceRow("ones and a lone top bit", 1, 1, 1, 1 << 2815, True),
            AliceRow("s1 of 769 bits, s2 of 2817 bits", Q - 1, (1 << 2304) - 1, (1 << 768) - 1, (1 << 2816) - 1, False),
            # rho and gamma all ones beside an accepted s1: s2 = e (2^2304 - 1) + 2^2816 - 1 has bit 2816 set (the 89th word is 1)
            AliceRow("s2 with its 89th word set", 0, (1 << 2304) - 1, r.bits(700), (1 << 2816) - 1, True),
        ]
        for f in FAMILIES:                                        # a = 0, rho = 0: s1 = alpha, s2 = gamma, w = h1^alpha h2^gamma
            rows.append(AliceRow(f"alpha, gamma {f}", 0, 0, fam[24][f], fam[88][f], _sure_verdict(0, fam[24][f])))
        for f in FAMILIES:                                        # a = 0: z = h2^rho alone
            rows.append(AliceRow(f"rho {f}", 0, fam[72][f], small(), r.bits(2816), True))
        for f in FAMILIES:                                        # rho = 0: z = h1^a alone
            rows.append(AliceRow(f"a {f}", fam[8][f], 0, small(), r.bits(2816), True))
        ones25, ones89 = (1 << 800) - 1, (1 << 2848) - 1
        for name, h in [("s1 all ones", Hostile(s1=ones25)), ("s2 all ones", Hostile(s2=ones89)),
                        ("s1 planted max", Hostile(s1=planted(r, 25, wb, 1))), ("s2 planted max", Hostile(s2=planted(r, 89, wb, 1))),
                        ("s1 planted 0", Hostile(s1=planted(r, 25, wb, 0) | 1 << 770)), ("s2 planted 0", Hostile(s2=planted(r, 89, wb, 0)))]:
            rows.append(AliceRow("hostile " + name, r.below(Q), r.bits(2300), small(), r.bits(2816), False, hostile=h))
        k = 0
        while len(rows) < ROWS:                                   # honest rows with the reference's ranges
            nn = F.alice_nonces(r, keys[len(rows) % PAILLIER_KEYS], keys[PAILLIER_KEYS + statement_index(len(rows), self.nst)])
            rows.append(AliceRow(f"honest {k}", r.below(Q), nn["rho"], r.bits(700), nn["gamma"], True))
            k += 1
        assert len(rows) == ROWS
        self.rows = rows
        self.B = ROWS
        self.kidx = [i % PAILLIER_KEYS for i in range(ROWS)]
        self.sidx = [statement_index(i, self.nst) for i in range(ROWS)]
        rr = F.Rng("fb-alice-paillier")                           # the Paillier side does not depend on the width: encrypted once
        self.r = [rr.below(keys[k].N) for k in self.kidx]
        self.beta = [rr.coprime_below(keys[k].N) for k in self.kidx]
        self._want = self._z = self._verify = None

    def statements(self):
        """(Nt, h1, h2) of the case's statements, as integers"""
        ks = _keys()[PAILLIER_KEYS:PAILLIER_KEYS + self.nst]
        return [k.Nt for k in ks], [k.h1 for k in ks], [k.h2 for k in ks]

    def paillier_N(self):
        return [k.N for k in _keys()[:PAILLIER_KEYS]]

    def cipher(self):
        return [_encrypt(k, row.a, r) for k, row, r in zip(self.kidx, self.rows, self.r)]

    def inputs(self):
        """word arrays of everything alice_generate takes"""
        return dict(a=F.words([x.a for x in self.rows], 8), c=F.words(self.cipher(), 128), r=F.words(self.r, 64),
                    alpha=F.words([x.alpha for x in self.rows], 24), beta=F.words(self.beta, 64),
                    gamma=F.words([x.gamma for x in self.rows], 88), rho=F.words([x.rho for x in self.rows], 72))

    def tables(self):
        Nt, h1, h2 = self.statements()
        return dict(N=F.words(self.paillier_N(), 64), Nt=F.words(Nt, 64), h1=F.words(h1, 64), h2=F.words(h2, 64))

    def python_z(self):
        """z = h1^a h2^rho mod N~ of every row, by Python's pow"""
        if self._z is None:
            Nt, h1, h2 = self.statements()
            self._z = [pow(h1[s], x.a, Nt[s]) * pow(h2[s], x.rho, Nt[s]) % Nt[s] for s, x in zip(self.sidx, self.rows)]
        return self._z

    def expected(self):
        """the oracle's proof of all rows {field: words}, cached on the case"""
        if self._want is None:
            import orc
            t, i = self.tables(), self.inputs()
            self._want = orc.alice_generate(t["N"], t["Nt"], t["h1"], t["h2"], self.kidx, self.sidx, i["a"], i["c"], i["r"], i["alpha"],
                                            i["beta"], i["gamma"], i["rho"])
        return self._want

    def hostile(self, proof):
        """a copy of `proof` (numpy fields of the first rows) with the hostile rows' fields written in"""
        out = {f: v.copy() for f, v in proof.items()}
        for i, row in enumerate(self.rows[:len(out["s1"])]):
            if row.hostile:
                for f, v in row.hostile.fields.items():
                    out[f][i] = F.words([v], ALICE_VERIFY_WORDS[f])[0]
        return out

    def expected_verdicts(self):
        """the oracle's verdicts on its own proofs with the hostile fields written in, cached on the case"""
        if self._verify is None:
            import orc
            t, i = self.tables(), self.inputs()
            self._verify = orc.alice_verify(t["N"], t["Nt"], t["h1"], t["h2"], self.kidx, self.sidx, i["c"], self.hostile(self.expected()))
        return self._verify

    def exponents(self):
        """{exponent words: the values the kernel is launched with at that width}, the verifier's taken from the oracle's proofs"""
        pr = self.hostile(self.expected())
        return {8: [x.a for x in self.rows], 24: [x.alpha for x in self.rows], 72: [x.rho for x in self.rows],
                88: [x.gamma for x in self.rows], 25: F.ints(pr["s1"]), 89: F.ints(pr["s2"])}


class BobCase:
    """18 rows of BobProof inputs: the families on beta' (64 words, t = h1^beta' alone: sigma = 0) and gamma (80 words) with b = 0;
    the families on gamma again with beta' = 0, so that the verifier's 81-word t1 = gamma; then honest rows with the reference's ranges"""

    def __init__(self, wb):
        self.wb, self.nst = wb, STATEMENTS[wb]
        keys = _keys()
        r = F.Rng(f"fb-bob-{wb}")
        fam = {w: family(r, w, wb) for w in (64, 80)}
        self.names, self.kidx, self.sidx, v = [], [], [], {f: [] for f in list(BOB_GENERATE_WORDS) + ["beta", "r", "a_enc", "mta"]}
        rp = F.Rng("fb-bob-paillier")                             # the Paillier side does not depend on the width
        specs = [("beta', gamma " + f, f, True) for f in FAMILIES] + [("t1 " + f, f, False) for f in FAMILIES] + [("honest", None, False)] * 4
        for i, (name, f, with_beta_prim) in enumerate(specs):
            k, s = i % PAILLIER_KEYS, statement_index(i, self.nst)
            ek, st = keys[k], keys[PAILLIER_KEYS + s]
            nn = F.bob_nonces(r, ek, st)
            b, beta_prim = r.below(Q), r.below(ek.N)
            if f is not None and with_beta_prim:                  # t = h1^beta' alone
                b, beta_prim, nn["sigma"], nn["gamma"] = 0, fam[64][f], 0, fam[80][f]
            elif f is not None:                                   # t1 = gamma: the verifier's 81-word exponent is chosen
                b, beta_prim, nn["gamma"] = 0, 0, fam[80][f]
            rr = rp.below(ek.N)
            a_enc = _encrypt(k, rp.below(Q), 1 + rp.below(1 << 64))
            mta = pow(a_enc, b, ek.NN) * _encrypt(k, beta_prim, rr) % ek.NN
            self.names.append(name)
            self.kidx.append(k); self.sidx.append(s)
            for g, x in dict(nn, b=b, beta_prim=beta_prim, r=rr, a_enc=a_enc, mta=mta).items():
                v[g].append(x)
        self.values, self.B = v, len(self.names)
        self._want = self._verify = None

    statements, paillier_N, tables = AliceCase.statements, AliceCase.paillier_N, AliceCase.tables

    def inputs(self):
        w = dict(BOB_GENERATE_WORDS, beta=64, r=64, a_enc=128, mta=128)
        return {f: F.words(x, w[f]) for f, x in self.values.items()}

    def python_t(self):
        """t = h1^beta' h2^sigma mod N~ of every row, by Python's pow"""
        Nt, h1, h2 = self.statements()
        return [pow(h1[s], bp, Nt[s]) * pow(h2[s], sg, Nt[s]) % Nt[s] for s, bp, sg in zip(self.sidx, self.values["beta_prim"], self.values["sigma"])]

    def expected(self):
        """the oracle's proof (check = false), cached on the case"""
        if self._want is None:
            import orc
            t, i = self.tables(), self.inputs()
            self._want = orc.bob_generate(t["N"], t["Nt"], t["h1"], t["h2"], self.kidx, self.sidx, i["a_enc"], i["mta"], i["b"], i["beta_prim"],
                                          i["r"], i["alpha"], i["beta"], i["gamma"], i["rho"], i["rho_prim"], i["sigma"], i["tau"], False)[0]
        return self._want

    def expected_verdicts(self):
        if self._verify is None:
            import orc
            t, i = self.tables(), self.inputs()
            self._verify = orc.bob_verify(t["N"], t["Nt"], t["h1"], t["h2"], self.kidx, self.sidx, i["a_enc"], i["mta"], self.expected())
        return self._verify

    def exponents(self):
        pr = self.expected()
        out = {}
        for f, w in BOB_GENERATE_WORDS.items():
            out.setdefault(w, []).extend(self.values[f])
        for f, w in BOB_VERIFY_WORDS.items():
            out.setdefault(w, []).extend(F.ints(pr[f]))
        return out


class SchedCase:
    """`n` honest rows, every value distinct (a scheduling bug lives in particular units): batch(B) = the first B rows.  r = 1, so
    that the ciphertext costs the host one multiplication; the Paillier side is not what these launches are about."""

    def __init__(self, n):
        self.wb, self.nst, self.B = SCHED_WB, STATEMENTS[SCHED_WB], n
        keys = _keys()
        r = F.Rng("fb-sched")
        self.kidx = [i % PAILLIER_KEYS for i in range(n)]
        self.sidx = [statement_index(i, self.nst) for i in range(n)]
        nn = [F.alice_nonces(r, keys[k], keys[PAILLIER_KEYS + s]) for k, s in zip(self.kidx, self.sidx)]
        self.rows = [AliceRow(f"honest {i}", r.below(Q), x["rho"], r.bits(700), x["gamma"], True) for i, x in enumerate(nn)]
        self.r, self.beta = [1] * n, [x["beta"] for x in nn]
        self._z = None

    statements, paillier_N, tables, cipher, inputs, python_z = (AliceCase.statements, AliceCase.paillier_N, AliceCase.tables,
                                                                 AliceCase.cipher, AliceCase.inputs, AliceCase.python_z)


alice_case = functools.lru_cache(maxsize=None)(AliceCase)
bob_case = functools.lru_cache(maxsize=None)(BobCase)
sched_case = functools.lru_cache(maxsize=None)(SchedCase)
