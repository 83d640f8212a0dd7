"""Launches of the batched modular inversion (`mpe_modinv`, multi_party_ecdsa_amd/csrc/mpe_modinv.h) that take the BATCHED route —
counting sort by modulus, up-sweep, one wave-cooperative gcd per chunk, down-sweep, masked lane-kernel fallback — at the shapes where
its stages can go wrong: ragged chunks, empty buckets, more moduli than the plan kernel has lanes, one chunk per item, a second trip of
the sweep kernels, non-units beside units, limb patterns that make carries run across lanes, 64-item chunks.  Pure Python: values,
moduli and the geometry the device derives from them; nothing here touches the product.

Moduli have KNOWN factors (p_i q_j of tests/golden/keys16.json, squared for 4096 bit), so a random residue is a unit with
overwhelming probability and every non-unit of the random families is planted (a multiple of a prime factor, or 0).

`cases(bits)` -> {name: Case}; `Case.expected()` -> the oracle's (out, ok), cached on the case;
tests/test_modinv_cases_cpu.py checks that the table is not vacuous, tests/test_modinv_gpu.py runs it on the GPU."""
import functools
import math

import fixtures as F

# ---- the routing of launch_modinv, mirrored (tests/test_modinv_cases_cpu.py pins these to the source text) ---------------------------
LANE_MAX_B = 32            # mpe_modinv.h, launch_modinv: `B <= 32 && ms->count > 1` takes the lane-serial kernel
PAR_ITEMS = 32768          # mpe_internal.h, mpe_ctx: `par_items = 32768` (not a context option)
CHUNK_SMALL, CHUNK_LARGE = 16, 64    # mpe_modinv.h, launch_modinv_batched: `B <= ctx->par_items ? 16 : 64` items per chunk
PLAN_LANES = 64            # inv_plan_kernel: one wave, every lane a run of ceil(nmod / 64) moduli
GROUPS_PER_WAVE = {2048: 16, 4096: 8}      # mpe_bigint.h: Cfg2048 has 4 threads per integer, Cfg4096 has 8
TWO_TRIP_OPTIONS = {"waves_per_cu": 1}     # the sweep kernels' grid is capped at (compute units) x 1 waves
CUS = 256                  # compute units of an MI355X (the GPU test asserts the device's own count against the case)

BITS = (2048, 4096)
BULK_ROWS = 512            # cases above this size are compared with Python on a strided sample, the others on every row
GEOMETRY_SIZES = [0, 1, 15, 16, 17, 31, 32, 33, 47, 1, 16, 5]
BULK_B = PAR_ITEMS + 777
BULK_SMALL_SIZES = [1, 63, 64, 65, 127, 128, 129]       # + one bucket with the large remainder
EDGE_KS = lambda bits: [1, 31, 32, 33, 63, 64, 65, bits - 2]


def route(B, count):
    return "lane" if B <= LANE_MAX_B and count > 1 else "batched"


def chunk_items(B):
    return CHUNK_SMALL if B <= PAR_ITEMS else CHUNK_LARGE


def max_chunks(B, count):
    """the size of the chunk table, which is what the sweep kernels' trip count is computed from"""
    return B // chunk_items(B) + min(count, B) + 2


def trip_capacity(bits, waves_per_cu, cus=CUS):
    """chunks that one trip of inv_up_kernel / inv_down_kernel serves: one lane group per chunk"""
    return cus * waves_per_cu * GROUPS_PER_WAVE[bits]


class Geometry:
    """buckets and chunks as inv_count / inv_plan / inv_perm make them, with the items of a bucket in launch order.  (On the device the
    64-item waves of a launch append to a bucket in the order their atomics arrive, so above 64 items the chunk an item lands in is
    nominal; the cases that need a non-unit in a given chunk keep their buckets' wave shares at multiples of the chunk size.)"""

    def __init__(self, idx, count, chunk):
        self.buckets = [[] for _ in range(count)]
        for i, m in enumerate(idx):
            self.buckets[m].append(i)
        self.sizes = [len(b) for b in self.buckets]
        self.chunks = []                      # (modulus index, [items])
        self.where = [None] * len(idx)        # item -> (modulus index, chunk number, position in the chunk)
        for m, b in enumerate(self.buckets):
            for s in range(0, len(b), chunk):
                for pos, i in enumerate(b[s:s + chunk]):
                    self.where[i] = (m, len(self.chunks), pos)
                self.chunks.append((m, b[s:s + chunk]))
        self.perm = [i for b in self.buckets for i in b]

    @property
    def chunk_lengths(self):
        return [len(c) for _, c in self.chunks]


class Case:
    def __init__(self, name, bits, mods, mod_idx, a, options=None, planted=(), family=""):
        self.name, self.bits, self.k32 = name, bits, bits // 32
        self.mods, self.mod_idx, self.a = list(mods), None if mod_idx is None else list(mod_idx), list(a)
        self.options = dict(options or {})
        self.planted = frozenset(planted)     # the rows that have no inverse
        self.family = family
        self.B, self.count = len(self.a), len(self.mods)
        assert self.mod_idx is not None or self.count == 1 or self.count >= self.B
        self._want = self._geo = self._words = None

    @property
    def idx(self):
        """the modulus index of every row, as `sel_of` resolves a missing mod_idx"""
        if self.mod_idx is not None:
            return self.mod_idx
        return [0] * self.B if self.count == 1 else list(range(self.B))

    @property
    def chunk(self):
        return chunk_items(self.B)

    @property
    def geometry(self):
        if self._geo is None:
            self._geo = Geometry(self.idx, self.count, self.chunk)
        return self._geo

    def words(self):
        """(moduli, values) as arrays of 32-bit words"""
        if self._words is None:
            self._words = F.words(self.mods, self.k32), F.words(self.a, self.k32)
        return self._words

    def expected(self):
        """the oracle's (out, ok), cached on the case"""
        if self._want is None:
            import orc
            mw, aw = self.words()
            self._want = orc.modinv(mw, aw, self.idx)
        return self._want

    def python_rows(self):
        """the rows compared with Python's pow(a, -1, n)"""
        if self.B <= BULK_ROWS:
            return list(range(self.B))
        return sorted(set(range(0, self.B, max(1, self.B // 256))) | set(self.planted))


# ---- moduli with known factors ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def modulus_table(bits):
    """256 moduli [(n, a prime factor, another prime factor)]: p_i q_j, squared for 4096 bit"""
    keys = F.load_keys()
    e = bits // 2048
    return [((k.p * l.q) ** e, k.p, l.q) for k in keys for l in keys]


def _unit(r, n):
    return 1 + r.below(n - 1)


def _non_unit(r, n, f):
    """a non-zero multiple of the factor f below n"""
    return f * (1 + r.below(n // f - 1))


def _interleave(r, sizes):
    """modulus indices with the given bucket sizes, shuffled: perm is not the identity"""
    idx = [m for m, c in enumerate(sizes) for _ in range(c)]
    keyed = sorted((r.bits(48), i) for i in range(len(idx)))
    return [idx[i] for _, i in keyed]


def _random_case(name, bits, table, mod_idx, seed, family, options=None):
    r = F.Rng(seed)
    return Case(name, bits, [t[0] for t in table], mod_idx, [_unit(r, table[m][0]) for m in mod_idx], options=options, family=family)


def _geometry_case(bits):
    tab = modulus_table(bits)[3:3 + len(GEOMETRY_SIZES)]
    r = F.Rng(f"modinv-geometry-{bits}")
    return _random_case("geometry", bits, tab, _interleave(r, GEOMETRY_SIZES), f"modinv-geometry-values-{bits}", "geometry")


def _single_modulus_cases(bits):
    out = []
    for B in (1, 2, 16, 17):
        r = F.Rng(f"modinv-single-{bits}-{B}")
        n = modulus_table(bits)[20 + B][0]
        out.append(Case(f"single modulus B={B}", bits, [n], None, [_unit(r, n) for _ in range(B)], family="single"))
    return out


def _many_moduli_cases(bits):
    out = []
    for nmod in (65, 130):
        r = F.Rng(f"modinv-many-{bits}-{nmod}")
        unused = {0, nmod - 1} | {m for m in range(nmod) if m % 3 == 1}
        used = [m for m in range(nmod) if m not in unused]
        B = 200
        idx = [used[r.below(len(used))] for _ in range(B)]
        idx[:len(used)] = used                                   # every used modulus has an item
        out.append(_random_case(f"{nmod} moduli", bits, modulus_table(bits)[:nmod], idx, f"modinv-many-values-{bits}-{nmod}", "many"))
    return out


def _per_item_case(bits):
    B, count = 40, 43                                             # count >= B: row i takes modulus i, the last three are idle
    tab = modulus_table(bits)
    mods = [tab[(7 * i) % 9][0] for i in range(count)]            # nine values, repeated at different indices
    r = F.Rng(f"modinv-per-item-{bits}")
    return Case("per-item moduli", bits, mods, None, [_unit(r, mods[i]) for i in range(B)], family="per-item")


def _two_trip_case(bits):
    B = {2048: 4200, 4096: 2100}[bits]
    tab = modulus_table(bits)
    mods = [tab[i % len(tab)][0] for i in range(B)]
    r = F.Rng(f"modinv-two-trips-{bits}")
    return Case("two trips", bits, mods, None, [_unit(r, mods[i]) for i in range(B)], options=TWO_TRIP_OPTIONS, family="two-trip")


def _non_unit_cases(bits):
    """64 items of one modulus = four chunks of 16: a non-unit first in chunk 0, last in chunk 1, chunk 2 all non-units (a = 0 among
    them), chunk 3 clean.  Then the same 64 items with 64 clean items of a second modulus between them: every wave of the counting
    sort holds 32 items of each modulus, so the chunks hold the same items whichever wave's atomic arrives first."""
    (n, p, q), (n2, _, _) = modulus_table(bits)[77], modulus_table(bits)[142]
    r = F.Rng(f"modinv-non-units-{bits}")
    a = [_unit(r, n) for _ in range(64)]
    planted = {0, 31} | set(range(32, 48))
    a[0], a[31] = _non_unit(r, n, p), _non_unit(r, n, q)
    for i in range(32, 48):
        a[i] = _non_unit(r, n, p if i % 2 else q)
    a[37] = 0
    a[40] = p                                                     # the factor itself
    one = Case("non-units, one modulus", bits, [n], None, a, planted=planted, family="non-unit")
    idx2, a2, planted2 = [], [], set()
    for i in range(64):
        if i in planted:
            planted2.add(len(a2))
        idx2 += [0, 1]
        a2 += [a[i], _unit(r, n2)]
    two = Case("non-units, clean second modulus", bits, [n, n2], idx2, a2, planted=planted2, family="non-unit")
    return [one, two]


def edge_moduli(bits):
    n, _, _ = modulus_table(bits)[0]                              # keys[0]: N at 2048 bit, N^2 at 4096 bit
    r = F.Rng(f"modinv-edge-modulus-{bits}")
    vals = [(1 << bits) - 1, (1 << (bits - 1)) + 1, n, 3, r.bits(bits - 40) | (1 << (bits - 41)) | 1]
    return dict(zip(EDGE_MODULI, vals))


def edge_values(bits, n):
    """limb patterns that make carries and borrows run across the lanes of the wave gcd (32-bit lanes at 2048 bit, 64-bit lanes at
    4096 bit), kept where they are below n; then the inverses of the units among them, so that results are edge values too"""
    k32 = bits // 32
    vals = [1, 2, n - 1, n - 2, (n + 1) // 2]
    for k in EDGE_KS(bits):
        vals += [1 << k, (1 << k) - 1, (1 << k) + 1, n - (1 << k)]
    vals += [int("AAAAAAAA" * k32, 16), int("55555555" * k32, 16)]
    vals += [int("AAAAAAAA" * k32, 16) >> 41, int("55555555" * k32, 16) >> 41]       # the same patterns below the short modulus
    vals += [(1 << (32 * (k32 - 1) + 7)) - 1, (1 << (32 * (k32 - 3))) - 1]           # all words 0xFFFFFFFF below the top
    vals += [n - ((1 << (32 * (k32 - 3))) - 1)]
    seen, out = set(), []
    for v in vals:
        if 0 < v < n and v not in seen:
            seen.add(v)
            out.append(v)
    for v in list(out):
        if math.gcd(v, n) == 1:
            w = pow(v, -1, n)
            if w not in seen:
                seen.add(w)
                out.append(w)
    return out


def _edge_cases(bits):
    """every value in a chunk of its own (per-item moduli: the value itself is what the wave gcd inverts) and again with all values of
    a modulus sharing chunks (the sweeps multiply edge values).  Padded by repetition to more than LANE_MAX_B rows."""
    out = []
    for label, n in edge_moduli(bits).items():
        vals = edge_values(bits, n)
        while len(vals) <= LANE_MAX_B:
            vals = vals + vals
        planted = {i for i, v in enumerate(vals) if math.gcd(v, n) != 1}
        out.append(Case(f"edges mod {label}, own chunks", bits, [n] * len(vals), None, vals, planted=planted, family="edge"))
        out.append(Case(f"edges mod {label}, shared chunks", bits, [n], None, vals, planted=planted, family="edge"))
    return out


def _bulk_case(bits):
    """64-item chunks: above PAR_ITEMS items.  Eight moduli (seven small buckets and the remainder), items shuffled; non-units in
    about one chunk in fifty of the large bucket (first, last and middle positions of the launch-order chunks) and at the head of the
    second chunk of the 127-item bucket."""
    sizes = BULK_SMALL_SIZES + [BULK_B - sum(BULK_SMALL_SIZES)]
    tab = modulus_table(bits)[100:100 + len(sizes)]
    r = F.Rng(f"modinv-bulk-{bits}")
    idx = _interleave(r, sizes)
    a = [r.bits(bits) % tab[m][0] for m in idx]
    geo = Geometry(idx, len(sizes), CHUNK_LARGE)
    planted = set()
    big = [c for m, c in geo.chunks if m == len(sizes) - 1]
    for j, c in enumerate(big[3::50]):
        n, p, q = tab[-1]
        i = c[(0, len(c) - 1, len(c) // 2)[j % 3]]
        a[i] = (_non_unit(r, n, p), 0, _non_unit(r, n, q))[j % 3]
        planted.add(i)
    i = geo.buckets[4][64]
    a[i] = _non_unit(r, tab[4][0], tab[4][1])
    planted.add(i)
    return Case("64-item chunks", bits, [t[0] for t in tab], idx, a, planted=planted, family="bulk")


EDGE_MODULI = ["2^bits - 1", "2^(bits-1) + 1", "N", "3", "40 bits short"]
# the families in table order: (the names of their cases, the builder of all of them).  Names are static, so that a test can be
# parametrised over them without building a value; a family is built when one of its cases is first asked for.
FAMILIES = [
    (["geometry"], lambda bits: [_geometry_case(bits)]),
    ([f"single modulus B={B}" for B in (1, 2, 16, 17)], _single_modulus_cases),
    (["65 moduli", "130 moduli"], _many_moduli_cases),
    (["per-item moduli"], lambda bits: [_per_item_case(bits)]),
    (["two trips"], lambda bits: [_two_trip_case(bits)]),
    (["non-units, one modulus", "non-units, clean second modulus"], _non_unit_cases),
    ([f"edges mod {m}, {how} chunks" for m in EDGE_MODULI for how in ("own", "shared")], _edge_cases),
    (["64-item chunks"], lambda bits: [_bulk_case(bits)]),
]
NAMES = [nm for nms, _ in FAMILIES for nm in nms]


@functools.lru_cache(maxsize=None)
def _family(bits, k):
    nms, build = FAMILIES[k]
    got = build(bits)
    assert [c.name for c in got] == nms, (nms, [c.name for c in got])
    return {c.name: c for c in got}


def case(bits, name):
    for k, (nms, _) in enumerate(FAMILIES):
        if name in nms:
            return _family(bits, k)[name]
    raise KeyError(name)


def cases(bits):
    return {nm: case(bits, nm) for nm in NAMES}
