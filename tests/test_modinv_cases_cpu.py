"""The case table of tests/modinv_cases.py against the oracle ALONE: the conditions without which the GPU tests of
tests/test_modinv_gpu.py would be vacuous (a table whose launches take the lane-serial kernel, whose buckets never leave a ragged
chunk, whose non-units are not non-units, or whose bulk case falls back in most chunks, would pass there whatever the batched
route does).  Conditions on the inputs, checked against the reference implementation and Python's own `pow`; nothing here touches
the product beyond reading a few lines of its source text."""
import os

import numpy as np
import pytest

import fixtures as F
import modinv_cases as MC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi_party_ecdsa_amd", "csrc")


@pytest.fixture(scope="module", params=MC.BITS)
def table(request):
    return request.param, MC.cases(request.param)


def test_the_thresholds_mirror_the_source():
    """a change of a routing threshold fails HERE and points at tests/modinv_cases.py, whose shapes are chosen around them"""
    assert (MC.LANE_MAX_B, MC.PAR_ITEMS, MC.CHUNK_SMALL, MC.CHUNK_LARGE) == (32, 32768, 16, 64)
    with open(os.path.join(CSRC, "mpe_modinv.h")) as f:
        modinv = f.read()
    with open(os.path.join(CSRC, "mpe_internal.h")) as f:
        internal = f.read()
    assert f"if (B <= {MC.LANE_MAX_B} && ms->count > 1) {{" in modinv
    assert f"const int CH = B <= ctx->par_items ? {MC.CHUNK_SMALL} : {MC.CHUNK_LARGE};" in modinv
    assert f"int par_items = {MC.PAR_ITEMS};" in internal
    assert f"per = (nmod + {MC.PLAN_LANES - 1}) / {MC.PLAN_LANES}" in modinv
    assert "maxch = B / CH + (nmod < B ? nmod : B) + 2;" in modinv           # MC.max_chunks
    assert "const int cap = ctx->cus * ctx->modexp_waves_per_cu;" in modinv   # MC.trip_capacity


def test_every_case_takes_the_batched_route(table):
    bits, cases = table
    assert list(cases) == MC.NAMES
    for nm, c in cases.items():
        assert c.bits == bits and MC.route(c.B, c.count) == "batched", nm
        assert c.B > MC.LANE_MAX_B or c.count == 1, nm
        assert all(0 <= v < c.mods[m] for v, m in zip(c.a, c.idx)), nm      # inputs are reduced, as every call site guarantees
        assert all(n & 1 for n in c.mods), nm
        assert (c.chunk == MC.CHUNK_LARGE) == (nm == "64-item chunks"), nm
    assert cases["64-item chunks"].B == MC.BULK_B > MC.PAR_ITEMS
    assert [cases[f"single modulus B={B}"].B for B in (1, 2, 16, 17)] == [1, 2, 16, 17]


def test_the_geometry_the_cases_are_named_for(table):
    bits, cases = table
    g = cases["geometry"].geometry
    assert g.sizes == [0, 1, 15, 16, 17, 31, 32, 33, 47, 1, 16, 5] and cases["geometry"].count == 12
    assert g.perm != sorted(g.perm)                                          # interleaved: the counting sort has work to do
    lens = g.chunk_lengths
    assert {1, 5, 15, 16} <= set(lens) and any(a != b for a, b in zip(lens, lens[1:]))      # neighbours of one wave differ in length
    per_wave = MC.GROUPS_PER_WAVE[bits]
    assert any(len(set(lens[w:w + per_wave])) > 1 for w in range(0, len(lens), per_wave))
    # more moduli than the plan kernel has lanes: runs of 2 and of 3 moduli per lane with idle tail lanes; unused moduli at both ends
    for nmod, per in ((65, 2), (130, 3)):
        c = cases[f"{nmod} moduli"]
        g = c.geometry
        assert c.count == nmod and -(-nmod // MC.PLAN_LANES) == per and -(-nmod // per) < MC.PLAN_LANES
        assert 190 <= c.B <= 210
        empty = [m for m, s in enumerate(g.sizes) if s == 0]
        assert g.sizes[0] == 0 and g.sizes[-1] == 0 and 0.25 * nmod <= len(empty) <= 0.45 * nmod
        assert any(s > 0 for s in g.sizes[per * (nmod // per - 1):])          # the last working lane has items to place
    # one chunk per item; values of the modulus table repeat at different indices
    c = cases["per-item moduli"]
    assert c.mod_idx is None and c.count >= c.B == 40 and set(c.geometry.chunk_lengths) == {1}
    assert len(set(c.mods)) < c.count and c.geometry.sizes[c.B:] == [0] * (c.count - c.B)
    # two trips of the sweep kernels under waves_per_cu = 1
    c = cases["two trips"]
    cap = MC.trip_capacity(bits, c.options["waves_per_cu"])
    assert c.options == {"waves_per_cu": 1} and c.mod_idx is None and c.count == c.B == {2048: 4200, 4096: 2100}[bits]
    assert len(c.geometry.chunks) > cap and MC.max_chunks(c.B, c.count) <= 2 * cap
    assert len(set(c.mods)) == 256
    assert all(not x.options for nm, x in cases.items() if nm != "two trips")
    # 64-item chunks
    c = cases["64-item chunks"]
    g = c.geometry
    assert set(MC.BULK_SMALL_SIZES) == {1, 63, 64, 65, 127, 128, 129} and set(MC.BULK_SMALL_SIZES) < set(g.sizes)
    assert max(g.sizes) > 30000 and {1, 63, 64} <= set(g.chunk_lengths) and max(g.chunk_lengths) == 64
    assert g.perm != sorted(g.perm)


def test_non_units_sit_where_the_cases_say(table):
    bits, cases = table
    c = cases["non-units, one modulus"]
    g = c.geometry
    assert c.B == 64 and c.count == 1 and [len(x) for _, x in g.chunks] == [16] * 4
    in_chunk = [sorted(g.where[i][2] for i in c.planted if g.where[i][1] == k) for k in range(4)]
    assert in_chunk == [[0], [15], list(range(16)), []]
    assert 0 in [c.a[i] for i in g.chunks[2][1]]
    c2 = cases["non-units, clean second modulus"]
    g2 = c2.geometry
    assert c2.count == 2 and g2.sizes == [64, 64] and all(c2.idx[i] == 0 for i in c2.planted)
    assert [c2.a[i] for i in g2.buckets[0]] == c.a
    # every 64-item wave of the counting sort holds 32 items of each modulus: whole chunks, whichever wave comes first
    assert all(sum(1 for m in c2.idx[w:w + 64] if m == 0) % MC.CHUNK_SMALL == 0 for w in range(0, c2.B, 64))
    # the bulk case: about one chunk in fifty, and at least 90 % of the chunks all-unit in ANY order of the buckets' items
    c = cases["64-item chunks"]
    nch = len(c.geometry.chunks)
    assert nch // 60 <= len(c.planted) <= nch // 40
    assert 0 in [c.a[i] for i in c.planted]
    dirty = {c.geometry.where[i][1] for i in c.planted}
    assert len(dirty) == len(c.planted) and 10 * len(c.planted) <= nch
    assert {c.geometry.where[i][2] for i in c.planted} >= {0, 63}


def test_the_oracles_verdicts_are_the_planted_ones(table):
    bits, cases = table
    for nm, c in cases.items():
        out, ok = c.expected()
        assert ok.shape == (c.B,) and out.shape == (c.B, c.k32)
        assert set(np.flatnonzero(ok == 0).tolist()) == set(c.planted), nm
        assert not out[ok == 0].any(), nm
        if c.family in ("non-unit", "bulk"):
            assert 0 < len(c.planted) < c.B, nm                              # both verdicts in one launch
        if c.family in ("geometry", "single", "many", "per-item", "two-trip"):
            assert not c.planted, nm
    assert any(c.planted for c in cases.values() if c.family == "edge")
    # most chunks of the bulk case get their answers from the Montgomery trick, not from the fallback
    c = cases["64-item chunks"]
    ok = c.expected()[1]
    clean = sum(1 for _, items in c.geometry.chunks if ok[items].all())
    assert clean >= 0.9 * len(c.geometry.chunks)


def test_the_edge_values_are_edge_values(table):
    bits, cases = table
    mods = MC.edge_moduli(bits)
    assert list(mods) == MC.EDGE_MODULI
    assert mods["2^bits - 1"] == 2 ** bits - 1 and mods["2^(bits-1) + 1"] == 2 ** (bits - 1) + 1 and mods["3"] == 3
    assert mods["N"] in (F.load_keys()[0].N, F.load_keys()[0].NN) and mods["N"].bit_length() > bits - 2
    assert mods["40 bits short"].bit_length() == bits - 40 and mods["40 bits short"] & 1
    for label, n in mods.items():
        own, shared = cases[f"edges mod {label}, own chunks"], cases[f"edges mod {label}, shared chunks"]
        assert own.a == shared.a and own.mods == [n] * own.B and shared.mods == [n]
        assert set(own.geometry.chunk_lengths) == {1}                         # the value itself is what the wave gcd inverts
        vals = set(own.a)
        want = {1, 2, n - 1, n - 2, (n + 1) // 2}
        for k in MC.EDGE_KS(bits):
            want |= {1 << k, (1 << k) - 1, (1 << k) + 1, n - (1 << k)}
        assert {v for v in want if 0 < v < n} <= vals, label
        if n > 3:
            assert {1, 31, 32, 33, 63, 64, 65} <= {v.bit_length() - 1 for v in vals if v & (v - 1) == 0}
            # a run of at least 96 one bits and a run of at least 96 zero bits above bit 0: carries cross 32- and 64-bit lanes
            assert any(v & (v + 1) == 0 and v.bit_length() >= 96 for v in vals), label
            assert any((n - v) & (n - v + 1) == 0 and (n - v).bit_length() >= 96 for v in vals), label
            pats = [int(w * (bits // 32), 16) >> sh for w in ("AAAAAAAA", "55555555") for sh in (0, 41)]
            assert sum(1 for v in pats if v in vals) >= 2, label
        inv_closed = [v for i, v in enumerate(own.a) if i not in own.planted]
        assert all(pow(v, -1, n) in vals for v in inv_closed), label            # results are edge values too


def test_the_oracle_agrees_with_python(table):
    bits, cases = table
    checked = 0
    for nm, c in cases.items():
        out, ok = c.expected()
        rows = c.python_rows()
        assert c.B <= MC.BULK_ROWS or 256 <= len(rows) <= 300, nm
        got = F.ints(out[rows])
        for i, g in zip(rows, got):
            try:
                want, wok = pow(c.a[i], -1, c.mods[c.idx[i]]), 1
            except ValueError:
                want, wok = 0, 0
            assert (g, int(ok[i])) == (want, wok), (nm, i)
        checked += len(rows)
    assert checked < 4000
