"""The case table of tests/fb_cases.py against the oracle and the source text ALONE: the conditions without which the GPU tests of
tests/test_fixedbase_gpu.py would be vacuous (a table whose planted digits miss the windows they are named for, whose splits never
leave a short run, whose batches never leave an idle lane group, or whose mirrors of the device geometry have drifted from the
kernel, would pass there whatever the ladder does).  Conditions on the inputs, checked against the reference implementation and
Python's own `pow`; nothing here touches the product beyond reading a few lines of its source text."""
import os

import pytest

import fixtures as F
import fb_cases as FB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi_party_ecdsa_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module", params=FB.WIDTHS)
def alice(request):
    return FB.alice_case(request.param)


@pytest.fixture(scope="module", params=FB.BOB_WIDTHS)
def bob(request):
    return FB.bob_case(request.param)


# ---- the mirrors -----------------------------------------------------------------------------------------------------------------------
def test_the_geometry_mirrors_the_source():
    """a change of the kernel's geometry or of the host's rules fails HERE and points at tests/fb_cases.py, whose shapes are chosen
    around them"""
    fb, proofs, internal, gg20, lib, bigint = (source(f) for f in ("mpe_fixedbase.h", "mpe_proofs.h", "mpe_internal.h", "mpe_gg20.h",
                                                                    "mpe_lib.hip", "mpe_bigint.h"))
    assert (FB.FB_EXP_BITS, FB.GROUPS, FB.ROW_WORDS, FB.WAVES_PER_CU, FB.FB_WINDOW_BITS) == (2848, 16, 72, 8, 13)
    # mpe_fixedbase.h: windows of a table and of a launch, the runs of the lane groups, the chain, the digit
    assert "constexpr int FB_EXP_BITS = 89 * 32;" in fb
    assert "inline int fb_windows(int wb) { return (FB_EXP_BITS + wb - 1) / wb; }" in fb
    assert "const int nwin = (exp_words * 32 + FB_WB - 1) / FB_WB;" in fb
    assert "const int S = split, per_wave = C::GROUPS / S;" in fb
    assert "const int part = ln.g & (S - 1), sub = ln.g / S;" in fb
    assert "const int cmax = (nwin + S - 1) / S;" in fb
    assert "const int lo = part * nwin / S, cnt = (part + 1) * nwin / S - lo;" in fb
    assert "const int total = cmax - 1 + lg + 1;" in fb
    assert "return k < cnt ? T + ((size_t)(lo + k) * FB_TE + fb_digit(ex, exp_words, lo + k, wb)) * C::K : one_row;" in fb
    assert "const int bitpos = i * wb, word = bitpos >> 5, sh = bitpos & 31;" in fb
    assert "uint32_t v = ex[word] >> sh;" in fb
    assert "if (sh + wb > 32 && word + 1 < exp_words) v |= ex[word + 1] << (32 - sh);" in fb
    assert "return v & ((1u << wb) - 1u);" in fb
    assert "region = lds + ((ln.g + h < C::GROUPS) ? ln.g + h : ln.g) * C::STRIDE;" in fb
    # mpe_bigint.h: 4 lanes per 2048-bit integer, 18 limbs per lane
    assert "using Cfg2048 = Cfg<2048, MPE_W, MPE_L, 4>;" in bigint and "#define MPE_L 18" in bigint
    assert "static constexpr int GROUPS = 64 / TPI_;" in bigint and "static constexpr int K = L_ * TPI_;" in bigint
    assert (64 // 4, 18 * 4) == (FB.GROUPS, FB.ROW_WORDS)
    # mpe_proofs.h: the split rule, the units, the table bytes, the widths mpe_statements_create_wb takes
    assert "const int cap = ctx->cus * ctx->modexp_waves_per_cu;" in proofs
    assert "if (ctx->fb_split > 0) { while (split * 2 <= ctx->fb_split && split * 2 <= (int)C::GROUPS) split *= 2; }" in proofs
    assert ("else if (ctx->adaptive_lanes) { while (split * 2 <= (int)C::GROUPS && ((long)B * split * 2 + C::GROUPS - 1) / C::GROUPS "
            "<= cap / 2) split *= 2; }") in proofs
    assert "const int units = (B + per_wave - 1) / per_wave;" in proofs
    assert "return (size_t)2 * count * mpe::fb_windows(wb) * ((size_t)1 << wb) * mpe::Cfg2048::K * sizeof(uint32_t);" in proofs
    assert "(wb != 0 && wb < 2) || wb > 16" in proofs
    assert min(FB.WIDTHS) == 2 and max(FB.WIDTHS) == 16
    assert "if (!stm->fb_tab || !ctx->use_fixed_base) return modexp(stm->ms, sel, base, exps, ew);" in proofs
    # mpe_internal.h: the three scheduler modes, the defaults
    assert "if (units <= cap) return (2 * units <= cap && !ctx->no_primaries) ? 2 * units : units;" in internal
    assert "if (2 * units <= cap) { if (!ctx->no_primaries) { a.state = state; a.mode = SCHED_PRIMARIES; } }" in internal
    assert "else if (units > cap) { a.state = state; a.mode = SCHED_ALL; }" in internal
    assert f"int fb_window_bits = {FB.FB_WINDOW_BITS};" in internal and f"int modexp_waves_per_cu = {FB.WAVES_PER_CU};" in internal
    # mpe_gg20.h: the width a key object's tables get
    assert "size_t budget = ctx->fb_budget_bytes ? ctx->fb_budget_bytes : free_b / 4;" in gg20
    assert "int wb = ctx->fb_window_bits;" in gg20
    assert "while (wb > 4 && mpe_statements_table_bytes(nkeysets * n, wb) > budget) --wb;" in gg20
    assert "if (mpe_statements_table_bytes(nkeysets * n, wb) > budget) wb = 0;" in gg20
    assert "s->fb_wb = 0;                                  // no tables unless they are built below" in proofs
    assert "if (ctx->use_fixed_base && wb != 0) {" in proofs
    # mpe_lib.hip: the options the GPU tests set
    assert 'MPE_OPT_INT("fb_split", 0, 64, fb_split)' in lib and 'MPE_OPT_INT("waves_per_cu", 1, 8, modexp_waves_per_cu)' in lib
    assert '{"fb_budget_mb", 0, 1 << 20, [](mpe_ctx* c, long v) { c->fb_budget_bytes = (size_t)v << 20; }' in lib
    assert 'MPE_OPT_BOOL_OFF("no_fixed_base", use_fixed_base)' in lib
    # the exponent widths of the launches: every fb_modexp call of the range proofs
    for words in (8, 72, 24, 88, 25, 89):
        assert f", {words});" in proofs
    bob_src = source("mpe_bob.h")
    for call in ("commit(rows(b, 8), 8, rows(nn->rho, 72), 72, out->z);", "commit(rows(nn->alpha, 24), 24, rows(nn->rho_prim, 88), 88, zp);",
                 "commit(rows(beta_prim, 64), 64, rows(nn->sigma, 72), 72, out->t);", "commit(rows(nn->gamma, 80), 80, rows(nn->tau, 88), 88, w);",
                 "open(pr.s1, 25, pr.s2, 89, pr.z, ok1);", "open(pr.t1, 81, pr.t2, 89, pr.t, ok3);"):
        assert call in bob_src
    launched = set(FB.ALICE_GENERATE_WORDS.values()) | set(FB.ALICE_VERIFY_WORDS.values()) | set(FB.BOB_GENERATE_WORDS.values()) | set(FB.BOB_VERIFY_WORDS.values())
    assert launched == set(FB.EXP_WORDS) and max(FB.EXP_WORDS) * 32 == FB.FB_EXP_BITS


@pytest.mark.parametrize("wb", range(2, 17))
def test_the_digit_and_the_runs_against_a_bit_slice(wb):
    """fb_digit's shifts (the straddle branch and its guard) against (e >> i wb) & mask, and the runs of every split against a plain
    partition of range(nwin): disjoint, in order, complete, lengths within one of each other"""
    r = F.Rng(f"fb-digit-{wb}")
    mask = (1 << wb) - 1
    for words in FB.EXP_WORDS + (1, 2):
        n = FB.nwin(words, wb)
        assert (n - 1) * wb < 32 * words <= n * wb and n <= FB.fb_windows(wb)
        for v in (r.bits(32 * words), (1 << (32 * words)) - 1, 1 << (32 * words - 1), 0x80000001 << (32 * (words - 1)) >> 1):
            assert FB.digits(v, words, wb) == [(v >> (i * wb)) & mask for i in range(n)]
            assert sum(d << (i * wb) for i, d in enumerate(FB.digits(v, words, wb))) == v
        st = FB.straddlers(words, wb)
        assert all((i * wb) // 32 != ((i + 1) * wb - 1) // 32 for i in st)
        assert (32 % wb == 0) == (not st) or words == 1
        assert FB.digits((1 << (32 * words)) - 1, words, wb)[-1] == FB.top_digit_max(words, wb)
        for S in FB.SPLITS:
            runs = [FB.run_of(p, words, wb, S) for p in range(S)]
            assert [i for lo, cnt in runs for i in range(lo, lo + cnt)] == list(range(n))
            assert max(c for _, c in runs) == FB.longest_run(words, wb, S) and min(c for _, c in runs) >= n // S
            assert FB.chain_length(words, wb, S) == -(-n // S) + {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}[S]
    assert FB.fb_windows(wb) == -(-2848 // wb)
    # the kernel comment's example: 217 windows at 13 bits (88 words): the first row is loaded, 216 rows and the final 1 are multiplied
    assert (FB.nwin(88, 13), FB.chain_length(88, 13, 1), FB.chain_length(88, 13, 8)) == (217, 217, 31)


def test_the_split_rule_and_the_scheduler_modes():
    cap = FB.CUS * FB.WAVES_PER_CU
    # option fb_split: rounded down to a power of two, at most the 16 groups of a wave
    assert [FB.split_of(5, s) for s in (1, 2, 3, 4, 7, 8, 15, 16, 17, 64)] == [1, 2, 2, 4, 4, 8, 8, 16, 16, 16]
    assert [FB.split_of(5, S) for S in FB.SPLITS] == list(FB.SPLITS)
    # chosen per launch: what the rest of the suite runs: tiny batches get 16, the full-size ones 1; the thresholds between
    assert FB.split_of(1) == FB.split_of(37) == FB.split_of(cap // 2) == 16 and FB.split_of(262144) == 1
    assert [FB.split_of(B) for B in (1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385)] == [16, 8, 8, 4, 4, 2, 2, 1, 1, 1]
    assert FB.split_of(37, adaptive=False) == 1
    # ... so without option fb_split no batch of the table's sizes would run S = 1, 2, 4 or 8
    assert {FB.split_of(B) for S in FB.SPLITS for B in FB.batch_sizes(S)} == {16}
    # batches per split: one item, a full wave, a wave and one item, several waves with a ragged last one
    assert [FB.batch_sizes(S) for S in FB.SPLITS] == [[1, 16, 17, 37], [1, 8, 9, 37], [1, 4, 5, 37], [1, 2, 3, 37], [1, 2, 37]]
    for S in FB.SPLITS:
        per_wave = FB.GROUPS // S
        assert FB.ROWS % per_wave != 0 or S == 16                  # the last wave of the 37-row batch has idle groups
        assert [FB.units_of(B, S) for B in (1, per_wave, per_wave + 1)] == [1, 1, 2]
        assert all(FB.sched_mode(FB.units_of(B, S), cap)[0] == "primaries" for B in FB.batch_sizes(S))
    # the three scheduler modes under {"fb_split": 16, "waves_per_cu": 1}: one item is one unit, cap = the compute units
    assert FB.SCHED_OPTIONS == {"fb_split": 16, "waves_per_cu": 1}
    for cus in (FB.CUS, 304, 64):
        sizes = FB.sched_sizes(cus)
        assert FB.split_of(sizes[0], FB.SCHED_OPTIONS["fb_split"], cus) == 16
        assert [FB.sched_mode(FB.units_of(B, 16), cus) for B in sizes] == [("primaries", 2 * (cus // 2)), ("static", cus // 2 + 1), ("queue", cus)]
    assert FB.sched_sizes(FB.CUS) == [128, 129, 259]


def test_the_budget_arithmetic():
    """3 statements (t = 1, n = 3, one key set): 19.7 MB at 4 bits, 157 MB at 8, 280 MB at 9, so budgets of 1, 20 and 200 MB select
    no tables, 4 bits and 8 bits"""
    assert FB.table_bytes(3, 4) == 2 * 3 * 712 * 16 * 288 == 19_685_376
    assert FB.table_bytes(3, 8) == 2 * 3 * 356 * 256 * 288 == 157_483_008
    assert FB.table_bytes(3, 9) == 2 * 3 * 317 * 512 * 288 == 280_461_312
    assert FB.table_bytes(1, 13) == 2 * 220 * 8192 * 288 == 1_038_090_240      # 0.5 GB per base at the default width
    assert FB.table_bytes(1, 16) // 2 == 178 * 65536 * 288 == 3_359_637_504     # 3.4 GB per base at 16 bits
    assert FB.table_bytes(1, 8) // 2 == 26_247_168                              # "26 MB per base at 8-bit windows"
    assert {mb: FB.select_width(3, mb << 20) for mb in FB.BUDGETS_MB} == FB.BUDGETS_MB == {1: 0, 20: 4, 200: 8}
    assert FB.table_bytes(3, 4) < 20 << 20 < FB.table_bytes(3, 5) and FB.table_bytes(3, 8) < 200 << 20 < FB.table_bytes(3, 9)
    assert FB.select_width(3, 1 << 40) == 13 and FB.select_width(3, 1 << 40, start=10) == 10
    assert FB.select_width(3, 200 << 20, fixed_base=False) == 0
    # widths below 4 are never selected: the loop stops at 4 and falls to 0
    assert {FB.select_width(c, b << 20) for c in (1, 3, 300) for b in (1, 5, 19, 50, 4000)} <= {0} | set(range(4, 14))


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def test_the_partition_leaves_short_runs():
    """A short run (padded with the form of 1) needs nwin % S != 0.  With the widths the library launches that holds for at least one
    exponent width at every (wb, S > 1) of the table except wb = 2, where nwin = 16 * words divides by every split; and no run is
    ever EMPTY: the shortest exponent has 8 words, 16 windows at 16 bits, one per group at S = 16 (`cnt = 0` is out of reach of every
    caller, so no case can plant it)."""
    ragged = {(wb, S): [w for w in FB.EXP_WORDS if FB.nwin(w, wb) % S] for wb in FB.WIDTHS for S in FB.SPLITS if S > 1}
    for (wb, S), words in ragged.items():
        for w in words:
            runs = [FB.run_of(p, w, wb, S)[1] for p in range(S)]
            assert min(runs) == max(runs) - 1 == FB.longest_run(w, wb, S) - 1
    assert all(ragged[(wb, 16)] for wb in FB.WIDTHS if wb != 2)
    assert all(ragged[(wb, S)] for wb in (5, 11, 13) for S in FB.SPLITS if S > 1)
    assert not any(ragged[(2, S)] for S in FB.SPLITS if S > 1) and all(FB.nwin(w, 2) == 16 * w for w in FB.EXP_WORDS)
    for S in FB.SPLITS[1:]:
        assert sum(1 for wb in FB.WIDTHS if ragged[(wb, S)]) >= 3
    # the widths of AliceProof alone (the sweep) reach a short run wherever any width does, but for (16, 2)
    alice_words = set(FB.ALICE_GENERATE_WORDS.values()) | set(FB.ALICE_VERIFY_WORDS.values())
    assert [k for k, words in ragged.items() if words and not alice_words & set(words)] == []
    assert min(FB.nwin(w, wb) for w in FB.EXP_WORDS for wb in FB.WIDTHS) == 16 == max(FB.SPLITS)
    assert all(FB.run_of(p, w, wb, S)[1] >= 1 for w in FB.EXP_WORDS for wb in FB.WIDTHS for S in FB.SPLITS for p in range(S))


def _covers(vals, words, wb, top_window=None):
    """which of (window, digit) the values reach: digit 0 and the maximal digit in window 0, in the top window, in a straddling one"""
    n = FB.nwin(words, wb)
    top = n - 1 if top_window is None else top_window
    mask = (1 << wb) - 1
    topmax = FB.top_digit_max(words, wb) if top_window is None else mask
    ds = [FB.digits(v, words, wb) for v in vals]
    got = {("low", 0): any(d[0] == 0 for d in ds), ("low", 1): any(d[0] == mask for d in ds),
           ("top", 0): any(d[top] == 0 and v >> (top * wb) == 0 and v for d, v in zip(ds, vals)), ("top", 1): any(d[top] == topmax for d in ds)}
    st = [i for i in FB.straddlers(words, wb) if i < top]
    if st:
        got[("straddle", 0)] = any(d[i] == 0 and d[i - 1] and d[i + 1] for d in ds for i in st)
        got[("straddle", 1)] = any(d[i] == mask and d[i - 1] != mask and d[i + 1] != mask for d in ds for i in st)
    return got


def test_planted_digits_sit_where_the_cases_say(alice):
    """every (wb, exponent width) of AliceProof: digit 0 and the maximal digit in window 0, in the top window and, where the width has
    one, in a window that straddles two words, each beside digits that are neither"""
    wb = alice.wb
    assert len(alice.rows) == FB.ROWS == 37 and len({x.name for x in alice.rows}) == FB.ROWS
    ex = alice.exponents()
    assert sorted(ex) == [8, 24, 25, 72, 88, 89]
    for words, vals in ex.items():
        assert len(vals) == FB.ROWS and all(0 <= v < 1 << (32 * words) for v in vals)
        got = _covers(vals, words, wb)
        assert all(got.values()), (wb, words, [k for k, ok in got.items() if not ok])
        assert (("straddle", 0) in got) == (32 % wb != 0)
        assert {0, 1, (1 << (32 * words)) - 1, 1 << (32 * words - 1)} <= set(vals) or words in (25, 89)
    # the verifier's exponents among the rows both sides ACCEPT: the top window their range reaches is the one holding bit 767 of s1
    # (s1 <= q^3) and bit 2816 of s2 (the 89th word is 1); above that only the hostile rows have digits
    ok = alice.expected_verdicts()
    s1 = [v for v, o in zip(ex[25], ok) if o]
    s2 = [v for v, o in zip(ex[89], ok) if o]
    assert max(s1) == FB.Q3 and any(v >> 2816 == 1 for v in s2) and max(s2) < 1 << 2817
    for vals, words, bit in ((s1, 25, 767), (s2, 89, 2816)):
        got = _covers(vals, words, wb, top_window=bit // wb)
        got.pop(("top", 1))
        assert all(got.values()), (wb, words, "accepted rows", [k for k, ok in got.items() if not ok])
    assert any(FB.digits(v, 25, wb)[767 // wb] == FB.digits(FB.Q3, 25, wb)[767 // wb] for v in s1)
    assert any(FB.digits(v, 89, wb)[2816 // wb] != 0 for v in s2)
    # a = 0 rows show h2^rho alone, rho = 0 rows h1^a alone; the families of both are complete
    assert sum(1 for x in alice.rows if x.a == 0 and x.rho) >= 7 and sum(1 for x in alice.rows if x.rho == 0 and x.a) >= 6
    assert sum(1 for x in alice.rows if x.a == 0 and x.rho == 0) >= 7
    # statements: an index array that repeats and skips, every statement used, within every batch above a few rows
    assert alice.nst == FB.STATEMENTS[wb] and set(alice.sidx) == set(range(alice.nst)) and set(alice.kidx) == set(range(4))
    if alice.nst == 3:
        assert alice.sidx[:8] == [0, 0, 2, 2, 1, 1, 0, 0]


def test_planted_digits_of_the_bob_rows(bob):
    wb = bob.wb
    ex = bob.exponents()
    assert sorted(ex) == [8, 24, 25, 64, 72, 80, 81, 88, 89] and bob.B == 18
    for words in (64, 80):
        got = _covers(ex[words], words, wb)
        assert all(got.values()), (wb, words, [k for k, ok in got.items() if not ok])
    # t1 = gamma on the rows with beta' = 0: the 81-word launch sees the planted digits of the 80-word family below its top word
    got = _covers(ex[81], 81, wb, top_window=(80 * 32 - 1) // wb)
    assert all(got.values()), (wb, 81, [k for k, ok in got.items() if not ok])
    assert set(bob.sidx) == set(range(bob.nst))


def test_the_oracle_agrees_with_python_and_with_the_design(alice):
    want = alice.expected()
    assert F.ints(want["z"]) == alice.python_z()
    Nt, h1, h2 = alice.statements()
    for i, x in enumerate(alice.rows):
        s = alice.sidx[i]
        if x.a == 0:
            assert alice.python_z()[i] == pow(h2[s], x.rho, Nt[s]), x.name
        if x.rho == 0:
            assert alice.python_z()[i] == pow(h1[s], x.a, Nt[s]), x.name
        if x.a == 0 and x.rho == 0:
            assert (F.ints(want["s1"][i:i + 1])[0], F.ints(want["s2"][i:i + 1])[0]) == (x.alpha, x.gamma), x.name
    ok = alice.expected_verdicts()
    assert [bool(o) for o in ok] == [x.accept for x in alice.rows], [x.name for x, o in zip(alice.rows, ok) if bool(o) != x.accept]
    # the range boundaries (s1 = q^3 accepted, the 769-bit s1 rejected), and the row whose s2 has bit 2816 set among accepted ones
    assert [x.accept for x in alice.rows[:5]] == [True, True, True, False, True]
    s1, s2 = F.ints(want["s1"]), F.ints(want["s2"])
    assert (s1[3].bit_length(), s2[3].bit_length()) == (769, 2817) and s1[3] > FB.Q3 and s1[0] == FB.Q3
    assert s2[4] >> 2816 == 1 and alice.rows[4].accept
    rejected = [x.name for x in alice.rows if not x.accept]
    assert len(rejected) == 8 and sum(1 for n in rejected if n.startswith("hostile")) == 6
    # the honest proofs of the hostile rows are fine: it is the written field that both sides reject
    import orc
    t, i = alice.tables(), alice.inputs()
    plain = orc.alice_verify(t["N"], t["Nt"], t["h1"], t["h2"], alice.kidx, alice.sidx, i["c"], want)
    assert all(plain[k] == 1 for k, x in enumerate(alice.rows) if x.hostile) and sum(plain) == FB.ROWS - 2


def test_the_bob_oracle_agrees_with_python(bob):
    want = bob.expected()
    assert F.ints(want["t"]) == bob.python_t()
    Nt, h1, h2 = bob.statements()
    for i, name in enumerate(bob.names):
        if name.startswith("beta'"):
            assert bob.python_t()[i] == pow(h1[bob.sidx[i]], bob.values["beta_prim"][i], Nt[bob.sidx[i]])
        if name.startswith("t1"):
            assert F.ints(want["t1"][i:i + 1])[0] == bob.values["gamma"][i]
    assert list(bob.expected_verdicts()) == [1] * bob.B


def test_the_scheduler_rows_are_distinct():
    c = FB.sched_case(FB.sched_sizes(FB.CUS)[-1])
    assert c.B == 259 and c.wb == 8 and c.nst == 3
    assert len({x.a for x in c.rows}) == len({x.rho for x in c.rows}) == c.B
    assert all(x.accept and 0 < x.a < FB.Q and x.rho.bit_length() > 2200 for x in c.rows)      # honest values of full length
    N = c.paillier_N()
    assert all(ct == (1 + x.a * N[k]) % (N[k] * N[k]) for ct, x, k in zip(c.cipher(), c.rows, c.kidx))


@pytest.mark.parametrize("wb", [5, 11, 13])
def test_the_straddle_guard_decides_digits_in_every_batch(wb):
    """Without `word + 1 < exp_words` the partial top window of row k takes the low bits of row k + 1's first word (rows are dense).
    Several family rows sit beside zero rows, so this is counted: in every batch of two or more rows some prover exponent gets another
    digit, at widths whose 32 * words is no multiple of wb.  (A batch of one row would read past its buffer: nothing to plant there.)"""
    case = FB.alice_case(wb)
    cols = {8: [x.a for x in case.rows], 24: [x.alpha for x in case.rows], 72: [x.rho for x in case.rows], 88: [x.gamma for x in case.rows]}
    assert any(32 * w % wb for w in cols)

    def unguarded(vals, words):
        out = []
        for k, v in enumerate(vals):
            ex = FB.to_words(v, words) + [vals[k + 1] & 0xFFFFFFFF if k + 1 < len(vals) else 0]
            out.append([FB.fb_digit(ex, words + 1, i, wb) for i in range(FB.nwin(words, wb))])
        return out
    for B in sorted({b for S in FB.SPLITS for b in FB.batch_sizes(S)} - {1}):
        changed = {w: [k for k, (g, u) in enumerate(zip((FB.digits(v, w, wb) for v in vals[:B]), unguarded(vals[:B], w))) if g != u]
                   for w, vals in cols.items()}
        assert any(changed.values()), (wb, B)
        assert all(not rows for w, rows in changed.items() if 32 * w % wb == 0)
        if B >= 4:
            assert changed[8] and changed[24] and changed[72]      # h1 and h2, z and w
