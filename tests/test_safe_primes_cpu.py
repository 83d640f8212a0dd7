"""CPU: the restatement of the device's safe-prime search (tests/pyref_safe_primes.py) checks itself against the plain restatement
and the oracle's keystream, the record of its results that the GPU tests read (tests/golden/safe_primes_expected.json) is checked
against it, and the new entry points reject bad arguments before any HIP call."""
import json
import math
import os

import numpy as np
import pytest

import orc
import pyref_primes as R
import pyref_safe_primes as S

HERE = os.path.dirname(os.path.abspath(__file__))
REDO_BELOW = 1 << 17                     # items won at or below this attempt are searched again in full


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "safe_primes_expected.json")) as f:
        return json.load(f)


def test_numpy_keystream_and_filters_are_the_plain_restatement():
    seed, sid = bytes(range(32)), 0x0300000000000011
    blocks = [0, 1, 7, (1 << 25) + 3]                                    # the last one: attempt 2^24, past every counter the search uses
    ks = S.chacha20_blocks(seed, sid, 5, blocks)
    for row, b in zip(ks, blocks):
        assert row.astype("<u4").tobytes() == orc.chacha20_block(seed, b, 5, sid & 0xffffffff, sid >> 32)
    for joint in (False, True):
        att, w = S.candidates(seed, sid, 2, 1000, 600, joint)
        kept = {int(a): S._int(row) for a, row in zip(att, w)}
        for a in range(1000, 1600):
            c = R.candidate(seed, sid, 2, a)
            small = [p for p in R.SMALL_PRIMES if p < S.FILTER_BOUND]
            out = any(c % p == 0 for p in small) or (joint and (c & 2 == 0 or any((c >> 1) % p == 0 for p in small)))
            assert (a in kept) == (not out) and (out or kept[a] == c)
    assert S.prime_attempts(seed, sid, 2, 0, 512)[0] == R.sample_prime(seed, sid, 2)[1]


def test_winners_are_their_candidates_and_safe(golden):
    k, n = golden["keygen"], golden["ntilde"]
    for case in (golden["search"], golden["giveup"]):
        seed = bytes.fromhex(case["seed"])
        for i, (p, a) in enumerate(zip(case["primes"], case["attempts"])):
            assert int(p, 16) == (R.candidate(seed, case["sid"], i, a) if a >= 0 else 0)
    seed = bytes.fromhex(k["seed"])
    got = [R.candidate(seed, R._field(k["counter"], f), g, k["attempts"][f * k["nkeys"] + g]) for f in (0, 1) for g in range(k["nkeys"])]
    assert got == [int(v, 16) for v in k["p"] + k["q"]]
    seed = bytes.fromhex(n["seed"])
    pt, qt = (R.candidate(seed, R._field(n["counter"], f), 0, a) for f, a in zip((2, 3), n["attempts"]))
    assert pt * qt == int(n["Nt"][0], 16) and (pt - 1) * (qt - 1) == int(n["phi"][0], 16)
    winners = [int(v, 16) for v in golden["search"]["primes"]] + got + [pt, qt]
    assert len(winners) == 13 and len(set(winners)) == 13
    for c in winners:
        h = (c - 1) // 2
        assert c.bit_length() == 1024 and R.is_prime(c) and R.is_prime(h) and R.gmp_confirms(c) and R.gmp_confirms(h)


def test_listed_prime_attempts_are_prime_with_a_composite_half(golden):
    """The record lists every attempt below a winner whose candidate is prime (~6400 in all).  What is checked here, for its cost: every
    listed candidate passes a Fermat test to the base 2 (GMP) — NOT a full primality test — and has a composite half (exact: even, a small
    factor, or a failed Fermat test); the restatement's own is_prime and GMP's test run on the first two and the last two entries of
    every item only; the list is recomputed, so shown complete, over the first 4096 attempts of every item only (and over the whole range
    by whoever runs tests/golden/make_safe_primes.py again); its first entry is the plain sample_prime of the stream"""
    s = golden["search"]
    seed = bytes.fromhex(s["seed"])
    for i, (listed, win) in enumerate(zip(s["prime_attempts"], s["attempts"])):
        assert listed == sorted(set(listed)) and listed and listed[-1] < win
        assert listed[0] == R.sample_prime(seed, s["sid"], i)[1]
        assert [a for a in listed if a < 4096] == S.prime_attempts(seed, s["sid"], i, 0, min(4096, win))
        blocks = np.array(listed, dtype=np.int64)
        lo = S._half_words(S.chacha20_blocks(seed, s["sid"], i, 2 * blocks + 1))
        hi = S._half_words(S.chacha20_blocks(seed, s["sid"], i, 2 * blocks))
        lo[:, 0] |= np.uint32(1)
        hi[:, 15] |= np.uint32(0x80000000)
        w = np.ascontiguousarray(np.concatenate([lo, hi], axis=1))
        assert S._fermat2(w).all()
        for a, row in zip(listed, w):
            h = S._int(row) >> 1
            assert h % 2 == 0 or math.gcd(h, R._PRIMORIAL) != 1 or pow(2, h - 1, h) != 1, a
        for k in sorted({0, 1, len(listed) - 2, len(listed) - 1} & set(range(len(listed)))):
            c = R.candidate(seed, s["sid"], i, listed[k])
            assert c == S._int(w[k]) and R.is_prime(c) and R.gmp_confirms(c) and not R.is_prime(c >> 1)


def test_early_winners_are_searched_again_in_full(golden):
    s = golden["search"]
    seed = bytes.fromhex(s["seed"])
    early = [i for i, a in enumerate(s["attempts"]) if a <= REDO_BELOW]
    assert len(early) >= 2 and max(s["attempts"]) >= 1 << 19 and s["fail"] == 0      # several passes at any block size
    for i in early:
        p, a = S.sample_safe_prime(seed, s["sid"], i, REDO_BELOW + 1)
        assert (hex(p), a) == (s["primes"][i], s["attempts"][i])


def test_give_up_and_key_material_records(golden):
    s, u, k, n = golden["search"], golden["giveup"], golden["keygen"], golden["ntilde"]
    assert (u["seed"], u["sid"], u["batch"]) == (s["seed"], s["sid"], s["batch"])
    assert 0 < u["fail"] < u["batch"] and u["fail"] == sum(a < 0 for a in u["attempts"])
    assert u["attempts"] == [a if a < u["max_attempts"] else -1 for a in s["attempts"]]
    assert S.sample_safe_prime(bytes.fromhex(u["seed"]), u["sid"], 0, 4096) == (0, -1)        # a cap below the winner: a give-up
    for i in range(k["nkeys"]):
        assert int(k["p"][i], 16) * int(k["q"][i], 16) == int(k["N"][i], 16)
    seed = bytes.fromhex(n["seed"])
    Nt, h1, h2, xhi, xhi_inv, xi, phi = (int(n[f][0], 16) for f in ("Nt", "h1", "h2", "xhi", "xhi_inv", "xi", "phi"))
    assert xi * (phi - xhi_inv) % phi == 1 and xhi == phi - xi and h2 == pow(h1, xi, Nt) and pow(h2, phi - xhi_inv, Nt) == h1
    assert xi == R.draw_xi(seed, R._field(n["counter"], 5), 0, phi)
    h1w, _ = orc.sample_below(1, seed, R._field(n["counter"], 4), R._words([Nt], 64), 64)
    assert h1 == sum(int(x) << (32 * j) for j, x in enumerate(h1w[0]))
    assert k["fail"] == 0 and n["fail"] == 0


def test_safe_entry_points_refuse_a_null_context_before_any_hip_call():
    """no context can exist without a GPU: what this checks is that the new entry points answer MPE_E_ARG for a NULL context or NULL
    pointers, whatever the other arguments, instead of touching HIP.  The range checks (bits, counter, max_attempts) are exercised with
    a live context in tests/test_safe_primes_gpu.py::test_bad_arguments_are_refused_with_a_context"""
    import ctypes as C
    from multi_party_ecdsa_amd import _native as N
    seed = bytes(32)
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    L = N.lib
    for bits in (512, 2048, 0, 1024):
        assert L.mpe_sample_safe_prime(None, 1, seed, 0, bits, 0, p, p, p, None) == N.MPE_E_ARG
    assert L.mpe_sample_safe_prime(None, 1, None, 0, 1024, 0, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_paillier_keygen_safe_primes(None, 1, seed, 0, 0, p, p, p, p, None) == N.MPE_E_ARG
    assert L.mpe_paillier_keygen_safe_primes(None, 1, None, 1 << 56, 0, None, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_ntilde_generate_safe_primes(None, 1, seed, 0, 0, p, p, p, p, p, p, None) == N.MPE_E_ARG
    assert L.mpe_ntilde_generate_safe_primes(None, 1, None, 0, -1, None, None, None, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_prime_search_counts(None, None, 0) == N.MPE_E_ARG
