"""CPU: the pure-Python restatement of the device's prime search (tests/pyref_primes.py) checks itself, the record of its results
that the GPU tests read (tests/golden/primes_expected.json) is checked against it, and the new entry points reject bad arguments
before any HIP call."""
import json
import os

import orc
import pyref_primes as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
    with open(os.path.join(HERE, "golden", "primes_expected.json")) as f:
        return json.load(f)


def test_attempt_is_its_own_128_bytes_with_top_and_bottom_bit_set():
    seed, sid = bytes(range(32)), 0x0300000000000011
    for a in range(4):                                                   # the oracle's BigInt::sample of the first 128 (a + 1) bytes: attempt a is its low 1024 bits
        w = orc.sample_bits(3, seed, sid, 1024 * (a + 1), 32 * (a + 1))
        for g in range(3):
            raw = sum(int(x) << (32 * j) for j, x in enumerate(w[g][:32]))
            c = R.candidate(seed, sid, g, a)
            assert c == raw | 1 | (1 << 1023) and c.bit_length() == 1024 and c & 1
            assert R.keystream(seed, sid, g, 128 * a, 128) == raw.to_bytes(128, "big")


def test_reference_primes_agree_with_gmp_and_are_the_lowest_attempt():
    g = _golden()["search"]
    seed = bytes.fromhex(g["seed"])
    early = sorted(range(g["batch"]), key=lambda i: g["attempts"][i])[:3]
    for i in early:                                                      # whole searches for the items that finish first
        p, a = R.sample_prime(seed, g["sid"], i)
        assert (hex(p), a) == (g["primes"][i], g["attempts"][i])
        assert R.gmp_confirms(p) and not any(R.is_prime(R.candidate(seed, g["sid"], i, b)) for b in range(a))
    assert R.is_prime(2) and R.is_prime(6361) and R.is_prime(6373) and not R.is_prime(6367 * 6373) and not R.is_prime(6373 ** 2) and not R.is_prime(1)


def test_recorded_expectations_are_what_the_restatement_gives():
    g = _golden()
    s = g["search"]
    assert min(s["attempts"]) <= 8 and max(s["attempts"]) >= 1500 and s["fail"] == 0       # several passes whatever the block size
    for case in (s, g["giveup"]):
        seed = bytes.fromhex(case["seed"])
        for i, (p, a) in enumerate(zip(case["primes"], case["attempts"])):
            assert int(p, 16) == (R.candidate(seed, case["sid"], i, a) if a >= 0 else 0)
    u = g["giveup"]
    assert 0 < u["fail"] < u["batch"] and u["fail"] == sum(a < 0 for a in u["attempts"]) and all(a < u["max_attempts"] for a in u["attempts"])
    for i in range(6):                                                   # 64 attempts per item: cheap enough to redo
        p, a = R.sample_prime(bytes.fromhex(u["seed"]), u["sid"], i, u["max_attempts"])
        assert (hex(p), a) == (u["primes"][i], u["attempts"][i])
    k = g["keygen"]
    seed = bytes.fromhex(k["seed"])
    for i in range(k["nkeys"]):
        p, q = int(k["p"][i], 16), int(k["q"][i], 16)
        assert p * q == int(k["N"][i], 16) and p.bit_length() == q.bit_length() == 1024
    n = g["ntilde"]
    for i in range(n["count"]):
        Nt, h1, h2, xhi, xhi_inv, xi, phi = (int(n[f][i], 16) for f in ("Nt", "h1", "h2", "xhi", "xhi_inv", "xi", "phi"))
        assert xi * (phi - xhi_inv) % phi == 1 and xhi == phi - xi and h2 == pow(h1, xi, Nt) and pow(h2, phi - xhi_inv, Nt) == h1
        assert xi == R.draw_xi(seed, n["counter"] | (5 << 56), i, phi)
    c = g["isprime"]
    small = [(int(v, 16), e) for v, e in zip(c["values"], c["expect"]) if int(v, 16) < 1 << 64]
    assert small and all(R.is_prime(v) == bool(e) for v, e in small)


def test_key_material_entry_points_reject_bad_arguments_without_gpu():
    """follows test_version_and_argument_errors_without_gpu: NULL pointers, bits != 1024 and rounds out of range are MPE_E_ARG
    before any HIP call (no context can exist without a GPU, so every call below also lacks one)"""
    import ctypes as C
    from multi_party_ecdsa_amd import _native as N
    seed = bytes(32)
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    L = N.lib
    assert b"0.7" in L.mpe_version()
    for rounds in (0, 17, -1, 8):
        assert L.mpe_is_probable_prime(None, 1, p, rounds, p, None) == N.MPE_E_ARG
    assert L.mpe_is_probable_prime(None, 1, None, 8, None, None) == N.MPE_E_ARG
    for bits in (512, 1023, 2048, 0, 1024):
        assert L.mpe_sample_prime(None, 1, seed, 0, bits, 0, p, p, p, None) == N.MPE_E_ARG
    assert L.mpe_sample_prime(None, 1, None, 0, 1024, 0, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_paillier_keygen(None, 1, seed, 0, 0, p, p, p, p, None) == N.MPE_E_ARG
    assert L.mpe_paillier_keygen(None, 1, None, 1 << 56, 0, None, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_ntilde_generate(None, 1, seed, 0, 0, p, p, p, p, p, p, None) == N.MPE_E_ARG
    assert L.mpe_ntilde_generate(None, 1, None, 0, -1, None, None, None, None, None, None, None) == N.MPE_E_ARG
