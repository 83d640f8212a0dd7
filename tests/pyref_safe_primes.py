"""Pure-Python restatement of the device's SAFE-prime search (multi_party_ecdsa_amd/csrc/mpe_primes.h, "safe primes"):
kzen-paillier's `sample_safe_prime(bits)` = loop { q = sample_prime(bits); if is_prime((q - 1) / 2) return q } on this library's
statement of sample_prime (tests/pyref_primes.py): the result of an item is the candidate c of the LOWEST attempt for which c and
(c - 1) / 2 are both prime; `Paillier::keypair_safe_primes()` and `generate_h1_h2_N_tilde()` with safe primes on top of it.

A safe prime costs ~380 000 attempts, so the search cannot call pyref_primes.candidate per attempt.  The keystream is computed in
numpy for a block of attempts at once (checked against the oracle's ChaCha20 by tests/test_safe_primes_cpu.py), and three EXACT
filters discard attempts before the restatement's own test sees them — none of them can discard a prime:
  * bit 1 of c clear: (c - 1) / 2 is even;
  * a table prime below FILTER_BOUND divides c or (c - 1) / 2 (residues of 64-bit multiply-add sums, in numpy);
  * 2^(n - 1) != 1 (mod n) for n = c or n = (c - 1) / 2 (Fermat: every prime passes).
What is left is decided by pyref_primes.is_prime, winners are confirmed by GMP, and a winner is rebuilt with pyref_primes.candidate."""
import functools
import math

import numpy as np

import orc
import pyref_primes as R

DEFAULT_MAX_ATTEMPTS = 1 << 24
CHUNK = 1 << 14                          # attempts per numpy block
FILTER_BOUND = 1000                      # table primes below this are tested in numpy


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def chacha20_blocks(seed, sid, item, blocks):
    """keystream words [len(blocks)][16] of the sampler's streams: key = seed, state[12] = block, [13] = item, [14..15] = sid"""
    blocks = np.asarray(blocks, dtype=np.uint32)
    n = blocks.shape[0]
    init = np.empty((16, n), dtype=np.uint32)
    init[0:4] = np.array([0x61707865, 0x3320646e, 0x79622d32, 0x6b206574], dtype=np.uint32)[:, None]
    init[4:12] = np.frombuffer(bytes(seed), dtype="<u4").astype(np.uint32)[:, None]
    init[12] = blocks
    init[13] = np.uint32(item)
    init[14] = np.uint32(sid & 0xffffffff)
    init[15] = np.uint32(sid >> 32)
    x = init.copy()
    col = (np.array([0, 1, 2, 3]), np.array([4, 5, 6, 7]), np.array([8, 9, 10, 11]), np.array([12, 13, 14, 15]))
    dia = (np.array([0, 1, 2, 3]), np.array([5, 6, 7, 4]), np.array([10, 11, 8, 9]), np.array([15, 12, 13, 14]))
    with np.errstate(over="ignore"):
        for _ in range(10):
            for ia, ib, ic, id_ in (col, dia):
                a, b, c, d = x[ia], x[ib], x[ic], x[id_]
                a += b; d = _rotl(d ^ a, 16)
                c += d; b = _rotl(b ^ c, 12)
                a += b; d = _rotl(d ^ a, 8)
                c += d; b = _rotl(b ^ c, 7)
                x[ia], x[ib], x[ic], x[id_] = a, b, c, d
        x += init
    return np.ascontiguousarray(x.T)


def _half_words(ks):
    """the 16 words (least significant first) of the 64 keystream bytes read as a big-endian integer"""
    return ks[:, ::-1].byteswap()


def _filter_tables():
    primes = [p for p in R.SMALL_PRIMES if p < FILTER_BOUND]
    groups, cur, prod = [], [], 1
    for p in primes:
        if prod * p >= 1 << 26:
            groups.append((prod, cur)); cur, prod = [], 1
        cur.append(p); prod *= p
    groups.append((prod, cur))
    return [(np.uint64(M), np.array([pow(2, 32 * i, M) for i in range(32)], dtype=np.uint64), ps) for M, ps in groups]


_TABLES = _filter_tables()


def _small_factor_mask(w, joint):
    """True where a table prime below FILTER_BOUND divides c (or, joint, c or (c - 1) / 2: c = 1 mod l)"""
    dead = np.zeros(w.shape[0], dtype=bool)
    w64 = w.astype(np.uint64)
    for M, pw, ps in _TABLES:
        r = (w64 * pw[None, :]).sum(axis=1, dtype=np.uint64) % M          # < 32 * 2^32 * 2^26 = 2^63
        for p in ps:
            t = r % np.uint64(p)
            dead |= (t == 0) | (t == 1) if joint else t == 0
    return dead


def candidates(seed, sid, item, a0, n, joint):
    """-> (attempts, words [.][32]) of the attempts in [a0, a0 + n) that the numpy filters leave"""
    att = np.arange(a0, a0 + n, dtype=np.int64)
    lo = _half_words(chacha20_blocks(seed, sid, item, 2 * att + 1))
    lo[:, 0] |= np.uint32(1)
    if joint:
        keep = (lo[:, 0] & np.uint32(2)) != 0
        att, lo = att[keep], lo[keep]
    hi = _half_words(chacha20_blocks(seed, sid, item, 2 * att))
    hi[:, 15] |= np.uint32(0x80000000)
    w = np.ascontiguousarray(np.concatenate([lo, hi], axis=1))
    keep = ~_small_factor_mask(w, joint)
    return att[keep], np.ascontiguousarray(w[keep])


def _int(row):
    return int.from_bytes(row.astype("<u4").tobytes(), "little")


def _fermat2(w):
    """2^(n - 1) == 1 (mod n) for every odd row n (GMP, through the oracle's batched modexp)"""
    if w.shape[0] == 0:
        return np.zeros(0, dtype=bool)
    base = np.zeros_like(w); base[:, 0] = 2
    e = w.copy(); e[:, 0] &= np.uint32(0xfffffffe)
    r = orc.modexp(w, base, e, np.arange(w.shape[0]))
    return (r[:, 0] == 1) & ~r[:, 1:].any(axis=1)


def prime_attempts(seed, sid, item, a0, a1):
    """the attempts in [a0, a1) whose candidate is prime (plain sample_prime's acceptances)"""
    out = []
    for lo in range(a0, a1, CHUNK):
        att, w = candidates(seed, sid, item, lo, min(CHUNK, a1 - lo), joint=False)
        ok = _fermat2(w)
        out += [int(a) for a, row in zip(att[ok], w[ok]) if R.is_prime(_int(row))]
    return out


@functools.lru_cache(maxsize=None)
def sample_safe_prime(seed, sid, item, max_attempts=DEFAULT_MAX_ATTEMPTS):
    """(safe prime, attempt) of the lowest attempt whose candidate c and (c - 1) / 2 are both prime, or (0, -1)"""
    for lo in range(0, max_attempts, CHUNK):
        att, w = candidates(seed, sid, item, lo, min(CHUNK, max_attempts - lo), joint=True)
        for a, row in zip(att, w):
            c = _int(row)
            h = c >> 1
            if math.gcd(h, R._PRIMORIAL) != 1 or math.gcd(c, R._PRIMORIAL) != 1 or pow(2, h - 1, h) != 1 or pow(2, c - 1, c) != 1:
                continue
            if R.is_prime(c) and R.is_prime(h):
                assert c == R.candidate(seed, sid, item, int(a)) and R.gmp_confirms(c) and R.gmp_confirms(h)
                return c, int(a)
    return 0, -1


def sample_safe_primes(seed, sid, batch, max_attempts=DEFAULT_MAX_ATTEMPTS):
    """-> (primes, attempts, failures)"""
    r = [sample_safe_prime(bytes(seed), sid, g, max_attempts) for g in range(batch)]
    return [p for p, _ in r], [a for _, a in r], sum(1 for _, a in r if a < 0)


def paillier_keygen(seed, counter, nkeys, max_attempts=DEFAULT_MAX_ATTEMPTS):
    """`Paillier::keypair_safe_primes()`: p, q from fields 0, 1 through the safe search; N = p q.  -> (p, q, N, failures)"""
    p, _, _ = sample_safe_primes(seed, R._field(counter, 0), nkeys, max_attempts)
    q, _, _ = sample_safe_primes(seed, R._field(counter, 1), nkeys, max_attempts)
    bad = [a == 0 or b == 0 for a, b in zip(p, q)]
    p = [0 if z else v for v, z in zip(p, bad)]
    q = [0 if z else v for v, z in zip(q, bad)]
    return p, q, [a * b for a, b in zip(p, q)], sum(bad)


def ntilde_generate(seed, counter, count, max_attempts=DEFAULT_MAX_ATTEMPTS):
    """generate_h1_h2_N_tilde with p~, q~ (fields 2, 3) safe primes; everything behind them is pyref_primes.ntilde_generate's body, run
    with its prime search swapped for the safe one (the body takes no search argument)"""
    seed = bytes(seed)
    plain = R.sample_primes
    R.sample_primes = lambda s, sid, n, cap: sample_safe_primes(s, sid, n, cap)
    try:
        return R.ntilde_generate(seed, counter, count, max_attempts)
    finally:
        R.sample_primes = plain
