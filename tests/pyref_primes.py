"""Pure-Python restatement of the device's key-material layer (multi_party_ecdsa_amd/csrc/mpe_primes.h): kzen-paillier's
sample_prime over the sampler's ChaCha20 streams, `Paillier::keypair()` and `generate_h1_h2_N_tilde()` (party_i.rs:137-177).

Keystream bytes come from the oracle (orc_chacha20_block / orc_sample_below expand the same seed); the arithmetic is on Python
integers.  Primality is decided by trial division plus Miller-Rabin with 20 bases from random.Random(0) — NOT the device's fixed
bases 2, 3, 5, ... — and every accepted prime is cross-checked with GMP (orc_nextprime(p - 1) == p), so agreement with the
device does not rest on one shared test."""
import functools
import math
import random

import numpy as np

import orc

SIEVE_BOUND = 6370
DEFAULT_MAX_ATTEMPTS = 16384
SAMPLER_MAX_ATTEMPTS = 128                # the sampler's rejection bound (option sampler_max_attempts)
SMALL_PRIMES = [p for p in range(3, SIEVE_BOUND, 2) if all(p % d for d in range(3, int(p ** 0.5) + 1, 2))]
_PRIMORIAL = math.prod(SMALL_PRIMES)
_rng = random.Random(0)
MR_BASES = [_rng.randrange(2, 1 << 64) for _ in range(20)]

orc.lib.orc_nextprime.restype = None


def keystream(seed, sid, item, first_byte, nbytes):
    """bytes [first_byte, first_byte + nbytes) of item's stream: ChaCha20, key = seed, state[12] = block, [13] = item, [14..15] = sid"""
    b0, b1 = first_byte // 64, (first_byte + nbytes - 1) // 64
    buf = b"".join(orc.chacha20_block(seed, b, item, sid & 0xffffffff, sid >> 32) for b in range(b0, b1 + 1))
    return buf[first_byte - 64 * b0: first_byte - 64 * b0 + nbytes]


def candidate(seed, sid, item, attempt, bits=1024):
    """attempt `attempt` of sample_prime: BigInt::sample(bits) of its own bytes, bit 0 and bit bits-1 set"""
    nb = bits // 8
    return int.from_bytes(keystream(seed, sid, item, nb * attempt, nb), "big") | 1 | (1 << (bits - 1))


def _strong_probable_prime(n, a):
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    x = pow(a, d, n)
    if x in (1, n - 1):
        return True
    for _ in range(s - 1):
        x = x * x % n
        if x == n - 1:
            return True
    return False


def is_prime(n):
    if n < 2:
        return False
    if n % 2 == 0:
        return n == 2
    if n < SIEVE_BOUND * SIEVE_BOUND:
        return all(n % p for p in SMALL_PRIMES if p * p <= n)
    if math.gcd(n, _PRIMORIAL) != 1:
        return False
    return all(_strong_probable_prime(n, a % n) for a in MR_BASES if a % n > 1)


def gmp_confirms(p):
    """mpz_nextprime(p - 1) == p (GMP's own test: a second opinion on an accepted prime)"""
    k32 = max(1, (p.bit_length() + 31) // 32)
    w = lambda v: np.array([(v >> (32 * j)) & 0xffffffff for j in range(k32)], dtype=np.uint32)
    out = np.zeros(k32, dtype=np.uint32)
    orc.lib.orc_nextprime(k32, orc._p(w(p - 1)), orc._p(out))
    return sum(int(x) << (32 * j) for j, x in enumerate(out)) == p


@functools.lru_cache(maxsize=None)
def sample_prime(seed, sid, item, max_attempts=DEFAULT_MAX_ATTEMPTS):
    """(prime, attempt) of the lowest passing attempt, or (0, -1)"""
    for a in range(max_attempts):
        c = candidate(seed, sid, item, a)
        if is_prime(c):
            assert gmp_confirms(c)
            return c, a
    return 0, -1


def sample_primes(seed, sid, batch, max_attempts=DEFAULT_MAX_ATTEMPTS):
    """-> (primes, attempts, failures)"""
    r = [sample_prime(bytes(seed), sid, g, max_attempts) for g in range(batch)]
    return [p for p, _ in r], [a for _, a in r], sum(1 for _, a in r if a < 0)


def _field(counter, f):
    return counter | (f << 56)


def paillier_keygen(seed, counter, nkeys, max_attempts=DEFAULT_MAX_ATTEMPTS):
    """`Paillier::keypair()`: p, q from fields 0, 1; N = p q.  -> (p, q, N, failures); a failed key is all zero"""
    p, _, _ = sample_primes(seed, _field(counter, 0), nkeys, max_attempts)
    q, _, _ = sample_primes(seed, _field(counter, 1), nkeys, max_attempts)
    bad = [a == 0 or b == 0 for a, b in zip(p, q)]
    p = [0 if z else v for v, z in zip(p, bad)]
    q = [0 if z else v for v, z in zip(q, bad)]
    return p, q, [a * b for a, b in zip(p, q)], sum(bad)


def _words(vals, k32):
    return np.array([[(v >> (32 * j)) & 0xffffffff for j in range(k32)] for v in vals], dtype=np.uint32)


def draw_xi(seed, sid, item, phi):
    """sample_below(phi) with fresh bytes per attempt until gcd(xi, phi) == 1; 0 when SAMPLER_MAX_ATTEMPTS draws were refused"""
    bits = phi.bit_length()
    nb = (bits + 7) // 8
    for a in range(SAMPLER_MAX_ATTEMPTS):
        x = int.from_bytes(keystream(seed, sid, item, nb * a, nb), "big") >> (8 * nb - bits)
        if x < phi and math.gcd(x, phi) == 1:
            return x
    return 0


def ntilde_generate(seed, counter, count, max_attempts=DEFAULT_MAX_ATTEMPTS):
    """party_i.rs:137-156: dict of lists Nt, h1, h2, xhi, xhi_inv (+ xi, phi for the tests' own checks) and `fail`"""
    seed = bytes(seed)
    pt, _, _ = sample_primes(seed, _field(counter, 2), count, max_attempts)
    qt, _, _ = sample_primes(seed, _field(counter, 3), count, max_attempts)
    out = dict(Nt=[], h1=[], h2=[], xhi=[], xhi_inv=[], xi=[], phi=[], fail=0)
    bounds = [a * b if a and b else 3 for a, b in zip(pt, qt)]
    h1s, _ = orc.sample_below(count, seed, _field(counter, 4), _words(bounds, 64), 64)
    for i, (a, b) in enumerate(zip(pt, qt)):
        ok = a != 0 and b != 0
        nt, phi = a * b, (a - 1) * (b - 1)
        h1 = sum(int(w) << (32 * j) for j, w in enumerate(h1s[i]))
        xi = draw_xi(seed, _field(counter, 5), i, phi) if ok else 0
        ok = ok and xi != 0
        if not ok:
            for f in ("Nt", "h1", "h2", "xhi", "xhi_inv", "xi", "phi"):
                out[f].append(0)
            out["fail"] += 1
            continue
        out["Nt"].append(nt); out["h1"].append(h1); out["h2"].append(pow(h1, xi, nt))
        out["xhi"].append(phi - xi); out["xhi_inv"].append(phi - pow(xi, -1, phi))
        out["xi"].append(xi); out["phi"].append(phi)
    return out
