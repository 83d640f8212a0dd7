"""The pair ladder's operation SEQUENCES (mpe_pairexp.h): runs of in-place squarings, window multiplications of either base, the
hand-over between them — chosen by exponent shape, not by size, and compared word for word with Python's pow.

The ladder is reached through the calls of the C-ABI that end in it, on contexts pinned to each lane layout (option no_wide: 18 limbs
per lane; the default context: 5 limbs at these batch sizes; xwide_div = 0: 9 limbs), each with the sliding windows on and off:

  pub.mul        c^k mod N^2                  2048-bit pairs, ONE base, a free exponent of 64 or 8 words on fixed windows
  pub.encrypt    r^N (1 + m N) mod N^2        2048-bit pairs, one base, the exponent IS the modulus: the sliding schedule; exponent shapes
                                              through "keys" no RSA modulus looks like (a lone top bit, all ones, alternating windows)
  message_b      c_a^b r^N (1 + t N)          2048-bit pairs, TWO bases, exp2_words = 8 (the range proofs handed in are blank: ok = 0, the
                                              ciphertext is written all the same, include/mpecdsa_hip.h)
  sk.encrypt     the holder's r^N             1024-bit pairs: a half-mode ladder modulo p | q, then a^p modulo p^2 | q^2
  sk.decrypt     c^(p-1) mod p^2 | q^2        1024-bit pairs, one base

Batches of 1, 15, 17 and 33 items over two keys: the launch is ordered by key, so at 17 and 33 one wave straddles the key boundary and
keeps the fixed windows while its neighbours slide.  What no call of the C-ABI reaches is not covered here: a second base on the 1024-bit
and half-mode ladders (the library has no such caller), a free FIRST exponent beside a second base, and the exponents 1 and 2 on the
1024-bit ladders (their exponents belong to the key)."""
import pytest
import torch

import fixtures as F

pytestmark = pytest.mark.gpu

BATCHES = [1, 15, 17, 33]
CONTEXTS = [(lay, opts, ns) for lay, opts in (("18limbs", {"no_wide": 1}), ("default", {}), ("9limbs", {"xwide_div": 0})) for ns in (0, 1)]
TOP = 1 << 2047


def alternating(bits, w):
    """`bits` bits of alternating full and empty w-bit windows, the top window full"""
    v = 0
    for lo in range(bits - w, -1, -2 * w):
        v |= ((1 << w) - 1) << lo
    return v


# "keys" whose modulus is the exponent shape: a lone top bit (2 047 squarings, then the bit that makes it odd), all ones (a
# multiplication after every window), alternating empty and full windows
SHAPES = [TOP + 1, (1 << 2048) - 1, alternating(2048, 6) | 1, alternating(2048, 5) | TOP | 1]


def split(B):
    """two keys, the boundary inside a wave's 16 items"""
    return [0 if i < (B + 1) // 2 else 1 for i in range(B)]


def bases_mod_nn(r, N, i):
    return [0, 1, N - 1, N, N + 1, N * N - 1, r.below(N * N), r.bits(4096)][i % 8]


def bases_mod_n(r, N, i):
    """64-word operands (the randomness of an encryption): the fixed values that fit, then random ones"""
    top = N + 1 if N + 1 < (1 << 2048) else N - 2
    return [0, 1, N - 1, N, top, r.below(N), r.bits(2048), r.below(N)][i % 8]


def exponent(r, words, i):
    bits = 32 * words
    return [1, 2, 1 << (bits - 1), (1 << bits) - 1, alternating(bits, 6 if words >= 48 else 4), r.bits(bits), r.bits(bits) | (1 << (bits - 1))][i % 7]


_REF = {}


def reference(name, B, make):
    """computed once per (route, batch) and shared by the six contexts"""
    if (name, B) not in _REF:
        _REF[(name, B)] = make()
    return _REF[(name, B)]


@pytest.fixture(scope="module", params=CONTEXTS, ids=[f"{lay}-{'fixed' if ns else 'sliding'}" for lay, _, ns in CONTEXTS])
def ctx(request):
    from multi_party_ecdsa_amd import engine as E
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (the HIP path has no CPU fallback)")
    lay, opts, ns = request.param
    c = E.Context(0, options={**opts, **({"no_sliding": 1} if ns else {})})
    yield c
    c.close()


@pytest.mark.parametrize("B", BATCHES)
def test_one_base_free_exponent(ctx, keys, B):
    """c^k mod N^2 on fixed windows: exponents 1, 2, a lone top bit, all ones, alternating windows, random — 64 words (6-bit windows) and
    8 words (4-bit windows); bases 0, 1, N - 1, N (z0 >= N carries into z1), N + 1, N^2 - 1, random, unreduced"""
    from multi_party_ecdsa_amd import engine as E
    pub = E.PaillierKeys(ctx, N=[k.N for k in keys[:2]])
    kidx = split(B)
    for kw in (64, 8):
        def make():
            r = F.Rng(f"glue-mul-{B}-{kw}")
            bs = [bases_mod_nn(r, keys[k].N, i + B) for i, k in enumerate(kidx)]
            es = [exponent(r, kw, i // 8 + i + B) for i in range(B)]
            return bs, es, [pow(b, e, keys[k].N ** 2) for b, e, k in zip(bs, es, kidx)]
        bs, es, want = reference(f"mul{kw}", B, make)
        assert pub.mul(bs, es, kidx, k_words=kw) == want


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("pair", [(0, 1), (2, 3)])
def test_one_base_public_exponent_shapes(ctx, B, pair):
    """r^N (1 + m N) mod N^2 where N is the exponent shape: the sliding schedule (fixed windows on the no_sliding contexts and in the
    wave that straddles the two keys)"""
    from multi_party_ecdsa_amd import engine as E
    mods = [SHAPES[pair[0]], SHAPES[pair[1]]]
    pub = E.PaillierKeys(ctx, N=mods)
    kidx = split(B)

    def make():
        r = F.Rng(f"glue-enc-{B}-{pair}")
        rr = [bases_mod_n(r, mods[k], i + B) for i, k in enumerate(kidx)]
        m = [0 if i % 3 == 0 else r.below(mods[k]) for i, k in enumerate(kidx)]
        return rr, m, [(1 + mm * mods[k]) * pow(x, mods[k], mods[k] ** 2) % mods[k] ** 2 for mm, x, k in zip(m, rr, kidx)]
    rr, m, want = reference(f"enc{pair}", B, make)
    assert pub.encrypt(m, rr, kidx) == want


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shaped", [False, True])
def test_two_bases_short_second_exponent(ctx, keys, B, shaped):
    """MessageB's ciphertext c_a^b r^N (1 + t N) mod N^2 on one ladder: second exponents 0 (every window multiplies by the form of 1),
    all ones, 1, 2, random — under two real keys and under two exponent shapes"""
    from multi_party_ecdsa_amd import engine as E
    mods = [SHAPES[1], SHAPES[2]] if shaped else [k.N for k in keys[:2]]
    pub = E.PaillierKeys(ctx, N=mods)
    stm = E.Statements(ctx, [keys[4].Nt], [keys[4].h1], [keys[4].h2], wb=0)
    kidx = split(B)

    def make():
        r = F.Rng(f"glue-mb-{B}-{shaped}")
        ca = [bases_mod_nn(r, mods[k], i + B) for i, k in enumerate(kidx)]
        rr = [bases_mod_n(r, mods[k], i // 8 + i) for i, k in enumerate(kidx)]
        b = [[0, (1 << 256) - 1, 1, 2, r.bits(256), alternating(256, 4)][(i + B) % 6] for i in range(B)]
        t = [r.below(mods[k]) for k in kidx]
        want = [pow(c, e, mods[k] ** 2) * pow(x, mods[k], mods[k] ** 2) * (1 + tt * mods[k]) % mods[k] ** 2
                for c, e, x, tt, k in zip(ca, b, rr, t, kidx)]
        return ca, rr, b, t, want
    ca, rr, b, t, want = reference(f"mb{shaped}", B, make)
    blank = {f: torch.zeros((B, w), dtype=torch.int32, device=ctx.device) for f, w in E.ALICE_PROOF_WORDS.items()}
    one = E.dev(ctx, [1] * B, 8)
    out = E.mta_message_b(ctx, pub, stm, E.dev(ctx, b, 8), E.dev(ctx, ca, 128), blank, E.dev(ctx, rr, 64), E.dev(ctx, t, 64), one, one,
                          torch.tensor(kidx, dtype=torch.int32, device=ctx.device))
    ctx.sync()
    assert E.host(out["c"]) == want
    stm.close()


@pytest.mark.parametrize("B", BATCHES)
def test_key_holder_halves(ctx, keys, B):
    """the 1024-bit ladders: the holder's r^N (half mode modulo p | q, then a^p modulo p^2 | q^2) and the decryption's c^(p-1)"""
    from multi_party_ecdsa_amd import engine as E
    ks = keys[:2]
    sk = E.PaillierKeys(ctx, p=[k.p for k in ks], q=[k.q for k in ks])
    kidx = split(B)

    def make():
        r = F.Rng(f"glue-sk-{B}")
        rr = [[0, 1, ks[k].N - 1, ks[k].N, ks[k].N + 1, ks[k].p * 3, r.below(ks[k].N), r.bits(2048)][(i + B) % 8] for i, k in enumerate(kidx)]
        m = [r.below(ks[k].N) for k in kidx]
        c = [(1 + mm * ks[k].N) * pow(x, ks[k].N, ks[k].N ** 2) % ks[k].N ** 2 for mm, x, k in zip(m, rr, kidx)]
        # ciphertexts to open: valid ones and the corners 1, 1 + N, N^2 - 1 (plaintexts 0, 1, and what the definition gives)
        cs, ms = [], []
        for i, k in enumerate(kidx):
            N, p, q = ks[k].N, ks[k].p, ks[k].q
            lam = (p - 1) * (q - 1)
            cc = [1, 1 + N, N * N - 1, (1 + m[i] * N) * pow(r.coprime_below(N), N, N * N) % (N * N)][(i + B) % 4]
            cs.append(cc)
            ms.append((pow(cc, lam, N * N) - 1) // N * pow(lam, -1, N) % N)
        return rr, m, c, cs, ms
    rr, m, c, cs, ms = reference("sk", B, make)
    assert sk.encrypt(m, rr, kidx) == c
    assert sk.decrypt(cs, kidx) == ms
