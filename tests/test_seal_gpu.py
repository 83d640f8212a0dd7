"""GPU tests of the sealed rows (`mpe_seal`, `mpe_unseal`, `mpe_poly1305`; csrc/mpe_seal.h): the kernels' rows equal
tests/pyref_seal.py — which tests/test_seal_cpu.py pins to OpenSSL — byte for byte, at 70 rows (one full workgroup and a partial
second one, so row indices 0 and >= 64 both appear in nonces) and at payload lengths on both sides of the Poly1305 and ChaCha20
block sizes; opening refuses every tampered region, another key and another kind with 841 and an all-zero row, for that row only."""
import numpy as np
import pytest
import torch

import pyref_seal as PS
import seal_cases as SC

pytestmark = pytest.mark.gpu

ROWS = 70


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def wk(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    k = E.WrapKey(gpu_ctx, SC.KEY)
    yield k
    k.close()


@pytest.fixture(scope="module")
def wk_other(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    k = E.WrapKey(gpu_ctx, SC.OTHER_KEY)
    yield k
    k.close()


@pytest.mark.parametrize("w", SC.LENGTHS)
def test_sealed_rows_equal_the_restatement_and_round_trip(gpu_ctx, wk, w):
    from multi_party_ecdsa_amd import engine as E
    plain = SC.payloads(w, ROWS)
    sealed = E.seal(gpu_ctx, wk, PS.KIND_USER, _dev(gpu_ctx, plain), nonce_hi=SC.NONCE_HI)
    got = _u32(sealed)
    assert got.shape == (ROWS, w + PS.EXTRA)
    want = np.array([PS.seal_row(SC.KEY, PS.KIND_USER, g, SC.NONCE_HI, plain[g]) for g in range(ROWS)], dtype=np.uint32)
    assert np.array_equal(got, want)
    assert list(got[:, 3]) == list(range(ROWS))                           # the row index is the nonce's first word: 0 and >= 64
    back, status = E.unseal(gpu_ctx, wk, PS.KIND_USER, sealed)
    assert not status.cpu().numpy().any() and np.array_equal(_u32(back), plain)


def test_every_tampered_region_another_key_and_another_kind_are_refused_row_by_row(gpu_ctx, wk, wk_other):
    from multi_party_ecdsa_amd import engine as E
    w = 72
    plain = SC.payloads(w, ROWS)
    sealed = _u32(E.seal(gpu_ctx, wk, PS.KIND_USER, _dev(gpu_ctx, plain), nonce_hi=SC.NONCE_HI)).copy()
    # one flipped bit per region, in rows on both sides of the workgroup boundary
    flips = {3: (0, 0), 64: (1, 4), 5: (2, 0), 66: (3, 9), 7: (4, 31), 68: (5, 17), 9: (PS.HEAD, 0), 69: (PS.HEAD + w - 1, 31),
             11: (PS.HEAD + w, 0), 63: (PS.HEAD + w + 3, 31)}                 # row -> (word, bit): magic, kind, length, nonce x3, ciphertext x2, tag x2
    for row, (word, bit) in flips.items():
        sealed[row, word] ^= np.uint32(1 << bit)
    other_key = _u32(E.seal(gpu_ctx, wk_other, PS.KIND_USER, _dev(gpu_ctx, plain[[13, 65]]), nonce_hi=SC.NONCE_HI))
    sealed[13], sealed[65] = other_key[0], other_key[1]                  # (sealed as rows 0, 1 of their call: authentic under the other key)
    other_kind = _u32(E.seal(gpu_ctx, wk, PS.KIND_USER + 1, _dev(gpu_ctx, plain[[15, 67]]), nonce_hi=SC.NONCE_HI))
    sealed[15], sealed[67] = other_kind[0], other_kind[1]
    bad = sorted(list(flips) + [13, 65, 15, 67])
    back, status = E.unseal(gpu_ctx, wk, PS.KIND_USER, _dev(gpu_ctx, sealed))
    back, status = _u32(back), status.cpu().numpy()
    for g in range(ROWS):
        code, words = PS.unseal_row(SC.KEY, PS.KIND_USER, w, sealed[g])
        assert code == (PS.REFUSED if g in bad else 0), g
        assert status[g] == code and [int(x) for x in back[g]] == words, g
    assert not back[bad].any() and np.array_equal(np.delete(back, bad, axis=0), np.delete(plain, bad, axis=0))
    # the rows of the other key open under that key, the rows of the other kind under that kind
    b2, s2 = E.unseal(gpu_ctx, wk_other, PS.KIND_USER, _dev(gpu_ctx, other_key))
    assert not s2.cpu().numpy().any() and np.array_equal(_u32(b2), plain[[13, 65]])
    b3, s3 = E.unseal(gpu_ctx, wk, PS.KIND_USER + 1, _dev(gpu_ctx, other_kind))
    assert not s3.cpu().numpy().any() and np.array_equal(_u32(b3), plain[[15, 67]])


def test_the_generic_pair_refuses_the_library_kinds(gpu_ctx, wk):
    from multi_party_ecdsa_amd import _native as N
    from multi_party_ecdsa_amd import engine as E
    plain = _dev(gpu_ctx, SC.payloads(72, 2))
    for kind in (0, PS.KIND_PRESIG, PS.KIND_KEYSHARE, 15):
        with pytest.raises(N.MpeError, match="rc=-1"):
            E.seal(gpu_ctx, wk, kind, plain, nonce_hi=1)
        with pytest.raises(N.MpeError, match="rc=-1"):
            E.unseal(gpu_ctx, wk, kind, torch.zeros((2, 82), dtype=torch.int32, device=gpu_ctx.device))
    # a key share sealed by the library does not open through the generic call under a caller's kind either
    ks = E.keyshare_seal(gpu_ctx, wk, plain[:, :8], plain[:, 8:40], plain[:, 40:72], nonce_hi=2)
    assert [int(x) for x in _u32(ks)[1]] == PS.seal_row(SC.KEY, PS.KIND_KEYSHARE, 1, 2, _u32(plain)[1])
    back, status = E.unseal(gpu_ctx, wk, PS.KIND_USER, ks)
    assert list(status.cpu().numpy()) == [PS.REFUSED] * 2 and not _u32(back).any()
    with pytest.raises(N.MpeError, match="rc=-1"):                       # 1 <= words <= 4096
        E.seal(gpu_ctx, wk, PS.KIND_USER, torch.zeros((1, 4097), dtype=torch.int32, device=gpu_ctx.device), nonce_hi=3)


def test_poly1305_reduction_corners_and_partial_blocks(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    keys = np.stack([SC.key_words(key) for _, key, _, _ in SC.POLY_CORNERS])
    msgs = np.stack([np.frombuffer(msg, dtype=np.uint8) for _, _, msg, _ in SC.POLY_CORNERS])
    tags = _u32(E.poly1305(gpu_ctx, _dev(gpu_ctx, keys), torch.from_numpy(msgs.copy()).to(gpu_ctx.device)))
    for g, (name, _, _, want) in enumerate(SC.POLY_CORNERS):
        assert tags[g].tobytes() == want, name
    rg = np.random.default_rng(9)
    for nbytes in (1, 15, 17, 33):                                        # 66 rows of random keys, a partial last block
        keys = rg.integers(0, 1 << 32, size=(66, 8), dtype=np.uint64).astype(np.uint32)
        msgs = rg.integers(0, 256, size=(66, nbytes), dtype=np.uint8)
        tags = _u32(E.poly1305(gpu_ctx, _dev(gpu_ctx, keys), torch.from_numpy(msgs).to(gpu_ctx.device)))
        for g in (0, 1, 63, 64, 65):
            assert tags[g].tobytes() == PS.poly1305(keys[g].tobytes(), msgs[g].tobytes()), (nbytes, g)
