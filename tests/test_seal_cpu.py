"""CPU tests of the sealed rows.  (1) tests/pyref_seal.py — RFC 8439 AEAD in plain Python plus the sealed-row layout — is pinned to
OpenSSL's EVP_chacha20_poly1305 (the libcrypto 1.1.1 tests/ossl.py links, reached through ctypes).  (2) The device code itself,
csrc/mpe_seal.h compiled for the host under MPE_SEAL_HOST (tools/model/seal_host.cpp), is driven through the same cases and the
Poly1305 reduction corners.  No GPU involved: the same header text is what hipcc compiles for gfx950."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyref_seal as PS
import seal_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUNSCREEN = b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, sunscreen would be it."
SUN_KEY = bytes(range(0x80, 0xA0))
SUN_NONCE = bytes.fromhex("070000004041424344454647")
SUN_AAD = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
SUN_TAG = bytes.fromhex("1ae10b594f09e26a7e902ecbd0600691")


@pytest.fixture(scope="module")
def crypto():
    import ossl                                              # loads oracle/libmpe_ossl.so, and with it the libcrypto it links
    assert "1.1.1" in ossl.version()
    lib = C.CDLL("libcrypto.so.1.1")
    lib.EVP_CIPHER_CTX_new.restype = C.c_void_p
    lib.EVP_chacha20_poly1305.restype = C.c_void_p
    lib.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
    lib.EVP_EncryptInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
    lib.EVP_CIPHER_CTX_ctrl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.EVP_EncryptUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    lib.EVP_EncryptFinal_ex.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    return lib


def ossl_aead(lib, key, nonce, aad, pt):
    """EVP_chacha20_poly1305 -> (ciphertext, tag)"""
    EVP_CTRL_AEAD_SET_IVLEN, EVP_CTRL_AEAD_GET_TAG = 0x9, 0x10
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        n = C.c_int(0)
        assert lib.EVP_EncryptInit_ex(ctx, lib.EVP_chacha20_poly1305(), None, None, None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_SET_IVLEN, 12, None) == 1
        assert lib.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
        assert lib.EVP_EncryptUpdate(ctx, None, C.byref(n), aad, len(aad)) == 1
        out = C.create_string_buffer(len(pt) + 16)
        assert lib.EVP_EncryptUpdate(ctx, out, C.byref(n), pt, len(pt)) == 1
        got = n.value
        assert lib.EVP_EncryptFinal_ex(ctx, C.cast(C.byref(out, got), C.c_char_p), C.byref(n)) == 1
        assert got + n.value == len(pt)
        tag = C.create_string_buffer(16)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_GET_TAG, 16, tag) == 1
        return out.raw[:len(pt)], tag.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


@pytest.fixture(scope="module")
def host():
    out = os.path.join(ROOT, "build", "libseal_host.so")
    src = os.path.join(ROOT, "tools", "model", "seal_host.cpp")
    inc = os.path.join(ROOT, "multi_party_ecdsa_amd", "csrc")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [src, os.path.join(inc, "mpe_seal.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMPE_SEAL_HOST", "-I", inc, src, "-o", out])
    lib = C.CDLL(out)
    lib.sealh_poly1305.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
    lib.sealh_poly1305.restype = None
    lib.sealh_seal_row.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_void_p]
    lib.sealh_open_row.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_seal(lib, key, kind, row, nonce_hi, words):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros(len(words) + PS.EXTRA, dtype=np.uint32)
    kw = SC.key_words(key)
    assert lib.sealh_seal_row(_p(kw), kind, row, nonce_hi & 0xFFFFFFFF, nonce_hi >> 32, len(words), _p(words), _p(out)) == 0
    return out


def host_open(lib, key, kind, w, sealed):
    sealed = np.ascontiguousarray(sealed, dtype=np.uint32)
    plain = np.full(w, 0xA5A5A5A5, dtype=np.uint32)
    kw = SC.key_words(key)
    return lib.sealh_open_row(_p(kw), kind, w, _p(sealed), _p(plain)), plain


def host_poly(lib, key, msg):
    kw = SC.key_words(key)
    tag = np.zeros(4, dtype=np.uint32)
    lib.sealh_poly1305(_p(kw), msg, len(msg), _p(tag))
    return tag.tobytes()


# ---- 1. the restatement against OpenSSL ------------------------------------------------------------------------------------
def test_pyref_sunscreen_vector(crypto):
    ct, tag = PS.aead_encrypt(SUN_KEY, SUN_NONCE, SUN_AAD, SUNSCREEN)
    assert tag == SUN_TAG and ct[:16] == bytes.fromhex("d31a8d34648e60db7b86afbc53ef7ec2")
    assert ossl_aead(crypto, SUN_KEY, SUN_NONCE, SUN_AAD, SUNSCREEN) == (ct, tag)
    assert PS.aead_decrypt(SUN_KEY, SUN_NONCE, SUN_AAD, ct, tag) == SUNSCREEN
    assert PS.aead_decrypt(SUN_KEY, SUN_NONCE, SUN_AAD, ct, bytes([tag[0] ^ 1]) + tag[1:]) is None


@pytest.mark.parametrize("w", SC.LENGTHS)
def test_pyref_rows_equal_openssl(crypto, w):
    for row, words in zip((0, 65, 69), SC.payloads(w, 3)):
        sealed = PS.seal_row(SC.KEY, PS.KIND_USER, row, SC.NONCE_HI, words)
        assert len(sealed) == w + PS.EXTRA and sealed[:6] == [PS.MAGIC, PS.KIND_USER, w, row, SC.NONCE_HI & 0xFFFFFFFF, SC.NONCE_HI >> 32]
        b = np.array(sealed, dtype="<u4").tobytes()
        ct, tag = ossl_aead(crypto, SC.KEY, b[12:24], b[:12], words.astype("<u4").tobytes())
        assert b[24:24 + 4 * w] == ct and b[24 + 4 * w:] == tag
        assert PS.unseal_row(SC.KEY, PS.KIND_USER, w, sealed) == (0, [int(x) for x in words])


def test_pyref_poly1305_corners():
    for name, key, msg, want in SC.POLY_CORNERS:
        assert PS.poly1305(key, msg) == want, name


# ---- 2. the device code, compiled for the host --------------------------------------------------------------------------------
def test_host_sunscreen_tag(host):
    """the RFC's vector through the Poly1305 core: its one-time key and MAC input are the restatement's"""
    otk = PS.chacha20_block(SUN_KEY, 0, SUN_NONCE)[:32]
    ct, tag = PS.aead_encrypt(SUN_KEY, SUN_NONCE, SUN_AAD, SUNSCREEN)
    mac = PS._pad16(SUN_AAD) + PS._pad16(ct) + (12).to_bytes(8, "little") + len(ct).to_bytes(8, "little")
    assert host_poly(host, otk, mac) == tag == SUN_TAG
    for n in (0, 1, 15, 16, 17, 31, 33, 114):                # partial last blocks of the stand-alone MAC
        assert host_poly(host, otk, SUNSCREEN[:n]) == PS.poly1305(otk, SUNSCREEN[:n]), n


@pytest.mark.parametrize("w", SC.LENGTHS)
def test_host_rows_equal_pyref_and_open(host, w):
    for row, words in zip((0, 65, 69), SC.payloads(w, 3)):
        sealed = host_seal(host, SC.KEY, PS.KIND_USER, row, SC.NONCE_HI, words)
        assert [int(x) for x in sealed] == PS.seal_row(SC.KEY, PS.KIND_USER, row, SC.NONCE_HI, words)
        code, plain = host_open(host, SC.KEY, PS.KIND_USER, w, sealed)
        assert code == 0 and np.array_equal(plain, words)
        # one flipped bit per region, another key, another kind: refused, and nothing of the plaintext comes out
        for pos in (0, 1, 2, 3, 4, 5, PS.HEAD, PS.HEAD + w - 1, PS.HEAD + w, PS.HEAD + w + 3):
            bad = sealed.copy()
            bad[pos] ^= 1 << (pos % 32)
            code, plain = host_open(host, SC.KEY, PS.KIND_USER, w, bad)
            assert code == PS.REFUSED and not plain.any(), pos
            assert PS.unseal_row(SC.KEY, PS.KIND_USER, w, bad)[0] == PS.REFUSED
        for key, kind in ((SC.OTHER_KEY, PS.KIND_USER), (SC.KEY, PS.KIND_USER + 1)):
            code, plain = host_open(host, key, kind, w, sealed)
            assert code == PS.REFUSED and not plain.any()


def test_host_poly1305_corners(host):
    for name, key, msg, want in SC.POLY_CORNERS:
        assert host_poly(host, key, msg) == want, name


def test_host_poly1305_random_keys_and_limb_patterns(host):
    rg = np.random.default_rng(5)
    keys = [bytes(rg.integers(0, 256, 32, dtype=np.uint8)) for _ in range(40)] + [b"\xff" * 32, b"\xff" * 16 + bytes(16), bytes(32)]
    msgs = [b"\xff" * 64, bytes(48), bytes(rg.integers(0, 256, 200, dtype=np.uint8)), b"\xff" * 1000]
    for key in keys:
        for msg in msgs:
            assert host_poly(host, key, msg) == PS.poly1305(key, msg)
