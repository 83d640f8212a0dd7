"""Plain-Python restatement of the sealed rows (include/mpecdsa_hip.h, "sealed records"): ChaCha20-Poly1305 as RFC 8439 §2.8
defines it, on Python integers and bytes, plus the library's sealed-row layout.  Written from the RFC's text and the header's, not
from csrc/mpe_seal.h; tests/test_seal_cpu.py pins it to OpenSSL's EVP_chacha20_poly1305."""
import struct

MAGIC = int.from_bytes(b"MPS1", "little")
REFUSED = 841
HEAD, EXTRA, MAX_WORDS = 6, 10, 4096
KIND_PRESIG, KIND_KEYSHARE, KIND_USER = 1, 2, 16
P1305 = (1 << 130) - 5


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF


def _qr(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & 0xFFFFFFFF; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & 0xFFFFFFFF; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & 0xFFFFFFFF; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & 0xFFFFFFFF; s[b] = _rotl(s[b] ^ s[c], 7)


def chacha20_block(key: bytes, counter: int, nonce: bytes) -> bytes:
    """RFC 8439 §2.3: 32-byte key, 32-bit block counter, 12-byte nonce -> 64 bytes"""
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(struct.unpack("<8I", key)) + [counter & 0xFFFFFFFF] + list(struct.unpack("<3I", nonce))
    s = list(init)
    for _ in range(10):
        _qr(s, 0, 4, 8, 12); _qr(s, 1, 5, 9, 13); _qr(s, 2, 6, 10, 14); _qr(s, 3, 7, 11, 15)
        _qr(s, 0, 5, 10, 15); _qr(s, 1, 6, 11, 12); _qr(s, 2, 7, 8, 13); _qr(s, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & 0xFFFFFFFF for a, b in zip(s, init)])


def chacha20_xor(key, counter, nonce, data):
    out = bytearray()
    for i in range(0, len(data), 64):
        ks = chacha20_block(key, counter + i // 64, nonce)
        out += bytes(a ^ b for a, b in zip(data[i:i + 64], ks))
    return bytes(out)


def poly1305(key: bytes, msg: bytes) -> bytes:
    """RFC 8439 §2.5: key = r | s, 16 bytes each"""
    r = int.from_bytes(key[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    s = int.from_bytes(key[16:], "little")
    acc = 0
    for i in range(0, len(msg), 16):
        acc = (acc + int.from_bytes(msg[i:i + 16] + b"\x01", "little")) * r % P1305
    return ((acc + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def _pad16(b):
    return b + b"\x00" * (-len(b) % 16)


def aead_encrypt(key, nonce, aad, plaintext):
    """RFC 8439 §2.8 -> (ciphertext, tag)"""
    otk = chacha20_block(key, 0, nonce)[:32]
    ct = chacha20_xor(key, 1, nonce, plaintext)
    mac = _pad16(aad) + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    return ct, poly1305(otk, mac)


def aead_decrypt(key, nonce, aad, ct, tag):
    """the plaintext, or None when the tag does not match"""
    otk = chacha20_block(key, 0, nonce)[:32]
    mac = _pad16(aad) + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    if poly1305(otk, mac) != tag:
        return None
    return chacha20_xor(key, 1, nonce, ct)


def _bytes(words):
    return struct.pack(f"<{len(words)}I", *[int(w) for w in words])


def _words(b):
    return list(struct.unpack(f"<{len(b) // 4}I", b))


def seal_row(key: bytes, kind: int, row: int, nonce_hi: int, words):
    """the sealed row (w + 10 words) of payload `words` as row `row` of a call with `nonce_hi`"""
    w = len(words)
    assert 1 <= w <= MAX_WORDS
    head = [MAGIC, kind, w]
    nonce = [row & 0xFFFFFFFF, nonce_hi & 0xFFFFFFFF, (nonce_hi >> 32) & 0xFFFFFFFF]
    ct, tag = aead_encrypt(key, _bytes(nonce), _bytes(head), _bytes(words))
    return head + nonce + _words(ct) + _words(tag)


def unseal_row(key: bytes, kind: int, w: int, sealed):
    """(status, payload words): (0, words) or (REFUSED, [0] * w) for a wrong magic, kind, length or tag"""
    sealed = [int(x) for x in sealed]
    assert len(sealed) == w + EXTRA
    if sealed[:3] != [MAGIC, kind, w]:
        return REFUSED, [0] * w
    pt = aead_decrypt(key, _bytes(sealed[3:6]), _bytes(sealed[:3]), _bytes(sealed[HEAD:HEAD + w]), _bytes(sealed[HEAD + w:]))
    return (REFUSED, [0] * w) if pt is None else (0, _words(pt))
