"""The cases tests/test_seal_cpu.py and tests/test_seal_gpu.py share: payload lengths on both sides of the 16-byte Poly1305 block
and the 64-byte ChaCha20 block, the key-share row (72 words) and the presignature records of 1, 2, 3 and 5 local parties
(28 + 32 L words), random and all-0xff payloads, and the Poly1305 reduction corners that need a chosen r."""
import numpy as np

LENGTHS = [1, 3, 4, 5, 15, 16, 17, 60, 72, 92, 124, 188]
KEY = bytes(range(0x80, 0xA0))                               # the key of RFC 8439 §2.8.2
OTHER_KEY = bytes((7 * i + 3) & 0xFF for i in range(32))
NONCE_HI = 0x0123456789ABCDEF


def payloads(w, rows):
    """[rows, w] uint32: random rows, the last one all 0xff"""
    rg = np.random.default_rng(1000 + w)
    a = rg.integers(0, 1 << 32, size=(rows, w), dtype=np.uint64).astype(np.uint32)
    a[-1] = 0xFFFFFFFF
    return a


def key_words(key: bytes):
    return np.frombuffer(key, dtype="<u4").astype(np.uint32)


# (name, key r | s as 32 bytes, message, expected tag): r = 1 survives the clamp, so the accumulator is the sum of the blocks
_R1 = (1).to_bytes(16, "little")
_FF = b"\xff" * 16
POLY_CORNERS = [
    ("2^130 - 2 before the last reduction", _R1 + bytes(16), _FF + _FF, (3).to_bytes(16, "little")),
    ("exactly 2^130 - 5", _R1 + bytes(16), b"\xfc" + _FF[1:] + _FF, bytes(16)),
    ("2^130 - 6: no subtraction", _R1 + bytes(16), b"\xfb" + _FF[1:] + _FF, b"\xfa" + _FF[1:]),
    ("the addition of s carries out of 128 bits", _R1 + _FF, _FF + _FF, (2).to_bytes(16, "little")),
]
