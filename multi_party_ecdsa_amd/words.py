"""Host-side conversion between Python integers and the C-ABI's little-endian u32 word arrays
(the analogue of curv `Converter::to_bytes/from_bytes`, big-endian there)."""
import numpy as np


def ints_to_words(vals, nwords):
    """list of non-negative ints -> np.uint32 array [len(vals), nwords] (little-endian words)."""
    buf = b"".join(int(v).to_bytes(nwords * 4, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u4").reshape(len(vals), nwords).copy()


def words_to_ints(arr):
    """np.uint32 array [n, nwords] -> list of ints."""
    a = np.ascontiguousarray(arr, dtype="<u4")
    nbytes = a.shape[1] * 4
    raw = a.tobytes()
    return [int.from_bytes(raw[i * nbytes:(i + 1) * nbytes], "little") for i in range(a.shape[0])]


# ---- signer sets of a many-set key object (mpe_gg20_keys_create_sets) --------------------------------------------------------
# A set is `S` ascending, distinct party indices below n <= 8.  The library keeps one 32-bit word per set: the party index of signer
# ordinal i in bits [4 i, 4 i + 4).  A presignature record names its set by the bit mask over party indices.
def pack_signer_set(signers):
    s = [int(x) for x in signers]
    if not s or len(s) > 8 or any(x < 0 or x > 7 for x in s) or any(b <= a for a, b in zip(s, s[1:])):
        raise ValueError(f"signer set {signers}: 1..8 ascending distinct party indices below 8")
    word = 0
    for i, p in enumerate(s):
        word |= p << (4 * i)
    return word


def unpack_signer_set(word, S):
    return [(int(word) >> (4 * i)) & 15 for i in range(S)]


def signer_set_mask(signers):
    mask = 0
    for p in signers:
        mask |= 1 << int(p)
    return mask


def signer_set_table(sets, n=8):
    """[[party, ...], ...] -> np.int32 [n_sets, S] as mpe_gg20_keys_create_sets takes it (rows checked: same length, ascending, distinct
    indices below n, no two equal rows, at most 256 rows)"""
    rows = [[int(x) for x in s] for s in sets]
    if not 1 <= len(rows) <= 256:
        raise ValueError("1..256 signer sets")
    if any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("every signer set of a key object has the same number of signers")
    words = [pack_signer_set(r) for r in rows]
    if any(x >= n for r in rows for x in r):
        raise ValueError(f"party index not below n = {n}")
    if len(set(words)) != len(words):
        raise ValueError("two equal signer sets")
    return np.asarray(rows, dtype=np.int32)


def rank_in_set(signers, party):
    """the signer ordinal of `party` in a set (its position in the ascending list), or -1: what a by-index local party's ordinal is"""
    word, S = pack_signer_set(signers), len(signers)
    r = -1
    for i in range(S):
        if (word >> (4 * i)) & 15 == int(party):
            r = i
    return r
