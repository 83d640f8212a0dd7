"""BIP32 public derivation (CKDpub) restated over hashlib / hmac (OpenSSL-backed) and the EC arithmetic of tests/pyref.py, with the
row conventions of mpe_bip32_derive, and the child-wallet builder the GG20 tweak tests compare against:
adding a public tweak t to every Shamir share gives the wallet of the child key x + t (x_i + t, X_i + t G, y + t G, everything else
the same)."""
import hashlib
import hmac

import numpy as np

import fixtures as F
import pyref

Q = pyref.Q
STATUS_HARDENED, STATUS_INVALID, STATUS_DEPTH = 1, 2, 3
BAD_TWEAK = 93
ALL_ONES = (1 << 256) - 1


def ser_p(pt):
    """the 33-byte compressed form: always 33 bytes, whatever the size of x"""
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def ckd_pub(K, cc, i):
    """one level: (I_L, child key, child chain code), or None where BIP32 calls the index invalid (I_L >= q, child at infinity)"""
    assert 0 <= i < 1 << 31 and len(cc) == 32
    I = hmac.new(cc, ser_p(K) + i.to_bytes(4, "big"), hashlib.sha512).digest()
    il = int.from_bytes(I[:32], "big")
    if il >= Q:
        return None
    child = pyref.ec_add(pyref.ec_mul(il, pyref.G), K)
    if child is None:
        return None
    return il, child, I[32:]


def ckd_priv(x, cc, i):
    """the non-hardened private derivation, for the check child_priv G == child_pub"""
    I = hmac.new(cc, ser_p(pyref.ec_mul(x, pyref.G)) + i.to_bytes(4, "big"), hashlib.sha512).digest()
    return (x + int.from_bytes(I[:32], "big")) % Q, I[32:]


def derive(parents, parent_idx, path, depth, max_depth):
    """one row of mpe_bip32_derive: (status, tweak, child key or None, chain code).  parents: [(K, cc)]; path: max_depth indices.
    A failed row: the all-ones tweak, no key, a zero chain code."""
    failed = lambda st: (st, ALL_ONES, None, bytes(32))
    if not 0 <= parent_idx < len(parents) or not 0 <= depth <= max_depth:
        return failed(STATUS_DEPTH)
    if any(i >> 31 for i in path[:depth]):
        return failed(STATUS_HARDENED)
    K, cc = parents[parent_idx]
    t = 0
    for i in path[:depth]:
        step = ckd_pub(K, cc, i)
        if step is None:
            return failed(STATUS_INVALID)
        il, K, cc = step
        t = (t + il) % Q
    return 0, t, K, cc


def child_wallet(lk, t):
    """the gg20_fixture LocalKey of the child key x + t: shares x_i + t, X_i + t G, y + t G; Paillier keys, N~ statements and the signer
    set are the parent's (the arrays are copies)"""
    tG = pyref.ec_mul(t % Q, pyref.G)
    arrays = {f: np.array(a, copy=True) for f, a in lk["arrays"].items()}
    arrays["x"] = F.words([(x + t) % Q for x in F.ints(lk["arrays"]["x"])], 8)
    arrays["X"] = F.point_words([pyref.ec_add(X, tG) for X in F.points(lk["arrays"]["X"])])
    y = pyref.ec_add(lk["y"], tG)
    arrays["y"] = F.point_words([y])
    return dict(lk, arrays=arrays, y=y, x=(lk["x"] + t) % Q)
