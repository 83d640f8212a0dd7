"""Writes the fixture file that tests/cpp/test_shim.cpp reads — the reference's own unit tests re-stated over include/mpecdsa.hpp, the
C++ host layer above the C-ABI: the seeded fixtures of tests/fixtures.py as flat little-endian word arrays.  (tests/cpp_build.py
builds the program.)"""
import struct

import numpy as np

import fixtures as F
import pyref

# the signer sets of the reference's state-machine tests (state_machine/sign.rs:726-762: t1_n2_s2, t1_n3_s2 x 3, t2_n3_s3)
SM_CASES = [(1, 2, [0, 1]), (1, 3, [0, 1]), (1, 3, [0, 2]), (1, 3, [1, 2]), (2, 3, [0, 1, 2])]


def write_fixture(path, keys, B=6, seed="cpp-shim"):
    r = F.Rng(seed)
    rs = lambda: r.below(pyref.Q - 1) + 1
    ek, st = keys[:2], keys[5:7]
    nst = len(st)
    kidx = [i % 2 for i in range(B)]
    sidx = [(i + 1) % nst for i in range(B)]
    a, b = [rs() for _ in range(B)], [rs() for _ in range(B)]
    r_a = [r.coprime_below(ek[k].N) for k in kidx]
    one = [F.alice_nonces(r, ek[kidx[i]], st[sidx[i]]) for i in range(B)]                         # alice_zkp: one statement per item
    al = [F.alice_nonces(r, ek[kidx[i]], st[s]) for i in range(B) for s in range(nst)]            # MessageA: every statement per exchange
    pd = [F.pdl_nonces(r, ek[kidx[i]], st[sidx[i]]) for i in range(B)]
    arrays = {
        "N": F.words([k.N for k in ek], 64), "p": F.words([k.p for k in ek], 32), "q": F.words([k.q for k in ek], 32),
        "Nt": F.words([k.Nt for k in st], 64), "h1": F.words([k.h1 for k in st], 64), "h2": F.words([k.h2 for k in st], 64),
        "key_idx": np.array(kidx, dtype=np.uint32).reshape(B, 1), "st_idx": np.array(sidx, dtype=np.uint32).reshape(B, 1),
        "a": F.words(a, 8), "b": F.words(b, 8), "r_a": F.words(r_a, 64),
        "mb_r": F.words([r.coprime_below(ek[k].N) for k in kidx], 64), "beta_tag": F.words([r.below(ek[k].N) for k in kidx], 64),
        "nonce_b": F.words([rs() for _ in range(B)], 8), "nonce_bt": F.words([rs() for _ in range(B)], 8),
    }
    for f, w in (("alpha", 24), ("beta", 64), ("gamma", 88), ("rho", 72)):
        arrays["one_" + f] = F.words([n[f] for n in one], w)
        arrays["al_" + f] = F.words([n[f] for n in al], w)
        arrays["pdl_" + f] = F.words([n[f] for n in pd], w)
    arrays.update(bob_zkp_case(keys, ek, st))
    arrays.update(lindell_case(keys))
    arrays.update(state_machine_cases(keys))
    with open(path, "wb") as f:
        for name, arr in arrays.items():
            arr = np.ascontiguousarray(arr, dtype=np.uint32)
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<II", arr.shape[1], arr.shape[0]) + arr.tobytes())
    return arrays


def state_machine_cases(keys, B=2):
    """LocalKeys, sampled values and messages of the signer sets the reference's `simulate_signing_*` tests run, as "sm<k>_<field>"
    arrays: the public vectors and every party's secrets (the C++ test gives each OfflineStage only its own), the nonce arrays in
    the C-ABI's [B][S] layout, msg[0] = SHA-256("ZenGo") as in sign.rs:697-699"""
    import hashlib
    import gg20_fixture as G
    out = {"sm_count": np.array([[len(SM_CASES)]], dtype=np.uint32)}
    for k, (t, n, signers) in enumerate(SM_CASES):
        lk = G.make_local_keys(keys, t, n, signers, seed=f"cpp-sm-keygen-{k}")
        nn = G.make_nonces(lk, B, seed=f"cpp-sm-{k}")
        a = lk["arrays"]
        pre = f"sm{k}_"
        out[pre + "shape"] = np.array([[t, n, len(signers), B]], dtype=np.uint32)
        out[pre + "signers"] = np.array(signers, dtype=np.uint32).reshape(-1, 1)
        for f in ("x", "p", "q", "Nt", "h1", "h2", "y", "X"):
            out[pre + f] = a[f]
        out[pre + "N"] = F.words([keys[i].N for i in range(n)], 64)
        msg = np.array(nn["msg"], copy=True)
        msg[0] = F.words([int.from_bytes(hashlib.sha256(b"ZenGo").digest(), "big") % pyref.Q], 8)[0]
        for f in G.NONCE_FIELDS:
            out[pre + f] = msg if f == "msg" else nn[f]
    return out


def bob_zkp_case(keys, ek, st, B=25):
    """`bob_zkp` (range_proofs.rs:636-709): 5 x 5 runs of MtA / MtAwc with fresh inputs = one batch of 25; "bz_<field>" arrays"""
    r = F.Rng("cpp-bob-zkp")
    rs = lambda: r.below(pyref.Q - 1) + 1
    kidx = [i % len(ek) for i in range(B)]
    sidx = [(i // 5) % len(st) for i in range(B)]
    nn = [F.bob_nonces(r, ek[kidx[i]], st[sidx[i]]) for i in range(B)]
    out = {"bz_key_idx": np.array(kidx, dtype=np.uint32).reshape(B, 1), "bz_st_idx": np.array(sidx, dtype=np.uint32).reshape(B, 1),
           "bz_a": F.words([rs() for _ in range(B)], 64), "bz_r_enc_a": F.words([r.coprime_below(ek[k].N) for k in kidx], 64),
           "bz_b": F.words([rs() for _ in range(B)], 8), "bz_beta_prim": F.words([r.below(ek[k].N) for k in kidx], 64),
           "bz_r": F.words([r.coprime_below(ek[k].N) for k in kidx], 64)}
    for f, w in (("alpha", 24), ("beta", 64), ("gamma", 80), ("rho", 72), ("rho_prim", 88), ("sigma", 72), ("tau", 88)):
        out["bz_" + f] = F.words([n[f] for n in nn], w)
    return out


def lindell_case(keys, B=8):
    """`test_two_party_sign` (lindell_2017/test.rs:85-137), B pairs of parties at once; item 0 signs the reference's message 1234.
    "l17_<field>" arrays; the Paillier keys are the fixture's 16 (party one's key of item i = key l17_key_idx[i])"""
    import lindell_fixture as L
    fx = L.make(keys, B, seed="cpp-lindell")
    fx["msg"][0] = F.words([1234], 8)[0]
    out = {"l17_" + f: np.ascontiguousarray(fx[f]) for f in ("N", "p", "q", "c_key", "x2", "k1", "k2", "R1", "R2", "msg", "rho", "r")}
    out["l17_key_idx"] = np.array(fx["kidx"], dtype=np.uint32).reshape(B, 1)
    out["l17_pub"] = F.point_words(fx["pub"])
    return out
