"""Case builder for batches whose sessions name their own signer set (`mpe_gg20_*_sets`), shared by the CPU and GPU tests.

A wallet is shared out once; `gg20_fixture.make_local_keys` is called once per signer set so that `arrays["signers"]` is that set (the
shares, the Paillier and N~ material are the same in all of them).  A mixed batch takes row b of every nonce field from
`gg20_fixture.make_nonces(lk_of_set, B, seed)` — the sampled ranges depend on the peers' moduli, hence on the set — and its
expectation comes from the oracle session by session: `orc_gg20_sign_ex` called with that session's set for `first = b, count = 1`."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np

import gg20_fixture as G

_spec = importlib.util.spec_from_file_location("mpe_words", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multi_party_ecdsa_amd", "words.py"))
words = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(words)

wire = G.wire
KEY_FIELDS = ("x", "p", "q", "Nt", "h1", "h2", "y", "X")
BAD_SET = 92


def all_sets(n, S):
    """every signer set of S parties out of n, in lexicographic order: 3 for (3, 2), 10 for (5, 3), 70 for (8, 4)"""
    return [list(c) for c in itertools.combinations(range(n), S)]


def wallet(keys, t, n, sets, nwallets=1):
    """lks[k] = the LocalKey fixture whose signer set is sets[k]; with nwallets > 1 the arrays hold that many key sets (wallet kk on the
    Paillier material rotated by kk, its own polynomial) and `per_wallet[kk][k]` are the single-wallet fixtures the nonces are drawn for"""
    per_wallet = [[G.make_local_keys(keys[kk:] + keys[:kk], t, n, s, seed="keygen" if kk == 0 else f"sigset-wallet-{kk}") for s in sets]
                  for kk in range(nwallets)]
    if nwallets == 1:
        return per_wallet[0], per_wallet
    lks = []
    for k in range(len(sets)):
        arrays = {f: np.concatenate([per_wallet[kk][k]["arrays"][f] for kk in range(nwallets)]) for f in KEY_FIELDS}
        arrays["signers"] = per_wallet[0][k]["arrays"]["signers"]
        lks.append(dict(per_wallet[0][k], arrays=arrays, nkeysets=nwallets))
    return lks, per_wallet


def mixed_nonces(per_wallet, sets_of_session, seed, keyset=None):
    """row b of every field from make_nonces(fixture of (wallet of b, set of b), B, seed)"""
    B = len(sets_of_session)
    ks = [0] * B if keyset is None else [int(x) for x in keyset]
    drawn = {}
    for b in range(B):
        key = (ks[b], int(sets_of_session[b]))
        if key not in drawn:
            drawn[key] = G.make_nonces(per_wallet[key[0]][key[1]], B, seed=seed)
    first = next(iter(drawn.values()))
    out = {}
    for f, a in first.items():
        per = a.shape[0] // B
        out[f] = np.ascontiguousarray(np.concatenate([drawn[(ks[b], int(sets_of_session[b]))][f][b * per:(b + 1) * per] for b in range(B)]))
    return out


def session_rows(nonces, B, sessions):
    """the rows of the sessions `sessions` of a [B]-leading nonce dict, in that order"""
    out = {}
    for f, a in nonces.items():
        per = a.shape[0] // B
        out[f] = np.ascontiguousarray(np.concatenate([a[b * per:(b + 1) * per] for b in sessions]))
    return out


def oracle_mixed(lks, nonces, sets_of_session, keyset=None):
    """The oracle's lock-step run of a mixed batch: one `orc_gg20_sign_ex` call per session (first = b, count = 1) with the key struct of
    that session's set.  Returns what gg20_fixture.oracle_sign_ex returns, over the whole batch."""
    import orc
    B = len(sets_of_session)
    S, n = lks[0]["S"], lks[0]["n"]
    slabs = {rnd: np.zeros((S, B, G.msg_words(S, n, rnd)), dtype=np.uint32) for rnd in G.ROUNDS}
    ptrs = (C.c_void_p * 7)(*[slabs[rnd].ctypes.data for rnd in G.ROUNDS])
    r, s = np.zeros((B, 8), dtype=np.uint32), np.zeros((B, 8), dtype=np.uint32)
    recid, status = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    R = np.zeros((B, 16), dtype=np.uint32)
    pst, pbad = np.zeros((S, B), dtype=np.int32), np.zeros((S, B), dtype=np.uint32)
    ns = G.nonces_struct(nonces)
    kset = None if keyset is None else np.ascontiguousarray(keyset, dtype=np.int32)
    for b in range(B):
        ks = G.keys_struct(lks[int(sets_of_session[b])])
        orc.lib.orc_gg20_sign_ex(C.byref(ks), C.byref(ns), orc._p(kset), B, b, 1, ptrs, orc._p(r), orc._p(s), orc._p(recid), orc._p(R),
                                 orc._p(status), orc._p(pst), orc._p(pbad))
    return dict(slabs=slabs, r=r, s=s, recid=recid, R=R, status=status, party_status=pst, party_bad=pbad)


def oracle_mixed_faults(lks, nonces, sets_of_session, step, corrupted):
    """per-party status and bad_actors [S][B] of a mixed batch in which the signer ORDINALS `corrupted` of every session run the reference's
    corrupt_step: the sessions of one set run together as OracleParty objects of that set"""
    B, S = len(sets_of_session), lks[0]["S"]
    pst, pbad = np.zeros((S, B), dtype=np.int32), np.zeros((S, B), dtype=np.uint32)
    for k in sorted(set(int(x) for x in sets_of_session)):
        sessions = [b for b in range(B) if int(sets_of_session[b]) == k]
        sub = session_rows(nonces, B, sessions)
        parties = [G.OracleParty(lks[k], i, len(sessions), G.party_nonces(sub, lks[k], i)) for i in range(S)]
        for i in corrupted:
            parties[i].fault(step)
        G.run_rounds(parties, sub["msg"])
        for i, p in enumerate(parties):
            res = p.result()
            pst[i, sessions], pbad[i, sessions] = res["status"], res["bad_actors"]
            p.close()
    return pst, pbad


def party_mask(signers):
    return words.signer_set_mask(signers)
