"""GPU: `mpe_gg20_sign_online` (PresigPool.sign_online) — the online step as one kernel: claim, every s_i, the sum, the low-s rule,
ONE verify, the wipe.  The yardstick is the composed path engine.gg20_sign_online (sign + complete, one verify per local party) on the
SAME presignatures: the exported records are imported twice, into two pools, and the oracle on the same nonces and messages."""
import hashlib

import numpy as np
import pytest
import torch

import fixtures as F
import gg20_fixture as G
import pyref_presig as PP

pytestmark = pytest.mark.gpu
CAP, B = 16, 9
ALL_EMPTY = dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def world(gpu_ctx, keys):
    """B presignatures as records (the only copy), the messages chosen afterwards, and the oracle's signatures"""
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, signers = gpu_ctx, 1, 3, [0, 2]
    lk = G.make_local_keys(keys, t, n, signers)
    nonces = G.make_nonces(lk, B, seed="presig-online")
    nonces["msg"] = F.words([int.from_bytes(hashlib.sha256(b"online %d" % b).digest(), "big") for b in range(B)], 8)
    gk = E.Gg20Keys(ctx, t, n, signers, lk["arrays"])
    pool = E.PresigPool(ctx, gk, [0, 1], CAP)
    slots = E.gg20_presign_fused(ctx, gk, {f: _dev(ctx, v) for f, v in nonces.items() if f != "msg"}, B, pool)
    assert list(slots) == list(range(B))
    rec, st = pool.export(slots)
    assert not st.cpu().numpy().any() and pool.audit() == ALL_EMPTY
    pool.close()
    wr, ws, wrecid, _, wstatus = G.oracle_sign(lk, nonces, B)
    assert not wstatus.any()
    yield dict(ctx=ctx, gk=gk, rec=rec, msg=nonces["msg"], want=(wr, ws, wrecid))
    gk.close()


def _np(out):
    r, s, recid, status = [o.cpu().numpy() for o in out]
    return r.view(np.uint32), s.view(np.uint32), recid, status


def test_fused_and_composed_online_steps_give_identical_bytes(world):
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx = w["ctx"]
    fused, composed = E.PresigPool(ctx, w["gk"], [0, 1], CAP), E.PresigPool(ctx, w["gk"], [0, 1], CAP)
    there = np.array([(7 * i + 3) % CAP for i in range(B)], dtype=np.int32)
    for p in (fused, composed):
        assert np.array_equal(p.import_(w["rec"], there), there)
    order = np.array([4, 0, 8, 2, 6, 1, 7, 3, 5])
    d_msg = _dev(ctx, w["msg"][order])
    a, b = _np(fused.sign_online(there[order], d_msg)), _np(E.gg20_sign_online(composed, there[order], d_msg))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    wr, ws, wrecid = w["want"]
    assert not a[3].any() and np.array_equal(a[0], wr[order]) and np.array_equal(a[1], ws[order]) and list(a[2]) == list(wrecid[order])
    for p in (fused, composed):
        assert p.audit() == ALL_EMPTY and p.free_slots() == CAP
        p.close()


def test_duplicate_indices_have_one_winner_and_an_index_out_of_range_is_811(world):
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx = w["ctx"]
    pool = E.PresigPool(ctx, w["gk"], [0, 1], CAP)
    assert list(pool.import_(w["rec"][:2].contiguous(), [5, 11])) == [5, 11]
    rows = np.array([5, 5, CAP + 83, 11, -1, 5], dtype=np.int32)
    src = np.array([0, 0, 0, 1, 0, 0])                              # the presignature (and message) a winning row signs with
    r, s, recid, status = _np(pool.sign_online(rows, _dev(ctx, w["msg"][src])))
    dup = [0, 1, 5]
    assert sorted(status[dup]) == [0, PP.SIGN_NOT_READY, PP.SIGN_NOT_READY]
    assert status[2] == PP.SIGN_RANGE and status[4] == PP.SIGN_RANGE and status[3] == 0
    wr, ws, wrecid = w["want"]
    for g in range(len(rows)):
        if status[g] == 0:
            assert np.array_equal(r[g], wr[src[g]]) and np.array_equal(s[g], ws[src[g]]) and recid[g] == wrecid[src[g]]
        else:
            assert not r[g].any() and not s[g].any() and recid[g] == 0
    assert pool.audit() == ALL_EMPTY and pool.free_slots() == CAP
    # a slot signs once: the second call finds it EMPTY
    assert list(_np(pool.sign_online([5, 11], _dev(ctx, w["msg"][:2])))[3]) == [PP.SIGN_NOT_READY] * 2
    assert pool.audit() == ALL_EMPTY
    pool.close()


def test_an_altered_sigma_fails_the_one_verify_with_zero_outputs_and_an_empty_slot(world):
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx = w["ctx"]
    rec = _u32(w["rec"])[:3].copy()
    at = PP.REC_HEAD + 8                                            # sigma_0 of record 1, altered by one
    assert rec[1, at] != 0xFFFFFFFF
    rec[1, at] += 1
    pool, composed = E.PresigPool(ctx, w["gk"], [0, 1], CAP), E.PresigPool(ctx, w["gk"], [0, 1], CAP)
    for p in (pool, composed):
        assert list(p.import_(_dev(ctx, rec), [2, 9, 4])) == [2, 9, 4]
    d_msg = _dev(ctx, w["msg"][:3])
    r, s, recid, status = _np(pool.sign_online([2, 9, 4], d_msg))
    assert list(status) == [0, PP.VERIFY_FAILED, 0] == list(_np(E.gg20_sign_online(composed, [2, 9, 4], d_msg))[3])
    assert not r[1].any() and not s[1].any() and recid[1] == 0
    wr, ws, wrecid = w["want"]
    assert np.array_equal(r[[0, 2]], wr[[0, 2]]) and np.array_equal(s[[0, 2]], ws[[0, 2]]) and list(recid[[0, 2]]) == list(wrecid[[0, 2]])
    for p in (pool, composed):
        assert p.audit() == ALL_EMPTY and p.free_slots() == CAP
        p.close()
