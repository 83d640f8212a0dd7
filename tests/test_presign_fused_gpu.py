"""GPU: `mpe_gg20_presign_sets` (engine.gg20_presign_fused) — the offline stage as one C call that chunks like mpe_gg20_sign_sets and
deposits where that function signs.  The world is the mixed-set one of tests/test_sigsets_presig_gpu.py; the yardstick is the session
path (rounds 0-8) on the same nonces and messages, and mpe_gg20_sign_sets for the status a failed session reports."""
import numpy as np
import pytest
import torch

import pyref_presig as PP
import sigset_cases as SC

pytestmark = pytest.mark.gpu
CAP = 16
ALL_EMPTY = dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def world(gpu_ctx, keys):
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, S = gpu_ctx, 1, 3, 2
    sets = SC.all_sets(n, S)
    sigset = [0, 1, 2, 2, 0, 1, 1, 2, 0]
    B = len(sigset)
    lks, per_wallet = SC.wallet(keys, t, n, sets)
    nonces = SC.mixed_nonces(per_wallet, sigset, seed="presign-fused")
    gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], signer_sets=sets)
    dn = {f: _dev(ctx, v) for f, v in nonces.items()}
    ds = torch.tensor(sigset, dtype=torch.int32, device=ctx.device)
    # the session path: rounds 0-8 on the same nonces and messages
    sess = E.Gg20Session(ctx, gk, B, list(range(S)), dn, sigset=ds)
    prev = None
    for rnd in range(7):
        prev = sess.round(rnd, d_in=prev)
    sess.round(8, d_in=sess.round(7, msg=dn["msg"]))
    res = sess.result()
    ctx.sync()
    want = dict(r=_u32(res["r"])[0], s=_u32(res["s"])[0], recid=res["recid"].cpu().numpy()[0])
    assert not res["status"].cpu().numpy().any()
    sess.close()
    yield dict(ctx=ctx, S=S, B=B, sigset=sigset, nonces=nonces, gk=gk, dn=dn, ds=ds, want=want)
    gk.close()


def _same(got, want, rows):
    r, s, recid, status = [o.cpu().numpy() for o in got]
    assert not status.any()
    assert np.array_equal(r.view(np.uint32), want["r"][rows]) and np.array_equal(s.view(np.uint32), want["s"][rows])
    assert list(recid) == list(want["recid"][rows])


def test_fused_offline_stage_then_online_in_another_order_equals_the_session_path(world):
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx, B, S = w["ctx"], w["B"], w["S"]
    pool = E.PresigPool(ctx, w["gk"], list(range(S)), CAP)
    slots = np.array([(7 * i + 3) % CAP for i in range(B)], dtype=np.int32)          # a permutation with gaps
    dn = {f: v for f, v in w["dn"].items() if f != "msg"}                            # the call reads no message
    assert np.array_equal(E.gg20_presign_fused(ctx, w["gk"], dn, B, pool, slots=slots, sigset=w["ds"]), slots)
    assert not pool.last_status.any()
    assert pool.audit() == dict(EMPTY=CAP - B, READY=B, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP - B
    first, second = np.array([8, 1, 5, 0]), np.array([2, 7, 3, 6, 4])
    _same(E.gg20_sign_online(pool, slots[first], _dev(ctx, w["nonces"]["msg"][first])), w["want"], first)
    _same(pool.sign_online(slots[second], _dev(ctx, w["nonces"]["msg"][second])), w["want"], second)
    assert pool.audit() == ALL_EMPTY and pool.free_slots() == CAP
    # ... and into slots of the pool's own free list
    got = E.gg20_presign_fused(ctx, w["gk"], w["dn"], B, pool, sigset=w["ds"])
    assert list(got) == list(range(B))
    order = np.array([4, 0, 8, 2, 6, 1, 7, 3, 5])
    _same(pool.sign_online(got[order], _dev(ctx, w["nonces"]["msg"][order])), w["want"], order)
    assert pool.audit() == ALL_EMPTY
    pool.close()


def test_a_failed_session_a_bad_set_and_an_occupied_slot_report_their_own_status(world):
    """session 3 encrypts with r_a = 0 (the tamper of test_a_tampered_batch_fails_alone), row 5 names set index 7, row 7 names a slot
    that is READY: the rows read the session's own status (what mpe_gg20_sign_sets reports), 92 and 802; their slots are unchanged;
    the other rows are READY and sign"""
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx, B, S = w["ctx"], w["B"], w["S"]
    pool = E.PresigPool(ctx, w["gk"], list(range(S)), CAP)
    slots = np.array([(5 * i + 2) % CAP for i in range(B)], dtype=np.int32)
    # the occupied slot: session 0's presignature, deposited alone by an earlier call
    held = 15
    assert held not in slots
    one = {f: v[:v.shape[0] // B].contiguous() for f, v in w["dn"].items()}
    assert list(E.gg20_presign_fused(ctx, w["gk"], one, 1, pool, slots=[held], sigset=w["ds"][:1])) == [held]
    bad = {f: v.copy() for f, v in w["nonces"].items()}
    bad["r_a"][3 * S:4 * S] = 0
    sigset = list(w["sigset"])
    sigset[5] = 7
    named = slots.copy()
    named[7] = held
    dn, ds = {f: _dev(ctx, v) for f, v in bad.items()}, torch.tensor(sigset, dtype=torch.int32, device=ctx.device)
    yard = E.gg20_sign(ctx, w["gk"], dn, B, sigset=ds)[3].cpu().numpy()
    assert yard[3] != 0 and yard[5] == SC.BAD_SET and not yard[[0, 1, 2, 4, 6, 7, 8]].any()
    got = E.gg20_presign_fused(ctx, w["gk"], dn, B, pool, slots=named, sigset=ds)
    want = yard.copy()
    want[7] = PP.DEPOSIT_NOT_EMPTY
    assert list(pool.last_status) == list(want)
    good = np.array([0, 1, 2, 4, 6, 8])
    assert list(got) == [int(named[b]) if b in good else -1 for b in range(B)]
    assert pool.audit() == dict(EMPTY=CAP - 7, READY=7, SIGNED=0, BUSY=0, stray=0)
    # the slots of rows 3 and 5 are EMPTY; the held slot still holds session 0's presignature and the good rows sign
    st = pool.sign_online(named[[3, 5]], _dev(ctx, bad["msg"][[3, 5]]))[3].cpu().numpy()
    assert list(st) == [PP.SIGN_NOT_READY] * 2
    _same(pool.sign_online([held], _dev(ctx, bad["msg"][:1])), w["want"], np.array([0]))
    _same(pool.sign_online(named[good], _dev(ctx, bad["msg"][good])), w["want"], good)
    assert pool.audit() == ALL_EMPTY
    pool.close()


def test_chunks_of_four_deposit_what_one_chunk_deposits(world):
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx, B, S = w["ctx"], w["B"], w["S"]
    pool = E.PresigPool(ctx, w["gk"], list(range(S)), CAP)
    slots = np.array([(3 * i + 1) % CAP for i in range(B)], dtype=np.int32)
    recs = []
    for chunk in (4, 0):
        assert np.array_equal(E.gg20_presign_fused(ctx, w["gk"], w["dn"], B, pool, slots=slots, sigset=w["ds"], chunk=chunk), slots)
        rec, st = pool.export(slots)
        assert not st.cpu().numpy().any()
        recs.append(_u32(rec).copy())
    assert recs[0].any() and np.array_equal(recs[0], recs[1])
    assert pool.audit() == ALL_EMPTY
    pool.close()


def test_a_pool_that_lacks_a_signer_is_refused_and_untouched(world):
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx, B = w["ctx"], w["B"]
    pool = E.PresigPool(ctx, w["gk"], [0], CAP)
    with pytest.raises(E.N_.MpeError):
        E.gg20_presign_fused(ctx, w["gk"], w["dn"], B, pool, sigset=w["ds"])
    assert pool.audit() == ALL_EMPTY and pool.free_slots() == CAP
    with pytest.raises(E.N_.MpeError):
        pool.sign_online([0], _dev(ctx, w["nonces"]["msg"][:1]))                     # the fused online step needs every signer too
    assert pool.audit() == ALL_EMPTY
    pool.close()
