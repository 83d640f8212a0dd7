"""GPU: the presignature pool over a key object with several signer sets.  A slot remembers the set its session signed with; the
export record carries that set's party mask in its existing mask word; import accepts a record of any of the key object's sets.  The
yardstick is the session path on the same nonces and messages; a pool over a one-set object reads and writes the bytes it always did
(tests/pyref_presig.py)."""
import numpy as np
import pytest
import torch

import fixtures as F
import gg20_fixture as G
import pyref_presig as PP
import sigset_cases as SC

pytestmark = pytest.mark.gpu
CAP = 16


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _offline(ctx, gk, B, S, dn, sigset=None):
    from multi_party_ecdsa_amd import engine as E
    sess = E.Gg20Session(ctx, gk, B, list(range(S)), dn, sigset=sigset)
    prev = None
    for rnd in range(7):
        prev = sess.round(rnd, d_in=prev)
    return sess


def _online(pool, slots, d_msg):
    from multi_party_ecdsa_amd import engine as E
    return [o.cpu().numpy() for o in E.gg20_sign_online(pool, slots, d_msg)]


@pytest.fixture(scope="module")
def world(gpu_ctx, keys):
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, S = gpu_ctx, 1, 3, 2
    sets = SC.all_sets(n, S)
    sigset = [0, 1, 2, 2, 0, 1, 1, 2, 0]
    B = len(sigset)
    lks, per_wallet = SC.wallet(keys, t, n, sets)
    nonces = SC.mixed_nonces(per_wallet, sigset, seed="sigsets-presig")
    gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], signer_sets=sets)
    dn = {f: _dev(ctx, v) for f, v in nonces.items()}
    ds = torch.tensor(sigset, dtype=torch.int32, device=ctx.device)
    # the session path: rounds 0-8 on the same nonces and messages
    sess = _offline(ctx, gk, B, S, dn, sigset=ds)
    s_i = sess.round(7, msg=dn["msg"])
    sess.round(8, d_in=s_i)
    res = sess.result()
    ctx.sync()
    fused = dict(r=_u32(res["r"])[0], s=_u32(res["s"])[0], recid=res["recid"].cpu().numpy()[0], status=res["status"].cpu().numpy())
    sess.close()
    assert not fused["status"].any()
    return dict(ctx=ctx, t=t, n=n, S=S, B=B, sets=sets, sigset=sigset, lks=lks, nonces=nonces, gk=gk, dn=dn, ds=ds, fused=fused)


def _same(got, fused, rows):
    r, s, recid, status = got
    assert not status.any()
    assert np.array_equal(r.view(np.uint32), fused["r"][rows]) and np.array_equal(s.view(np.uint32), fused["s"][rows])
    assert list(recid) == list(fused["recid"][rows])


def test_mixed_sessions_through_the_pool_equal_the_session_path(world):
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx, B, S = w["ctx"], w["B"], w["S"]
    pool = E.PresigPool(ctx, w["gk"], list(range(S)), CAP)
    slots = np.array([(7 * i + 3) % CAP for i in range(B)], dtype=np.int32)          # a permutation with gaps
    # engine.gg20_presign(sigset=): the pool's own free list hands out slots 0 .. B-1
    got = E.gg20_presign(ctx, w["gk"], w["dn"], B, pool, sigset=w["ds"])
    assert list(got) == list(range(B))
    rows = np.array([6, 2, 8])
    _same(_online(pool, got[rows], _dev(ctx, w["nonces"]["msg"][rows])), w["fused"], rows)
    pool.discard(got)
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP
    # ... and slots of the caller's choosing
    sess = _offline(ctx, w["gk"], B, S, w["dn"], sigset=w["ds"])
    assert np.array_equal(pool.deposit(sess, slots), slots)
    sess.close()
    # signed online in another order, in two subsets
    first, second = np.array([8, 1, 5, 0]), np.array([2, 7, 3, 6, 4])
    for rows in (first, second):
        _same(_online(pool, slots[rows], _dev(ctx, w["nonces"]["msg"][rows])), w["fused"], rows)
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pool.close()


def test_records_carry_their_sessions_party_mask_and_import_into_another_pool(world):
    from multi_party_ecdsa_amd import engine as E
    w = world
    ctx, B, S, n, t = w["ctx"], w["B"], w["S"], w["n"], w["t"]
    pool = E.PresigPool(ctx, w["gk"], list(range(S)), CAP)
    slots = np.array([(5 * i + 2) % CAP for i in range(B)], dtype=np.int32)
    sess = _offline(ctx, w["gk"], B, S, w["dn"], sigset=w["ds"])
    assert np.array_equal(pool.deposit(sess, slots), slots)
    sess.close()
    rec, st = pool.export(slots)
    assert not st.cpu().numpy().any()
    rec_np = _u32(rec)
    for b in range(B):
        u = PP.record_unpack([int(x) for x in rec_np[b]])
        assert u["mask"] == SC.party_mask(w["sets"][w["sigset"][b]]), b
        assert u["version"] == PP.RECORD_VERSION and u["L"] == S and u["local"][:S] == list(range(S)) and u["keyset"] == 0
        assert [p["k"] for p in u["parties"]] == [F.ints(w["nonces"]["k"][b * S + i:b * S + i + 1])[0] for i in range(S)]
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    # a second pool over the same many-set key object signs from the records what the session path signed
    other = E.PresigPool(ctx, w["gk"], list(range(S)), CAP)
    there = np.array([(3 * i + 1) % CAP for i in range(B)], dtype=np.int32)
    assert np.array_equal(other.import_(rec, there), there)
    order = np.array([4, 0, 8, 2, 6, 1, 7, 3, 5])
    _same(_online(other, there[order], _dev(ctx, w["nonces"]["msg"][order])), w["fused"], order)
    assert other.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    # a key object that lacks the record's set refuses it: 832, the slot stays EMPTY
    two = E.Gg20Keys(ctx, t, n, None, w["lks"][0]["arrays"], signer_sets=w["sets"][:2])
    narrow = E.PresigPool(ctx, two, list(range(S)), CAP)
    got = narrow.import_(rec, there)
    lacks = [w["sigset"][b] == 2 for b in range(B)]
    assert [int(x) for x in narrow.last_status] == [PP.IMPORT_REFUSED if l else 0 for l in lacks]
    assert [int(x) for x in got] == [-1 if l else int(there[b]) for b, l in enumerate(lacks)]
    keep = np.array([b for b in range(B) if not lacks[b]])
    _same(_online(narrow, there[keep], _dev(ctx, w["nonces"]["msg"][keep])), w["fused"], keep)
    assert narrow.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    for p in (pool, other, narrow):
        p.close()
    two.close()


def test_a_pool_over_a_one_set_object_writes_the_bytes_it_always_did(gpu_ctx, keys):
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, signers, B = gpu_ctx, 1, 3, [0, 2], 3
    S = len(signers)
    lk = G.make_local_keys(keys, t, n, signers)
    nonces = G.make_nonces(lk, B, seed="sigsets-presig-one-set")
    gk = E.Gg20Keys(ctx, t, n, signers, lk["arrays"])
    dn = {f: _dev(ctx, v) for f, v in nonces.items()}
    pool = E.PresigPool(ctx, gk, list(range(S)), CAP)
    sess = _offline(ctx, gk, B, S, dn)
    R = _u32(sess.result(signature=False)["R"])
    slots = np.array([9, 0, 15], dtype=np.int32)
    assert np.array_equal(pool.deposit(sess, slots), slots)
    sess.close()
    rec, st = pool.export(slots)
    assert not st.cpu().numpy().any()
    rec_np = _u32(rec)
    ref = PP.Pool(signers, list(range(S)), [lk["y"]], CAP)
    for b in range(B):
        words = [int(x) for x in rec_np[b]]
        u = PP.record_unpack(words)
        assert ref.record_ok(words) and u["mask"] == PP.signer_mask(signers)
        assert [p["R"] for p in u["parties"]] == [F.points(R[i][b:b + 1])[0] for i in range(S)]
        assert PP.record_pack(ref.mask, ref.local, 0, lk["y"], u["parties"]) == words
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pool.close()
    gk.close()
