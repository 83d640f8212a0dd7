"""GPU tests of the presignature pool (`mpe_gg20_presig_*`, engine.PresigPool): GG20's offline stage kept in single-use
device slots and signed online later.  The yardstick is the fused path — `Gg20Session` rounds 0-8 on the same nonces and
messages — whose (r, s, recid, status) and partial signatures the pool must reproduce byte for byte, at (t, n) = (1, 3)
with 67 sessions (one full wavefront and a tail of three) and at (2, 5) with 5, in a pool of 130 slots (three workgroups)
addressed through a fixed non-monotonic permutation with gaps.  OpenSSL re-checks the signatures; tests/pyref_presig.py is
the restatement of the slot states, the online arithmetic and the export record."""
import numpy as np
import pytest
import torch

import fixtures as F
import gg20_fixture as G
import pyref
import pyref_presig as PP

pytestmark = pytest.mark.gpu

CAP = 130
Q = pyref.Q


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _i32(t):
    return t.cpu().numpy()


def perm(count, mul=37, add=11):
    """`count` distinct slots of the pool, non-monotonic, with gaps (37 is a unit modulo 130)"""
    return np.array([(mul * i + add) % CAP for i in range(count)], dtype=np.int32)


def offline(ctx, gk, B, local, dn, keyset=None, upto=6, sess=None):
    """rounds 0..upto of a session with every signer local: an output [L, B, W] is the next round's input"""
    from multi_party_ecdsa_amd import engine as E
    if sess is None:
        sess = E.Gg20Session(ctx, gk, B, local, dn, keyset=keyset)
    prev = None
    for rnd in range(upto + 1):
        prev = sess.round(rnd, d_in=prev)
    return sess, prev


def fused(ctx, gk, B, S, dn, msg, keyset=None):
    """(a) of the issue: Gg20Session rounds 0-8; numpy r, s [S,B,8], recid, status [S,B], the partial signatures s_i [S,B,8], R [S,B,16]"""
    sess, _ = offline(ctx, gk, B, list(range(S)), dn, keyset=keyset)
    s_i = sess.round(7, msg=msg)
    sess.round(8, d_in=s_i)
    res = sess.result()
    ctx.sync()
    out = dict(r=_u32(res["r"]), s=_u32(res["s"]), recid=_i32(res["recid"]), status=_i32(res["status"]), s_i=_u32(s_i), R=_u32(res["R"]))
    sess.close()
    return out


class World:
    """one (t, n, signers, B) shape: keys, two sets of nonces on the device, the fused results of both (computed once, never changed)"""

    def __init__(self, ctx, keys, t, n, signers, B, tag):
        from multi_party_ecdsa_amd import engine as E
        self.ctx, self.t, self.n, self.signers, self.B, self.S = ctx, t, n, signers, B, len(signers)
        self.lk = G.make_local_keys(keys, t, n, signers)
        self.gk = E.Gg20Keys(ctx, t, n, signers, self.lk["arrays"])
        self.nonces = [G.make_nonces(self.lk, B, seed=f"presig-{tag}-{j}") for j in range(2)]
        self.dn = [{f: _dev(ctx, v) for f, v in z.items()} for z in self.nonces]
        self.msg = [z["msg"] for z in self.nonces]
        self.fused = [fused(ctx, self.gk, B, self.S, self.dn[j], self.dn[j]["msg"]) for j in range(2)]
        for f in self.fused:
            assert not f["status"].any()
        self.y = self.lk["arrays"]["y"][0]

    def pool(self, local=None, capacity=CAP):
        from multi_party_ecdsa_amd import engine as E
        return E.PresigPool(self.ctx, self.gk, list(range(self.S)) if local is None else local, capacity)

    def presign(self, pool, slots, j=0):
        """(b): a session through rounds 0-6 on nonce set j, deposited into `slots`; returns the usable slots"""
        sess, _ = offline(self.ctx, self.gk, self.B, list(range(self.S)), self.dn[j])
        got = pool.deposit(sess, slots)
        sess.close()
        return got


@pytest.fixture(scope="module")
def wa(gpu_ctx, keys):
    return World(gpu_ctx, keys, 1, 3, [0, 2], 67, "a")


@pytest.fixture(scope="module")
def wb(gpu_ctx, keys):
    return World(gpu_ctx, keys, 2, 5, [0, 2, 4], 5, "b")


@pytest.fixture(scope="module")
def records_a(wa):
    """the 67 presignatures of shape a, nonce set 0, as export records (tests that only need READY slots import them)"""
    pool = wa.pool()
    slots = perm(wa.B)
    assert np.array_equal(wa.presign(pool, slots), slots)
    rec, st = pool.export(slots)
    assert not _i32(st).any()
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pool.close()
    return rec


def ready_pool(wa, records_a, slots):
    pool = wa.pool()
    assert np.array_equal(pool.import_(records_a[:len(slots)], slots), slots)
    return pool


def online(pool, slots, d_msg):
    """sign + complete with every signer local; numpy dict"""
    s_i, st7 = pool.sign(slots, d_msg)
    res = pool.complete(slots, s_i)
    pool.ctx.sync()
    return dict(s_i=_u32(s_i), st7=_i32(st7), r=_u32(res["r"]), s=_u32(res["s"]), recid=_i32(res["recid"]), status=_i32(res["status"]))


def assert_same_as_fused(got, want, rows=None):
    rows = slice(None) if rows is None else rows
    assert not got["st7"].any() and not got["status"].any()
    for f in ("s_i", "r", "s", "recid"):
        assert np.array_equal(got[f], want[f][:, rows]), f


# ---- 1. the same bytes as the fused path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
def test_online_bytes_equal_the_fused_path(which, wa, wb):
    import ossl
    w = wa if which == "a" else wb
    pool = w.pool()
    slots = perm(w.B)
    assert np.array_equal(w.presign(pool, slots), slots) and not pool.last_status.any()
    assert pool.audit() == dict(EMPTY=CAP - w.B, READY=w.B, SIGNED=0, BUSY=0, stray=0)
    got = online(pool, slots, w.dn[0]["msg"])
    assert_same_as_fused(got, w.fused[0])
    for i in range(w.S):
        assert ossl.ecdsa_verify(w.y, w.msg[0], got["r"][i], got["s"][i]).all()
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pool.close()


def test_one_party_per_pool_two_pools_exchange_partial_signatures(wa):
    """L = 1 on each side of the two-signer session: two key objects that hold one party's secrets, two sessions, two pools"""
    from multi_party_ecdsa_amd import engine as E
    ctx, B = wa.ctx, wa.B
    gks = [E.Gg20Keys(ctx, wa.t, wa.n, wa.signers, wa.lk["arrays"], own=[wa.signers[i]]) for i in range(2)]
    sess = [E.Gg20Session(ctx, gks[i], B, [i], {f: _dev(ctx, v) for f, v in G.party_nonces(wa.nonces[0], wa.lk, i).items()}) for i in range(2)]
    prev = None
    for rnd in range(7):
        outs = [s.round(rnd, d_in=prev) for s in sess]
        prev = torch.cat(outs, 0) if outs[0] is not None else None
    pools = [E.PresigPool(ctx, gks[i], [i], CAP) for i in range(2)]
    slots = [perm(B), perm(B, mul=51, add=3)]
    for i in range(2):
        assert np.array_equal(pools[i].deposit(sess[i], slots[i]), slots[i])
    parts = [pools[i].sign(slots[i], wa.dn[0]["msg"]) for i in range(2)]
    d_in = torch.cat([p[0] for p in parts], 0)                           # the relay: both partial signatures, sender-major
    for i in range(2):
        res = pools[i].complete(slots[i], d_in)
        assert not _i32(parts[i][1]).any() and not _i32(res["status"]).any()
        assert np.array_equal(_u32(parts[i][0])[0], wa.fused[0]["s_i"][i])
        for f in ("r", "s"):
            assert np.array_equal(_u32(res[f])[0], wa.fused[0][f][i]), f
        assert np.array_equal(_i32(res["recid"])[0], wa.fused[0]["recid"][i])
        assert pools[i].audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    for o in sess + pools + gks:
        o.close()


# ---- 2. any order, any subset, any time ---------------------------------------------------------------------------------------
def test_any_order_any_subset_two_deposits_of_one_rearmed_session(wa):
    import ossl
    ctx, B, S = wa.ctx, wa.B, wa.S
    pool = wa.pool()
    first = perm(B)
    rest = np.array(sorted(set(range(CAP)) - set(first.tolist()))[::-1], dtype=np.int32)       # the 63 other slots, descending
    second = np.concatenate([rest, np.array([CAP, -1, 1 << 20, CAP + 7], dtype=np.int32)])      # 67 rows: four have nowhere to go
    sess, _ = offline(ctx, wa.gk, B, list(range(S)), wa.dn[0])
    R = [_u32(sess.result(signature=False)["R"])]
    assert np.array_equal(pool.deposit(sess, first), first)
    sess.rearm(wa.dn[1])
    offline(ctx, wa.gk, B, list(range(S)), wa.dn[1], sess=sess)
    R.append(_u32(sess.result(signature=False)["R"]))
    got2 = pool.deposit(sess, second)
    assert list(pool.last_status) == [0] * 63 + [PP.DEPOSIT_RANGE] * 4
    assert np.array_equal(got2, np.where((second >= 0) & (second < CAP), second, -1))
    sess.close()
    assert pool.audit() == dict(EMPTY=0, READY=CAP, SIGNED=0, BUSY=0, stray=0)
    where = {int(s): (0, b) for b, s in enumerate(first)}
    where.update({int(s): (1, b) for b, s in enumerate(rest)})
    rg = np.random.default_rng(20)
    order = rg.permutation(CAP).astype(np.int32)                          # slots of both deposits, mixed
    msgs = rg.integers(0, 2 ** 32, size=(CAP, 8), dtype=np.uint32)        # messages of their own, as round 7 takes them (any 256 bits)
    for part in (order[:40], order[40:]):
        rows = np.array([np.where(order == s)[0][0] for s in part])
        got = online(pool, part, _dev(ctx, msgs[rows]))
        assert not got["st7"].any() and not got["status"].any()
        for g, slot in enumerate(part):
            j, b = where[int(slot)]
            m = F.ints(msgs[rows[g]:rows[g] + 1])[0] % Q
            Rp = F.points(R[j][0][b:b + 1])[0]
            parts = [F.ints(got["s_i"][i][g:g + 1])[0] for i in range(S)]
            want = PP.output_signature(parts, m, Rp[0] % Q, Rp, wa.lk["y"])
            assert want[0] == 0
            for i in range(S):
                assert (F.ints(got["r"][i][g:g + 1])[0], F.ints(got["s"][i][g:g + 1])[0], int(got["recid"][i][g])) == want[1:]
        assert ossl.ecdsa_verify(wa.y, msgs[rows], got["r"][0], got["s"][0]).all()
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pool.close()


# ---- 3. single use ---------------------------------------------------------------------------------------------------------------
def test_a_signed_slot_does_not_sign_again(wa, records_a):
    slots = perm(wa.B, mul=7, add=5)
    pool = ready_pool(wa, records_a, slots)
    s1, st1 = pool.sign(slots, wa.dn[0]["msg"])
    s2, st2 = pool.sign(slots, wa.dn[0]["msg"])
    assert not _i32(st1).any() and np.array_equal(_u32(s1), wa.fused[0]["s_i"])
    assert list(_i32(st2)) == [PP.SIGN_NOT_READY] * wa.B and not _u32(s2).any()
    assert pool.audit() == dict(EMPTY=CAP - wa.B, READY=0, SIGNED=wa.B, BUSY=0, stray=0)
    pool.close()


def test_every_index_three_times_exactly_one_row_wins(wa, records_a):
    B = wa.B
    slots = perm(B, mul=9, add=1)
    pool = ready_pool(wa, records_a, slots)
    rows = np.random.default_rng(3).permutation(np.tile(np.arange(B), 3))          # row -> session; every session three times, scattered
    s_i, st = pool.sign(slots[rows], _dev(wa.ctx, wa.msg[0][rows]))
    s_i, st = _u32(s_i), _i32(st)
    assert set(st.tolist()) == {0, PP.SIGN_NOT_READY}
    for b in range(B):
        mine = np.where(rows == b)[0]
        won = mine[st[mine] == 0]
        assert len(won) == 1, b
        for i in range(wa.S):
            assert np.array_equal(s_i[i][won[0]], wa.fused[0]["s_i"][i][b])
            assert not s_i[i][mine[st[mine] != 0]].any()
    assert pool.audit() == dict(EMPTY=CAP - B, READY=0, SIGNED=B, BUSY=0, stray=0)
    winners = np.array([np.where((rows == b) & (st == 0))[0][0] for b in range(B)])
    res = pool.complete(slots, _dev(wa.ctx, s_i[:, winners]))
    assert not _i32(res["status"]).any() and np.array_equal(_u32(res["s"]), wa.fused[0]["s"]) and np.array_equal(_u32(res["r"]), wa.fused[0]["r"])
    pool.close()


def test_two_sign_calls_on_two_streams_one_winner_per_slot(wa, records_a):
    """the invariant holds under every interleaving of the two kernels; asserted once, no loop"""
    B, ctx = wa.B, wa.ctx
    slots = perm(B, mul=11, add=2)
    pool = ready_pool(wa, records_a, slots)
    d_slot = _dev(ctx, slots)
    ctx.sync()
    streams = [torch.cuda.Stream(device=ctx.device) for _ in range(2)]
    out = []
    for s in streams:                                                     # queued back to back, no synchronisation between the two
        with torch.cuda.stream(s):
            out.append(pool.sign(d_slot, wa.dn[0]["msg"]))
    for s in streams:
        s.synchronize()
    st = np.stack([_i32(o[1]) for o in out])
    assert ((st == 0).sum(axis=0) == 1).all() and set(st.ravel().tolist()) == {0, PP.SIGN_NOT_READY}
    s_i = np.stack([_u32(o[0]) for o in out])                             # [call, S, B, 8]
    for c in range(2):
        assert np.array_equal(s_i[c][:, st[c] == 0], wa.fused[0]["s_i"][:, st[c] == 0]) and not s_i[c][:, st[c] != 0].any()
    assert pool.audit() == dict(EMPTY=CAP - B, READY=0, SIGNED=B, BUSY=0, stray=0)
    pool.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_deposit_into_a_ready_slot_is_refused_and_the_first_content_signs(wa):
    pool = wa.pool()
    slots = perm(wa.B)
    assert np.array_equal(wa.presign(pool, slots, 0), slots)
    assert list(wa.presign(pool, slots, 1)) == [-1] * wa.B and list(pool.last_status) == [PP.DEPOSIT_NOT_EMPTY] * wa.B
    assert pool.audit() == dict(EMPTY=CAP - wa.B, READY=wa.B, SIGNED=0, BUSY=0, stray=0)
    assert_same_as_fused(online(pool, slots, wa.dn[0]["msg"]), wa.fused[0])
    pool.close()


def test_out_of_range_slots_and_wrong_states(wa, records_a):
    B, ctx = 8, wa.ctx
    slots = perm(B)
    pool = ready_pool(wa, records_a, slots)
    far = np.array([CAP, -1, 1 << 30, -(1 << 31), CAP + 1, 131, 4096, -2], dtype=np.int32)
    s_i, st = pool.sign(far, wa.dn[0]["msg"][:B])
    assert list(_i32(st)) == [PP.SIGN_RANGE] * B and not _u32(s_i).any()
    res = pool.complete(far, s_i)
    assert (_i32(res["status"]) == PP.COMPLETE_RANGE).all()
    rec, st = pool.export(far)
    assert list(_i32(st)) == [PP.RECORD_RANGE] * B and not _u32(rec).any()
    assert list(pool.import_(records_a[:B], far)) == [-1] * B and list(pool.last_status) == [PP.RECORD_RANGE] * B
    pool.discard(far)
    # complete on READY slots: 822, outputs zero, the slots still sign
    res = pool.complete(slots, _dev(ctx, wa.fused[0]["s_i"][:, :B]))
    assert (_i32(res["status"]) == PP.COMPLETE_NOT_SIGNED).all() and not _u32(res["r"]).any() and not _u32(res["s"]).any()
    assert pool.audit() == dict(EMPTY=CAP - B, READY=B, SIGNED=0, BUSY=0, stray=0)
    # a doubled s_i of signer 1 among d_in (the reference's step-7 corruption): 701 where it is read, and a freed slot
    s_i, st = pool.sign(slots, wa.dn[0]["msg"][:B])
    bad = _u32(s_i).copy()
    bad[1] = F.words([2 * v % Q for v in F.ints(bad[1])], 8)
    res = pool.complete(slots, _dev(ctx, bad))
    st = _i32(res["status"])
    assert list(st[0]) == [PP.VERIFY_FAILED] * B and not _u32(res["r"])[0].any() and not _u32(res["s"])[0].any() and not _i32(res["recid"])[0].any()
    assert list(st[1]) == [0] * B and np.array_equal(_u32(res["s"])[1], wa.fused[0]["s"][1][:B])       # party 1 takes its OWN s_i from the slot
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pool.close()


def test_a_failed_session_deposits_as_803(wb):
    from multi_party_ecdsa_amd import engine as E
    ctx, B, S = wb.ctx, wb.B, wb.S
    pool = wb.pool()
    sess = E.Gg20Session(ctx, wb.gk, B, list(range(S)), wb.dn[0])
    sess.fault_inject(5, 0b010)                                           # signer 1 doubles its delta_i: phase5_check_R_dash_sum fails
    offline(ctx, wb.gk, B, list(range(S)), wb.dn[0], sess=sess)
    assert list(pool.deposit(sess, perm(B))) == [-1] * B and list(pool.last_status) == [PP.SESSION_FAILED] * B
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP
    assert (_i32(sess.result(signature=False)["status"]) == 502).all()    # what it failed with stays readable
    sess.close()
    pool.close()


def test_deposit_before_round_6_is_an_argument_error_and_leaves_the_session_alone(wb):
    from multi_party_ecdsa_amd import _native as N
    ctx, B, S = wb.ctx, wb.B, wb.S
    pool = wb.pool()
    sess, m5 = offline(ctx, wb.gk, B, list(range(S)), wb.dn[0], upto=5)
    with pytest.raises(N.MpeError, match="rc=-1"):
        pool.deposit(sess, perm(B))
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP
    sess.round(6, d_in=m5)
    s_i = sess.round(7, msg=wb.dn[0]["msg"])
    with pytest.raises(N.MpeError, match="rc=-1"):                        # behind round 7 is too late as well
        pool.deposit(sess, perm(B))
    sess.round(8, d_in=s_i)
    res = sess.result()
    assert np.array_equal(_u32(s_i), wb.fused[0]["s_i"]) and not _i32(res["status"]).any()
    for f in ("r", "s"):
        assert np.array_equal(_u32(res[f]), wb.fused[0][f]), f
    assert np.array_equal(_i32(res["recid"]), wb.fused[0]["recid"])
    other = wb.pool(local=[0, 1])                                         # another set of local parties than the session's
    sess.rearm(wb.dn[1])
    offline(ctx, wb.gk, B, list(range(S)), wb.dn[1], sess=sess)
    with pytest.raises(N.MpeError, match="rc=-1"):
        other.deposit(sess, perm(B))
    assert np.array_equal(pool.deposit(sess, perm(B)), perm(B))           # ... and untouched by the refusal: it still deposits
    assert_same_as_fused(online(pool, perm(B), wb.dn[1]["msg"]), wb.fused[1])
    for o in (sess, pool, other):
        o.close()


# ---- 5. the session after a deposit --------------------------------------------------------------------------------------------
def test_session_after_a_deposit_refuses_rounds_and_rearms(wb):
    from multi_party_ecdsa_amd import _native as N
    ctx, B, S = wb.ctx, wb.B, wb.S
    pool = wb.pool()
    sess, _ = offline(ctx, wb.gk, B, list(range(S)), wb.dn[0])
    assert np.array_equal(pool.deposit(sess, perm(B)), perm(B))
    out = torch.zeros((S, B, 8), dtype=torch.int32, device=ctx.device)
    with pytest.raises(N.MpeError):
        sess.round(7, msg=wb.dn[0]["msg"], out=out)
    with pytest.raises(N.MpeError):
        sess.round(0)
    with pytest.raises(N.MpeError):
        pool.deposit(sess, perm(B, add=12))
    assert not _u32(out).any()
    sess.rearm(wb.dn[1])
    offline(ctx, wb.gk, B, list(range(S)), wb.dn[1], sess=sess)
    s_i = sess.round(7, msg=wb.dn[1]["msg"])
    sess.round(8, d_in=s_i)
    res = sess.result()
    assert not _i32(res["status"]).any() and np.array_equal(_u32(s_i), wb.fused[1]["s_i"])
    for f in ("r", "s"):
        assert np.array_equal(_u32(res[f]), wb.fused[1][f]), f
    assert np.array_equal(_i32(res["recid"]), wb.fused[1]["recid"])
    assert_same_as_fused(online(pool, perm(B), wb.dn[0]["msg"]), wb.fused[0])          # the earlier presignatures waited meanwhile
    sess.close()
    pool.close()


# ---- 6. export / import ------------------------------------------------------------------------------------------------------------
def test_export_import_round_trip_and_tampered_records(wa):
    ctx, B = wa.ctx, wa.B
    pool = wa.pool()
    slots = perm(B)
    sess, _ = offline(ctx, wa.gk, B, list(range(wa.S)), wa.dn[0])
    R = _u32(sess.result(signature=False)["R"])
    assert np.array_equal(pool.deposit(sess, slots), slots)
    sess.close()
    rows = np.array([5, 66, 0, 64, 17, 63, 2, 40, 65, 31])                # ten sessions, both sides of the wavefront boundary
    rec, st = pool.export(slots[rows])
    assert not _i32(st).any() and pool.audit() == dict(EMPTY=CAP - B + 10, READY=B - 10, SIGNED=0, BUSY=0, stray=0)
    assert pool.free_slots() == CAP - B + 10
    again, st = pool.export(slots[rows])
    assert list(_i32(st)) == [PP.EXPORT_NOT_READY] * 10 and not _u32(again).any()
    rec_np = _u32(rec)
    assert rec_np.shape == (10, 28 + 32 * wa.S) == (10, pool.record_words)
    ref = PP.Pool(wa.signers, list(range(wa.S)), [wa.lk["y"]], CAP)
    for g, b in enumerate(rows):
        u = PP.record_unpack([int(x) for x in rec_np[g]])
        assert ref.record_ok([int(x) for x in rec_np[g]])
        assert [p["R"] for p in u["parties"]] == [F.points(R[i][b:b + 1])[0] for i in range(wa.S)]
        assert [p["k"] for p in u["parties"]] == [F.ints(wa.nonces[0]["k"][b * wa.S + i:b * wa.S + i + 1])[0] for i in range(wa.S)]
        assert PP.record_pack(ref.mask, ref.local, 0, wa.lk["y"], u["parties"]) == [int(x) for x in rec_np[g]]
        # the restatement signs from the record what the fused path signed
        assert ref.import_(int(slots[b]), [int(x) for x in rec_np[g]]) == 0
        code, s_i = ref.sign(int(slots[b]), F.ints(wa.msg[0][b:b + 1])[0])
        assert code == 0 and s_i == [F.ints(wa.fused[0]["s_i"][i][b:b + 1])[0] for i in range(wa.S)]
    # into another pool of the same keys, at other indices
    other = wa.pool()
    there = perm(10, mul=29, add=100)
    assert np.array_equal(other.import_(rec, there), there)
    assert list(other.import_(rec, there)) == [-1] * 10 and list(other.last_status) == [PP.IMPORT_NOT_EMPTY] * 10
    assert_same_as_fused(online(other, there, _dev(ctx, wa.msg[0][rows])), wa.fused[0], rows)
    # tampered records: 832 each, the slot stays EMPTY
    q8 = F.words([Q], 8)[0]
    t = np.repeat(rec_np[:1], 8, axis=0).copy()
    t[0, 12] ^= 1                                                         # wrong y
    t[1, 1] = 0b011                                                       # wrong signer-set mask
    t[2, 28:36] = 0                                                       # k_i = 0
    t[3, 28 + 32:36 + 32] = q8                                            # k_i = q (the second party's)
    t[4, 28 + 16] ^= 1                                                    # R off the curve
    t[5, 0] = 2                                                           # another version
    t[6, 4] = 0                                                           # other ordinals
    t[7, 36:44] = q8                                                      # sigma_i = q
    for g in range(8):
        assert not ref.record_ok([int(x) for x in t[g]]), g
    spot = perm(8, mul=3, add=50)
    assert list(other.import_(_dev(ctx, t), spot)) == [-1] * 8 and list(other.last_status) == [PP.IMPORT_REFUSED] * 8
    assert other.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0) and other.free_slots() == CAP
    pool.close()
    other.close()


def test_two_key_sets_a_slot_signs_under_its_own_y(gpu_ctx, keys):
    import ossl
    from multi_party_ecdsa_amd import engine as E
    K, t, n, signers, B = 2, 1, 3, [0, 1], 6
    lks = [G.make_local_keys(keys[kk:] + keys[:kk], t, n, signers, seed=f"presig-wallet-{kk}") for kk in range(K)]
    arrays = {f: np.concatenate([lk["arrays"][f] for lk in lks]) for f in ("x", "p", "q", "Nt", "h1", "h2", "y", "X")}
    keyset = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    parts = [G.make_nonces(lks[int(keyset[b])], 1, seed=f"presig-mw-{b}") for b in range(B)]
    nonces = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
    gk = E.Gg20Keys(gpu_ctx, t, n, signers, arrays, nkeysets=K)
    dn = {f: _dev(gpu_ctx, v) for f, v in nonces.items()}
    d_ks = torch.from_numpy(keyset).to(gpu_ctx.device)
    want = fused(gpu_ctx, gk, B, 2, dn, dn["msg"], keyset=d_ks)
    pool = E.PresigPool(gpu_ctx, gk, [0, 1], CAP)
    slots = E.gg20_presign(gpu_ctx, gk, dn, B, pool, keyset=d_ks)
    assert list(slots) == list(range(B))                                  # the free list's choice
    order = np.array([4, 0, 5, 2, 1, 3])
    r, s, recid, status = E.gg20_sign_online(pool, slots[order], dn["msg"][torch.from_numpy(order).to(gpu_ctx.device)])
    assert not _i32(status).any()
    assert np.array_equal(_u32(r), want["r"][0][order]) and np.array_equal(_u32(s), want["s"][0][order]) and np.array_equal(_i32(recid), want["recid"][0][order])
    for g, b in enumerate(order):
        y = lks[int(keyset[b])]["arrays"]["y"][0]
        assert ossl.ecdsa_verify(y, nonces["msg"][b:b + 1], _u32(r)[g:g + 1], _u32(s)[g:g + 1]).all()
        assert not ossl.ecdsa_verify(lks[1 - int(keyset[b])]["arrays"]["y"][0], nonces["msg"][b:b + 1], _u32(r)[g:g + 1], _u32(s)[g:g + 1]).any()
    assert pool.free_slots() == CAP
    # the record names the slot's key set and carries that key set's y
    slots = E.gg20_presign(gpu_ctx, gk, dn, B, pool, keyset=d_ks)
    rec = _u32(pool.export(slots)[0])
    assert list(rec[:, 11]) == list(keyset) and all(np.array_equal(rec[b, 12:28], arrays["y"][keyset[b]]) for b in range(B))
    pool.close()
    gk.close()


# ---- 7. hygiene ------------------------------------------------------------------------------------------------------------------------
def test_no_stray_secret_words_and_clean_scratch(keys):
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    t, n, signers, B = 1, 3, [0, 2], 9
    lk = G.make_local_keys(keys, t, n, signers)
    gk = E.Gg20Keys(ctx, t, n, signers, lk["arrays"])
    dn = [{f: _dev(ctx, v) for f, v in G.make_nonces(lk, B, seed=f"presig-hygiene-{j}").items()} for j in range(2)]
    ctx.wipe()
    before = ctx.scratch_audit()[0]
    pool = E.PresigPool(ctx, gk, [0, 1], CAP)
    slots = E.gg20_presign(ctx, gk, dn[0], B, pool)
    assert (slots >= 0).all() and pool.audit() == dict(EMPTY=CAP - B, READY=B, SIGNED=0, BUSY=0, stray=0)
    assert ctx.scratch_audit()[0] == before                               # the session arena, the workspace, the tables: as before
    s_i, st = pool.sign(slots[:3], dn[0]["msg"][:3])                      # sign: k_i, sigma_i leave the slot in the same kernel
    assert pool.audit() == dict(EMPTY=CAP - B, READY=B - 3, SIGNED=3, BUSY=0, stray=0)
    pool.discard(slots[2:5])                                              # a SIGNED slot and two READY ones
    assert pool.audit() == dict(EMPTY=CAP - B + 3, READY=B - 5, SIGNED=2, BUSY=0, stray=0) and pool.free_slots() == CAP - B + 3
    rec, st = pool.export(slots[5:7])
    assert not _i32(st).any() and pool.audit() == dict(EMPTY=CAP - B + 5, READY=B - 7, SIGNED=2, BUSY=0, stray=0)
    # failed deposits: into the READY slots (802), out of range (801)
    sess, _ = offline(ctx, gk, B, [0, 1], dn[1])
    pool.deposit(sess, np.concatenate([slots[7:9], slots[7:9], np.full(B - 4, CAP, dtype=np.int32)]))
    sess.close()
    ctx.wipe()
    assert list(pool.last_status) == [PP.DEPOSIT_NOT_EMPTY] * 4 + [PP.DEPOSIT_RANGE] * (B - 4)
    assert pool.audit() == dict(EMPTY=CAP - B + 5, READY=B - 7, SIGNED=2, BUSY=0, stray=0)
    assert ctx.scratch_audit()[0] == before
    pool.close()
    pool = E.PresigPool(ctx, gk, [0, 1], CAP)                             # close()-then-recreate: nothing of the old pool shows
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP
    pool.close()
    gk.close()
    ctx.close()
