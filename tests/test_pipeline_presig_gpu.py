"""GPU: the pipelined engine fills the presignature pool (mpe_gg20_pipeline_create_presig / submit_presig / submit_presig_seeded) and
takes a signer set per session (submit_sets / submit_seeded_sets).  A stream of offline stages, whatever the grouping, the lanes and the
order of waiting, followed by the online step with messages chosen afterwards gives what the oracle signs from the same nonces and
messages; a failed pass is every ticket's news and leaves its slots EMPTY."""
import hashlib

import numpy as np
import pytest
import torch

import fixtures as F
import gg20_fixture as G
import sigset_cases as SC
from multi_party_ecdsa_amd import engine as E

pytestmark = pytest.mark.gpu
SEED = hashlib.sha256(b"pipeline-presig").digest()
CAP = 32


def dv(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(ctx.device)


def hv(t):
    return t.cpu().numpy().view(np.uint32)


def messages(tag, B):
    return F.words([int.from_bytes(hashlib.sha256(b"%s %d" % (tag, i)).digest(), "big") for i in range(B)], 8)


@pytest.fixture(scope="module")
def wallet(gpu_ctx):
    lk = G.make_local_keys(F.load_keys(), 1, 3, [0, 1])
    gk = E.Gg20Keys(gpu_ctx, 1, 3, [0, 1], lk["arrays"])
    yield lk, gk
    gk.close()


@pytest.fixture(scope="module")
def setworld(gpu_ctx, keys):
    sets = SC.all_sets(3, 2)
    lks, per_wallet = SC.wallet(keys, 1, 3, sets)
    gk = E.Gg20Keys(gpu_ctx, 1, 3, None, lks[0]["arrays"], signer_sets=sets)
    yield lks, per_wallet, gk
    gk.close()


def signs_like_the_oracle(ctx, pool, slots, msg, want):
    r, s, recid, status = pool.sign_online(slots, dv(ctx, msg))
    wr, ws, wrecid = want
    assert not status.cpu().numpy().any()
    assert np.array_equal(hv(r), wr) and np.array_equal(hv(s), ws) and np.array_equal(recid.cpu().numpy(), wrecid)


@pytest.mark.parametrize("group,lanes,nb", [(3, 2, 5), (1, 1, 2)])
def test_stream_of_offline_stages_then_online_equals_the_oracle(gpu_ctx, wallet, group, lanes, nb):
    ctx = gpu_ctx
    lk, gk = wallet
    B = 6
    host = [G.make_nonces(lk, B, seed="pp-%d" % b) for b in range(nb)]
    dev = [{f: dv(ctx, v) for f, v in h.items() if f != "msg"} for h in host]
    slots = [np.array([(11 * (b * B + i) + 5) % CAP for i in range(B)], dtype=np.int32) for b in range(nb)]     # spread over the pool
    pool = E.PresigPool(ctx, gk, [0, 1], CAP)
    pipe = E.Gg20Pipeline(ctx, gk, B, group=group, lanes=lanes, pool=pool)
    tickets = [pipe.submit_presig(dev[b], slots=slots[b]) for b in range(nb)]
    assert tickets == list(range(1, nb + 1)) and pool.free_slots() == CAP - nb * B
    # waiting in reverse order: the last ticket sits in a partly filled group that wait() must flush
    for b in reversed(range(nb)):
        usable, status = pipe.wait(tickets[b])
        assert pipe.done(tickets[b]) and not status.cpu().numpy().any() and np.array_equal(usable, slots[b])
    assert pool.audit() == dict(EMPTY=CAP - nb * B, READY=nb * B, SIGNED=0, BUSY=0, stray=0)
    # the messages arrive now
    for b in (nb - 1, 0) + tuple(range(1, nb - 1)):
        host[b]["msg"] = messages(b"late %d" % b, B)
        wr, ws, wrecid, _, wstatus = G.oracle_sign(lk, host[b], B)
        assert not wstatus.any()
        signs_like_the_oracle(ctx, pool, slots[b], host[b]["msg"], (wr, ws, wrecid))
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP
    pipe.close()
    pool.close()


def test_seeded_stream_with_mixed_sets_equals_the_oracle_expanding_the_same_seed(gpu_ctx, setworld):
    """row b of a mixed draw is row b of the uniform draw with that session's set (tests/test_sigsets_sample_gpu.py): the expectation takes
    row b from the oracle's expansion of (seed, counter) under the fixture of b's set"""
    ctx = gpu_ctx
    lks, _, gk = setworld
    B, nb = 5, 4
    sigsets = [[0, 1, 2, 2, 0], [1, 1, 2, 0, 2], [2, 0, 1, 1, 0], [0, 0, 2, 1, 2]]
    pool = E.PresigPool(ctx, gk, [0, 1], CAP)
    pipe = E.Gg20Pipeline(ctx, gk, B, group=2, lanes=2, pool=pool)
    tickets = [pipe.submit_presig_seeded(SEED, 2000 + b, sigset=torch.tensor(sigsets[b], dtype=torch.int32, device=ctx.device)) for b in range(nb)]
    pipe.flush()
    got = [pipe.wait(t) for t in tickets]
    assert pipe.sampler_failures() == 0
    for b in range(nb):
        usable, status = got[b]
        assert not status.cpu().numpy().any() and list(usable) == list(range(b * B, (b + 1) * B))      # the pool's free list, in order
        drawn = {}
        for k in sorted(set(sigsets[b])):
            drawn[k], fails = G.oracle_sample_nonces(lks[k], B, SEED, 2000 + b)
            assert fails == 0
        z = {}
        for f, a in drawn[sigsets[b][0]].items():
            per = a.shape[0] // B
            z[f] = np.ascontiguousarray(np.concatenate([drawn[sigsets[b][i]][f][i * per:(i + 1) * per] for i in range(B)]))
        z["msg"] = messages(b"seeded %d" % b, B)
        res = SC.oracle_mixed(lks, z, sigsets[b])
        assert not res["status"].any()
        signs_like_the_oracle(ctx, pool, usable, z["msg"], (res["r"], res["s"], res["recid"]))
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pipe.close()
    pool.close()


def test_a_failed_pass_leaves_its_slots_empty_and_the_next_group_deposits(gpu_ctx, wallet):
    ctx = gpu_ctx
    lk, gk = wallet
    B, group = 4, 2
    pool = E.PresigPool(ctx, gk, [0, 1], CAP)
    pipe = E.Gg20Pipeline(ctx, gk, B, group=group, lanes=2, pool=pool)
    rc = E.N_.MPE_E_NOMEM
    pipe.inject_fault(1, rc)
    tickets = [pipe.submit_presig_seeded(SEED, 700 + b) for b in range(2 * group)]               # no submit raises
    assert pool.free_slots() == CAP - 2 * group * B
    usable = {}
    for b, t in enumerate(tickets):
        failed = b < group
        assert pipe.ticket_rc(t) == (True, rc if failed else 0)
        if failed:
            status = pipe._keep[t][5]
            with pytest.raises(E.N_.MpeError):
                pipe.wait(t)
            assert pipe.done(t) and (status.cpu().numpy() == E.N_.gg20_status_pass_failed(rc)).all()
        else:
            usable[b], status = pipe.wait(t)
            assert not status.cpu().numpy().any() and list(usable[b]) == list(range(b * B, (b + 1) * B))
    assert pipe.counters()["failed"] == 1 and pipe.counters()["groups"] == 2
    # the failed group's slots never left EMPTY and are the free list's again; the next group's are READY
    assert pool.audit() == dict(EMPTY=CAP - group * B, READY=group * B, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP - group * B
    assert list(pool.sign_online(list(range(group * B)), dv(ctx, messages(b"none", group * B)))[3].cpu().numpy()) == [812] * (group * B)
    for b in range(group, 2 * group):
        msg = messages(b"after %d" % b, B)
        z, fails = G.oracle_sample_nonces(lk, B, SEED, 700 + b, msg=msg)
        wr, ws, wrecid, _, wstatus = G.oracle_sign(lk, z, B)
        assert fails == 0 and not wstatus.any()
        signs_like_the_oracle(ctx, pool, usable[b], msg, (wr, ws, wrecid))
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP
    pipe.close()
    pool.close()


def test_the_signing_engine_takes_a_signer_set_per_session(gpu_ctx, setworld):
    """one group of two batches: the first names its sets (mixed, one index out of range), the second does not (set 0); both equal
    mpe_gg20_sign_sets on the same arrays, and the out-of-range row alone gets 92"""
    ctx = gpu_ctx
    lks, per_wallet, gk = setworld
    B = 5
    sigset = [2, 0, 1, 7, 1]
    host = [SC.mixed_nonces(per_wallet, [2, 0, 1, 0, 1], seed="pipe-sets"), SC.mixed_nonces(per_wallet, [0] * B, seed="pipe-plain")]
    dev = [{f: dv(ctx, v) for f, v in h.items()} for h in host]
    ds = torch.tensor(sigset, dtype=torch.int32, device=ctx.device)
    pipe = E.Gg20Pipeline(ctx, gk, B, group=2, lanes=1)
    t1, t2 = pipe.submit(dev[0], sigset=ds), pipe.submit(dev[1])
    for t, d, ss in ((t1, dev[0], ds), (t2, dev[1], None)):
        r, s, recid, status = pipe.wait(t)
        r1, s1, recid1, status1 = E.gg20_sign(ctx, gk, d, B, sigset=ss)
        ctx.sync()
        assert np.array_equal(status.cpu().numpy(), status1.cpu().numpy()) and np.array_equal(hv(r), hv(r1)) and np.array_equal(hv(s), hv(s1))
        assert np.array_equal(recid.cpu().numpy(), recid1.cpu().numpy())
        assert list(status.cpu().numpy()) == ([0, 0, 0, SC.BAD_SET, 0] if ss is not None else [0] * B) and hv(r)[0].any()
    # ... and the seeded form draws with the sets: equal to signing the sampler's own mixed draw
    good = torch.tensor([1, 2, 0, 2, 1], dtype=torch.int32, device=ctx.device)
    msg = dv(ctx, messages(b"sets seeded", B))
    t3 = pipe.submit_seeded(SEED, 4100, msg, sigset=good)
    r, s, recid, status = pipe.wait(t3)
    z, fail = E.gg20_sample_nonces(ctx, gk, B, SEED, 4100, msg=msg, sigset=good)
    r1, s1, recid1, status1 = E.gg20_sign(ctx, gk, z, B, sigset=good)
    ctx.sync()
    assert int(fail.item()) == 0 and not status.cpu().numpy().any() and not status1.cpu().numpy().any()
    assert np.array_equal(hv(r), hv(r1)) and np.array_equal(hv(s), hv(s1)) and np.array_equal(recid.cpu().numpy(), recid1.cpu().numpy())
    pipe.close()


def test_the_wrong_kind_of_submission_takes_no_slot_and_no_ticket(gpu_ctx, wallet):
    """the check of test_a_refused_submission_takes_no_slot_and_no_ticket for the two kinds of engine: the refused calls leave the ticket
    counter and the open group as they were"""
    ctx = gpu_ctx
    lk, gk = wallet
    B = 4
    host = G.make_nonces(lk, B, seed="wrong-kind")
    dev = {f: dv(ctx, v) for f, v in host.items()}
    msg = messages(b"wrong kind", B)
    pool = E.PresigPool(ctx, gk, [0, 1], CAP)
    pre = E.Gg20Pipeline(ctx, gk, B, group=3, lanes=1, pool=pool)
    t1 = pre.submit_presig_seeded(SEED, 31)
    for _ in range(2):
        with pytest.raises(E.N_.MpeError):
            pre.submit(dev)
        with pytest.raises(E.N_.MpeError):
            pre.submit_seeded(SEED, 32, dv(ctx, msg))
    t2 = pre.submit_presig_seeded(SEED, 33)
    assert (t1, t2) == (1, 2) and pool.free_slots() == CAP - 2 * B
    for c, t in ((31, t1), (33, t2)):
        usable, status = pre.wait(t)
        z, fails = G.oracle_sample_nonces(lk, B, SEED, c, msg=msg)
        wr, ws, wrecid, _, wstatus = G.oracle_sign(lk, z, B)
        assert fails == 0 and not wstatus.any() and not status.cpu().numpy().any()
        signs_like_the_oracle(ctx, pool, usable, msg, (wr, ws, wrecid))
    assert pre.counters()["groups"] == 1
    # ... and the reverse: a presig submission to a signing engine
    import ctypes as C
    sign = E.Gg20Pipeline(ctx, gk, B, group=3, lanes=1)
    t1 = sign.submit(dev)
    d_slot, d_status, tk = torch.arange(B, dtype=torch.int32, device=ctx.device), torch.zeros(B, dtype=torch.int32, device=ctx.device), C.c_uint64(0)
    nn = E._struct(E.N_.Gg20Nonces, dev)
    for _ in range(2):                                              # (the harness refuses by itself without pool=: the C calls)
        with pytest.raises(E.N_.MpeError):
            sign.submit_presig(dev)
        assert E.N_.lib.mpe_gg20_pipeline_submit_presig(sign.h, None, None, C.byref(nn), d_slot.data_ptr(), d_status.data_ptr(), ctx.stream(),
                                                        C.byref(tk)) == E.N_.MPE_E_ARG
        assert E.N_.lib.mpe_gg20_pipeline_submit_presig_seeded(sign.h, None, None, SEED, 34, d_slot.data_ptr(), d_status.data_ptr(), ctx.stream(),
                                                               C.byref(tk)) == E.N_.MPE_E_ARG
    assert tk.value == 0
    t2 = sign.submit(dev)
    assert (t1, t2) == (1, 2) and pool.free_slots() == CAP and pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    wr, ws, wrecid, _, wstatus = G.oracle_sign(lk, host, B)
    for t in (t1, t2):
        r, s, recid, status = sign.wait(t)
        assert not wstatus.any() and not status.cpu().numpy().any() and np.array_equal(hv(r), wr) and np.array_equal(hv(s), ws)
    assert sign.counters()["groups"] == 1
    sign.close()
    pre.close()
    pool.close()
