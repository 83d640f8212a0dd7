#!/usr/bin/env python3
"""The online rate of GG20: what a caller with a message in hand waits for once the offline stage lies in a presignature pool.

    python tools/exp_presig.py [--out profiles/r10/presig.json] [--slots 65536] [--windows 7] [--calls 32] [--commit LABEL]

  offline    E.gg20_presign at (t, n) = (1, 3), signers [0, 2], both local: `slots` sessions through rounds 0-6 and into the pool, the
             nonces from the device sampler; timed once (after a warm-up batch of 1 024), for the offline / online ratio of one box.
  refill     The presignatures are exported ONCE; every timed call below is preceded by an UNTIMED mpe_gg20_presig_import of the same
             records into the same slots (for `complete`: import + sign).  Importing a record twice is the nonce reuse the slots exist to
             prevent — here on a throw-away key, to time 7 x 32 calls without 7 x 32 offline stages.
  sign       mpe_gg20_presig_sign over all `slots` slots, given as a fixed permutation.       items = slots (L partial signatures each)
  complete   mpe_gg20_presig_complete over the same slots.                                     items = L x slots verifications
  online     engine.gg20_sign_online = sign + complete + the status fold.                      items = slots signatures
  verify     mpe_ecdsa_verify on `slots` (key, message, signature) items: the same comb + GLV verification, the yardstick of `complete`.
  The four alternate inside one loop.  A call's time is the span between two device events around it; a window is the sum over `calls`
  calls; figures are medians of `windows` windows with min..max kept.  complete_over_verify = verifications/s of `complete` over
  items/s of `verify`: parity minus the slot gather and the S additions is expected, below 0.8 wants an explanation.

    python tools/exp_presig.py --stream [--out profiles/r12/presig_stream.json] [--batches 32] [--rounds 5] [--slots 65536] ...

  The stream form: one 3-set key object of a (1, 3) wallet, the sets round-robin over the sessions.
  offline    a stream of `batches` 1 024-session seeded batches at 4 lanes x 4 batches per group, wall time from the first submit to the
             last wait: through a PRESIG engine (submit_presig_seeded into the pool), through the SIGNING engine (submit_seeded_sets), as
             the Python loop (gg20_sample_nonces + gg20_presign per batch) and as the one C call per lone batch (gg20_presign_fused).
             The four alternate, `rounds` rounds, who goes first rotating; medians with min..max.  The pool is discarded between runs.
  online     PresigPool.sign_online (one launch) against engine.gg20_sign_online (sign + complete + the status fold) on the same
             imported records, `slots` slots, `windows` windows of `calls` calls, alternating inside one loop, an untimed import in front
             of every call."""
import argparse
import hashlib
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def figure(items, window_ms, calls):
    rates = [items * calls / (ms * 1e-3) for ms in window_ms]
    return dict(items_per_s=round(statistics.median(rates), 1), items_per_s_min=round(min(rates), 1), items_per_s_max=round(max(rates), 1),
                ms_per_call_median=round(statistics.median(window_ms) / calls, 4), items_per_call=items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--commit", default="unlabelled")
    a = ap.parse_args()
    if a.stream:
        return stream_main(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "r10", "presig.json")
    import numpy as np
    import torch
    import fixtures as F
    import gg20_fixture as G
    import ossl
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    signers = [0, 2]
    lk = G.make_local_keys(F.load_keys(), 1, 3, signers)
    gk = E.Gg20Keys(ctx, 1, 3, signers, lk["arrays"])
    S, B = 2, a.slots
    seed = hashlib.sha256(b"exp_presig").digest()
    pool = E.PresigPool(ctx, gk, [0, 1], B)

    def presign(count, counter):
        nonces, fail = E.gg20_sample_nonces(ctx, gk, count, seed, counter)
        got = E.gg20_presign(ctx, gk, nonces, count, pool)
        ctx.sync()
        assert int(fail.item()) == 0 and (got >= 0).all()
        return got

    warm = presign(min(B, 1024), 1)
    pool.discard(warm)
    ctx.sync()
    t0 = time.perf_counter()
    filled = presign(B, 2)
    t_offline = time.perf_counter() - t0
    assert sorted(filled.tolist()) == list(range(B))
    slots = torch.from_numpy(np.random.default_rng(1).permutation(B).astype(np.int32)).to(ctx.device)      # never arange
    rec, st = pool.export(slots)
    assert not st.any().item() and pool.audit()["stray"] == 0
    msg = E.sample_bits(ctx, B, seed, 99, 256, 8)
    status = torch.empty((B,), dtype=torch.int32, device=ctx.device)

    def refill():
        E.N_.check(E.N_.lib.mpe_gg20_presig_import(pool.h, B, E._ptr(slots), E._ptr(rec), E._ptr(status), ctx.stream()), "import")

    # what is timed signs: once through, checked by OpenSSL; its (r, s) are the yardstick's inputs
    refill()
    r, s, recid, st = E.gg20_sign_online(pool, slots, msg)
    ctx.sync()
    assert not st.any().item() and not status.any().item()
    npu = lambda t: t.cpu().numpy().view("uint32")
    chk = min(B, 512)
    assert ossl.ecdsa_verify(lk["arrays"]["y"][0], npu(msg)[:chk], npu(r)[:chk], npu(s)[:chk]).all()
    pub = torch.from_numpy(np.ascontiguousarray(np.repeat(lk["arrays"]["y"][:1], B, axis=0)).view(np.int32)).to(ctx.device)
    assert E.ecdsa_verify(ctx, pub, msg, r, s).all().item()
    pool._reap()

    def span(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        return e0, e1, out

    win = dict(sign=[], complete=[], online=[], verify=[])
    for _ in range(a.windows):
        ev = dict(sign=[], complete=[], online=[], verify=[])
        for _ in range(a.calls):
            refill()
            e0, e1, (s_i, _st) = span(lambda: pool.sign(slots, msg))
            ev["sign"].append((e0, e1))
            e0, e1, _o = span(lambda: pool.complete(slots, s_i))
            ev["complete"].append((e0, e1))
            refill()
            e0, e1, _o = span(lambda: E.gg20_sign_online(pool, slots, msg))
            ev["online"].append((e0, e1))
            e0, e1, _o = span(lambda: E.ecdsa_verify(ctx, pub, msg, r, s))
            ev["verify"].append((e0, e1))
            pool._pending.clear()                                              # the loop refills the same slots itself: no host free list here
        ctx.sync()
        for k, pairs in ev.items():
            win[k].append(sum(e0.elapsed_time(e1) for e0, e1 in pairs))
    assert pool.audit()["stray"] == 0
    res = dict(box="%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0)), commit=a.commit,
               shape="(t, n) = (1, 3), signers [0, 2], both local", slots=B, windows=a.windows, calls_per_window=a.calls,
               offline=dict(sessions=B, seconds=round(t_offline, 3), presignatures_per_s=round(B / t_offline, 1)),
               sign=figure(B, win["sign"], a.calls), complete=figure(S * B, win["complete"], a.calls),
               online=figure(B, win["online"], a.calls), verify=figure(B, win["verify"], a.calls))
    res["complete_over_verify"] = round(res["complete"]["items_per_s"] / res["verify"]["items_per_s"], 3)
    res["online_over_offline"] = round(res["online"]["items_per_s"] / res["offline"]["presignatures_per_s"], 1)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    pool.close()
    gk.close()


def spread(vals):
    return dict(median=round(statistics.median(vals), 1), min=round(min(vals), 1), max=round(max(vals), 1))


def stream_main(a):
    import numpy as np
    import torch
    import fixtures as F
    import ossl
    import sigset_cases as SC
    from multi_party_ecdsa_amd import engine as E
    out = a.out or os.path.join(ROOT, "profiles", "r12", "presig_stream.json")
    ctx = E.Context(0)
    t, n, S, PER, LANES, GROUP = 1, 3, 2, 1024, 4, 4
    sets = SC.all_sets(n, S)
    lks, _ = SC.wallet(F.load_keys(), t, n, sets)
    gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], signer_sets=sets)
    seed = hashlib.sha256(b"exp_presig_stream").digest()
    cap = max(a.slots, a.batches * PER)
    pool = E.PresigPool(ctx, gk, [0, 1], cap)
    ds = (torch.arange(PER, dtype=torch.int32, device=ctx.device) % len(sets)).contiguous()
    perm = torch.from_numpy(np.random.default_rng(1).permutation(cap).astype(np.int32)).to(ctx.device)      # never arange
    slot_of = [perm[b * PER:(b + 1) * PER].contiguous() for b in range(cap // PER)]
    msg = E.sample_bits(ctx, PER, seed, 99, 256, 8)
    counter = [1]

    def fresh():
        counter[0] += 1
        return counter[0]

    def empty_pool():
        pool.discard(perm)
        pool._reap()
        ctx.sync()
        assert pool.audit()["EMPTY"] == cap and pool.free_slots() == cap

    def run_presig_engine(nb, check=False):
        pipe = E.Gg20Pipeline(ctx, gk, PER, group=GROUP, lanes=LANES, pool=pool)
        ctx.sync()
        t0 = time.perf_counter()
        tk = [pipe.submit_presig_seeded(seed, fresh(), slots=slot_of[b], sigset=ds) for b in range(nb)]
        pipe.flush()
        res = [pipe.wait(x) for x in tk]
        dt = time.perf_counter() - t0
        assert all((u >= 0).all() for u, _ in res) and pipe.sampler_failures() == 0
        pipe.close()
        return dt

    def run_sign_engine(nb):
        pipe = E.Gg20Pipeline(ctx, gk, PER, group=GROUP, lanes=LANES)
        ctx.sync()
        t0 = time.perf_counter()
        tk = [pipe.submit_seeded(seed, fresh(), msg, sigset=ds) for b in range(nb)]
        pipe.flush()
        res = [pipe.wait(x) for x in tk]
        dt = time.perf_counter() - t0
        assert not any(r[3].any().item() for r in res)
        pipe.close()
        return dt

    def run_python_loop(nb):
        ctx.sync()
        t0 = time.perf_counter()
        for b in range(nb):
            z, _ = E.gg20_sample_nonces(ctx, gk, PER, seed, fresh(), sigset=ds)
            got = E.gg20_presign(ctx, gk, z, PER, pool, sigset=ds)
            assert (got >= 0).all()
        ctx.sync()
        return time.perf_counter() - t0

    def run_fused_lone(nb):
        ctx.sync()
        t0 = time.perf_counter()
        for b in range(nb):
            z, _ = E.gg20_sample_nonces(ctx, gk, PER, seed, fresh(), sigset=ds)
            got = E.gg20_presign_fused(ctx, gk, z, PER, pool, slots=slot_of[b], sigset=ds)
            assert (got >= 0).all()
        ctx.sync()
        return time.perf_counter() - t0

    runs = dict(presig_engine=run_presig_engine, sign_engine=run_sign_engine, python_loop=run_python_loop, fused_lone=run_fused_lone)
    for fn in runs.values():                                        # warm-up: allocations, workspaces, one group per lane
        fn(LANES * GROUP)
        empty_pool()
    names = list(runs)
    rate = {k: [] for k in names}
    for rnd in range(a.rounds):
        for k in names[rnd % len(names):] + names[:rnd % len(names)]:
            rate[k].append(a.batches * PER / runs[k](a.batches))
            empty_pool()
    offline = {k: spread(v) for k, v in rate.items()}
    offline["presig_over_sign_engine"] = round(offline["presig_engine"]["median"] / offline["sign_engine"]["median"], 4)
    offline["presig_engine_over_python_loop"] = round(offline["presig_engine"]["median"] / offline["python_loop"]["median"], 4)
    print(json.dumps(dict(offline=offline)), flush=True)

    # ---- online: the same records, imported in front of every timed call
    B = a.slots
    run_presig_engine(B // PER)
    slots = perm[:B].contiguous() if cap == B else torch.cat(slot_of[:B // PER])
    rec, st = pool.export(slots)
    assert not st.any().item() and pool.audit()["stray"] == 0
    pool._reap()
    msgs = E.sample_bits(ctx, B, seed, 98, 256, 8)
    status = torch.empty((B,), dtype=torch.int32, device=ctx.device)

    def refill():
        E.N_.check(E.N_.lib.mpe_gg20_presig_import(pool.h, B, E._ptr(slots), E._ptr(rec), E._ptr(status), ctx.stream()), "import")

    refill()
    r0, s0, c0, st0 = E.gg20_sign_online(pool, slots, msgs)
    refill()
    r1, s1, c1, st1 = pool.sign_online(slots, msgs)
    ctx.sync()
    assert not st0.any().item() and not st1.any().item() and not status.any().item()
    assert torch.equal(r0, r1) and torch.equal(s0, s1) and torch.equal(c0, c1)
    npu = lambda x: x.cpu().numpy().view("uint32")
    assert ossl.ecdsa_verify(lks[0]["arrays"]["y"][0], npu(msgs)[:512], npu(r1)[:512], npu(s1)[:512]).all()      # every set signs for the one wallet key
    pool._pending.clear()

    def span(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    win = dict(composed=[], fused=[])
    for _ in range(a.windows):
        ev = dict(composed=[], fused=[])
        for _ in range(a.calls):
            refill()
            ev["composed"].append(span(lambda: E.gg20_sign_online(pool, slots, msgs)))
            refill()
            ev["fused"].append(span(lambda: pool.sign_online(slots, msgs)))
            pool._pending.clear()
        ctx.sync()
        for k, pairs in ev.items():
            win[k].append(sum(e0.elapsed_time(e1) for e0, e1 in pairs))
    assert pool.audit() == dict(EMPTY=cap, READY=0, SIGNED=0, BUSY=0, stray=0)
    online = dict(composed=figure(B, win["composed"], a.calls), fused=figure(B, win["fused"], a.calls))
    online["fused_over_composed"] = round(online["fused"]["items_per_s"] / online["composed"]["items_per_s"], 4)
    online["fused_median_above_composed_range"] = online["fused"]["items_per_s"] > online["composed"]["items_per_s_max"]
    res = dict(box="%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0)), commit=a.commit,
               shape="(t, n) = (1, 3), one 3-set key object, sets round-robin, both signers local",
               offline_stream=dict(batch=PER, lanes=LANES, group=GROUP, batches_per_run=a.batches, rounds=a.rounds, sessions_per_s=offline),
               online=dict(slots=B, windows=a.windows, calls_per_window=a.calls, **online))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    pool.close()
    gk.close()


if __name__ == "__main__":
    main()
