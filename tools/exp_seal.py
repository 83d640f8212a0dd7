#!/usr/bin/env python3
"""What sealing costs: sealed presignature export / import against the plain calls of the same run, and the generic seal rate.

    python tools/exp_seal.py [--out profiles/r13/seal.json] [--slots 65536] [--windows 7] [--calls 16] [--commit LABEL]

  records    (t, n) = (1, 3), signers [0, 2], both local: `slots` presignatures made once (gg20_presign, nonces from the device
             sampler) and exported.  The four calls then alternate inside one loop over the same slots, given as a fixed permutation —
             import (plain records) -> export -> import_sealed (the sealed rows of the previous round) -> export_sealed (a fresh
             nonce_hi) — so every call finds the slots in the state it needs and nothing untimed runs in between.  Importing a record
             again is the nonce reuse the slots exist to prevent: here on a throw-away key, to time the calls without an offline stage
             per call.
  rows       mpe_seal and mpe_unseal on `slots` caller rows of 72 words (a key share's size) and of 1 024 words, alternating.
  A call's time is the span between two device events around it; a window is the sum over `calls` calls; figures are medians of
  `windows` windows with min..max kept (DESIGN §14's protocol).  The plain calls of the same run are the baseline: the ratios
  sealed / plain are what DESIGN §17 reports.  No test asserts a rate."""
import argparse
import hashlib
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def figure(items, window_ms, calls):
    rates = [items * calls / (ms * 1e-3) for ms in window_ms]
    return dict(items_per_s=round(statistics.median(rates), 1), items_per_s_min=round(min(rates), 1), items_per_s_max=round(max(rates), 1),
                ms_per_call_median=round(statistics.median(window_ms) / calls, 4), items_per_call=items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "seal.json"))
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--commit", default="unlabelled")
    a = ap.parse_args()
    import numpy as np
    import torch
    import fixtures as F
    import gg20_fixture as G
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    signers = [0, 2]
    lk = G.make_local_keys(F.load_keys(), 1, 3, signers)
    gk = E.Gg20Keys(ctx, 1, 3, signers, lk["arrays"])
    B = a.slots
    seed = hashlib.sha256(b"exp_seal").digest()
    wk = E.WrapKey(ctx, hashlib.sha256(b"exp_seal wrapping key").digest())
    pool = E.PresigPool(ctx, gk, [0, 1], B)
    nonces, fail = E.gg20_sample_nonces(ctx, gk, B, seed, 1)
    got = E.gg20_presign(ctx, gk, nonces, B, pool)
    ctx.sync()
    assert int(fail.item()) == 0 and sorted(got.tolist()) == list(range(B))
    del nonces
    slots = torch.from_numpy(np.random.default_rng(1).permutation(B).astype(np.int32)).to(ctx.device)      # never arange
    rec, st = pool.export(slots)
    assert not st.any().item() and pool.audit()["stray"] == 0
    N, dv = E.N_, ctx.device
    status = torch.empty((B,), dtype=torch.int32, device=dv)
    sealed = torch.empty((B, pool.sealed_words), dtype=torch.int32, device=dv)
    out_rec = torch.empty_like(rec)
    ctr = [1]

    def imp():
        N.check(N.lib.mpe_gg20_presig_import(pool.h, B, E._ptr(slots), E._ptr(rec), E._ptr(status), ctx.stream()), "import")

    def exp():
        N.check(N.lib.mpe_gg20_presig_export(pool.h, B, E._ptr(slots), E._ptr(out_rec), E._ptr(status), ctx.stream()), "export")

    def imp_sealed():
        N.check(N.lib.mpe_gg20_sealed_presig_import(pool.h, wk.h, B, E._ptr(slots), E._ptr(sealed), E._ptr(status), ctx.stream()), "import_sealed")

    def exp_sealed():
        ctr[0] += 1
        N.check(N.lib.mpe_gg20_sealed_presig_export(pool.h, wk.h, B, E._ptr(slots), ctr[0], E._ptr(sealed), E._ptr(status), ctx.stream()), "export_sealed")

    # once through, checked: the sealed round trip gives the records back
    imp(); exp_sealed(); assert not status.any().item()
    imp_sealed(); assert not status.any().item()
    exp(); assert not status.any().item() and torch.equal(out_rec, rec)
    imp(); exp_sealed()                                                      # the loop starts with EMPTY slots and sealed rows in hand
    ctx.sync()

    def span(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    calls = dict(**{"import": imp, "export": exp, "import_sealed": imp_sealed, "export_sealed": exp_sealed})
    win = {k: [] for k in calls}
    for _ in range(a.windows):
        ev = {k: [] for k in calls}
        for _ in range(a.calls):
            for k, fn in calls.items():
                ev[k].append(span(fn))
        ctx.sync()
        assert not status.any().item()
        for k, pairs in ev.items():
            win[k].append(sum(e0.elapsed_time(e1) for e0, e1 in pairs))
    assert pool.audit() == dict(EMPTY=B, READY=0, SIGNED=0, BUSY=0, stray=0)
    res = dict(box="%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0)), commit=a.commit,
               shape="(t, n) = (1, 3), signers [0, 2], both local", slots=B, record_words=pool.record_words, sealed_words=pool.sealed_words,
               windows=a.windows, calls_per_window=a.calls, **{k: figure(B, win[k], a.calls) for k in calls})
    res["export_sealed_over_export"] = round(res["export_sealed"]["ms_per_call_median"] / res["export"]["ms_per_call_median"], 2)
    res["import_sealed_over_import"] = round(res["import_sealed"]["ms_per_call_median"] / res["import"]["ms_per_call_median"], 2)
    pool.close()
    # the generic rows
    res["rows"] = {}
    for words in (72, 1024):
        plain = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, words), dtype=torch.int32, device=dv)
        srow = torch.empty((B, words + 10), dtype=torch.int32, device=dv)
        back = torch.empty_like(plain)

        def do_seal():
            ctr[0] += 1
            N.check(N.lib.mpe_seal(ctx.h, wk.h, 16, B, words, E._ptr(plain), ctr[0], E._ptr(srow), ctx.stream()), "mpe_seal")

        def do_unseal():
            N.check(N.lib.mpe_unseal(ctx.h, wk.h, 16, B, words, E._ptr(srow), E._ptr(back), E._ptr(status), ctx.stream()), "mpe_unseal")

        do_seal(); do_unseal(); ctx.sync()
        assert not status.any().item() and torch.equal(back, plain)
        w2 = dict(seal=[], unseal=[])
        for _ in range(a.windows):
            ev = dict(seal=[], unseal=[])
            for _ in range(a.calls):
                ev["seal"].append(span(do_seal))
                ev["unseal"].append(span(do_unseal))
            ctx.sync()
            for k, pairs in ev.items():
                w2[k].append(sum(e0.elapsed_time(e1) for e0, e1 in pairs))
        r = {k: figure(B, w2[k], a.calls) for k in w2}
        for k in r:
            r[k]["payload_GB_per_s"] = round(r[k]["items_per_s"] * words * 4 / 1e9, 2)
        res["rows"][str(words)] = r
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    wk.close()
    gk.close()


if __name__ == "__main__":
    main()
