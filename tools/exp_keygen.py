#!/usr/bin/env python3
"""Keygen dealing and the round-3 verdict: the new calls against the composition the library offered before, same run, same box.

    python tools/exp_keygen.py [--out profiles/r07/keygen_deal.json] [--items 65536] [--reps 7] [--calls 32]

For (t, n) = (1, 3) and (2, 5) at `items` items (dealers for mpe_vss_share, (session, party) pairs for the verdict):
  vss_share    mpe_vss_share
  round3       mpe_keygen_verify_round3 (masks and xi_commit)
  composed     the same verdict by hand: mpe_vss_point_commitment per (party, dealer), n - 1 x mpe_ec_add, mpe_dlog_verify, one comparison
The two verdict paths are timed alternately (`reps` windows each, after a warm-up of both); a window is `calls` back-to-back calls (one call
lasts a few milliseconds) and ends in a device synchronise; the figures are per call, medians over the windows, the spread is min..max.
Both paths get their inputs laid out beforehand.  Before timing, both paths must give the same xi_commit rows and verdicts."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, fn, calls):
    ctx.sync()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    ctx.sync()
    return (time.perf_counter() - t) / calls


def rate(items, secs):
    return dict(items_per_s=round(items / statistics.median(secs), 1), ms_median=round(1e3 * statistics.median(secs), 3),
                ms_min=round(1e3 * min(secs), 3), ms_max=round(1e3 * max(secs), 3))


def shape(ctx, E, torch, t, n, items, reps, calls):
    seed = hashlib.sha256(b"exp_keygen").digest()
    t1, S = t + 1, items // n
    B = S * n                                                              # whole sessions
    coef, _ = E.sample_scalar(ctx, B * t1, seed, 1)
    coef = coef.reshape(B, t1, 8)
    nonce, _ = E.sample_scalar(ctx, B, seed, 2)
    share = lambda: E.vss_share(ctx, n, coef)
    commits, shares = share()
    # honest sessions: party i of session s received shares[s, :, i]
    recv = shares.reshape(S, n, n, 8).transpose(1, 2).contiguous().reshape(B, n, 8)
    y = commits[:, 0].reshape(S, 1, n, 16).expand(S, n, n, 16).contiguous().reshape(B, n, 16)
    x, ysum, pk, R, z = E.keygen_construct_keypair(ctx, recv, y, nonce)
    z[1::7, 0] ^= 1                                                        # a seventh of the proofs is wrong: both paths must refuse the same items
    index = torch.arange(1, n + 1, dtype=torch.int32, device=ctx.device).reshape(1, n, 1).expand(S, n, n).reshape(B * n).contiguous()

    def fused():
        return E.keygen_verify_round3(ctx, n, commits, pk, R, z, want_xi=True)

    # the hand composition wants one row of commitments per (party, dealer): laid out once, outside the timed calls, as the inputs of the new call are
    com = commits.reshape(S, 1, n, t1 * 16).expand(S, n, n, t1 * 16).reshape(B * n, t1 * 16).contiguous()

    def composed():
        pts = E.vss_point_commitment(ctx, t1, com, index).reshape(B, n, 16)
        acc = pts[:, 0].contiguous()
        for j in range(1, n):
            acc = E.ec_add(ctx, acc, pts[:, j].contiguous())
        ok = E.dlog_verify(ctx, pk, R, z) & (acc == pk).all(dim=1).to(torch.uint8)
        return ok, acc

    (ok_f, _, xi_f), (ok_c, xi_c) = fused(), composed()                     # warm-up of both, and the agreement the timing rests on
    share()
    ctx.sync()
    assert torch.equal(xi_f, xi_c) and torch.equal(ok_f, ok_c), "the two verdict paths disagree"
    refused = int((ok_f == 0).sum().item())
    assert refused == len(range(1, B, 7)), refused
    tf, tc, ts = [], [], []
    for _ in range(reps):
        tf.append(timed(ctx, fused, calls))
        tc.append(timed(ctx, composed, calls))
        ts.append(timed(ctx, share, calls))
    res = dict(t=t, n=n, items=B, sessions=S, reps=reps, calls_per_window=calls, refused=refused, vss_share=rate(B, ts), round3=rate(B, tf), composed=rate(B, tc))
    res["round3_over_composed"] = round(res["round3"]["items_per_s"] / res["composed"]["items_per_s"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "keygen_deal.json"))
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=32)
    a = ap.parse_args()
    import torch
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    res = dict(shapes=[shape(ctx, E, torch, t, n, a.items, a.reps, a.calls) for t, n in ((1, 3), (2, 5))])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
