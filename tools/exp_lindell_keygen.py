#!/usr/bin/env python3
"""Lindell'17 key generation on the device: whole wallets per second, the signature check, and the fused long-term verdict against
the composition the library offered before — same run, same box.

    python tools/exp_lindell_keygen.py [--out profiles/r07/lindell_keygen.json] [--wallets 4096] [--items 65536] [--reps 7] [--calls 32]
                                       [--keygen-reps R] [--keygen-calls C]

  keygen     E.lindell_keygen at `wallets` wallets (material minted on the device, a fresh counter per call), and beside it the four
             prime searches of one call alone (mpe_sample_prime x 4 at the same batch): their share of the chain's time
  verify     mpe_ecdsa_verify at `items` items (1024 distinct valid signatures tiled: the kernel's work does not depend on the values)
  verdict    mpe_lindell_keygen_verify_first_msg at `items` items against the same verdict by hand: 2 x mpe_hash_commit_point,
             mpe_dlog_verify and two comparisons; the two paths alternate; a seventh of the proofs is wrong and both must refuse it
A window is `calls` back-to-back calls and ends in a device synchronise; figures are per call, medians over `reps` windows, the spread
is min..max.  Every input is laid out before the window opens.  The whole chain lasts seconds per call, so its windows have their
own two parameters (default: those of the other parts); the file records what was run."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def keygen_part(ctx, E, B, reps, calls):
    seed = hashlib.sha256(b"exp_lindell_keygen").digest()
    counter = [0]

    def chain():
        counter[0] += 1
        w = E.lindell_keygen(ctx, B, seed, counter[0])
        assert bool(w["ok"].all().item()) and w["failures"] == 0
        return w

    def primes():
        counter[0] += 1
        for f in range(4):
            E.sample_prime(ctx, B, seed, counter[0] | (f << 56))

    chain(); primes()                                                      # warm-up of both
    tk, tp = [], []
    for _ in range(reps):
        tk.append(timed(ctx, chain, calls))
        tp.append(timed(ctx, primes, calls))
    res = dict(wallets=B, reps=reps, calls_per_window=calls, keygen=rate(B, tk), prime_search=rate(B, tp))
    res["wallets_per_s"] = res["keygen"]["items_per_s"]
    res["prime_search_share"] = round(statistics.median(tp) / statistics.median(tk), 3)
    return res


def verify_part(ctx, E, torch, items, reps, calls):
    import fixtures as F
    import orc
    import pyref
    Q = pyref.Q
    r = F.Rng("exp_lindell_verify")
    n = 1024
    d, k, m = ([r.below(Q - 1) + 1 for _ in range(n)] for _ in range(3))
    pub, R = orc.ec_mul_base(F.words(d, 8)), orc.ec_mul_base(F.words(k, 8))
    rr = [x % Q for x in F.ints(R[:, :8])]
    s = [pow(k[i], -1, Q) * (m[i] + rr[i] * d[i]) % Q for i in range(n)]
    s = [min(v, Q - v) for v in s]
    tile = lambda a: torch.from_numpy(a.view("int32")).to(ctx.device).repeat((items + n - 1) // n, 1)[:items].contiguous()
    dp, dm, dr, ds = tile(pub), tile(F.words(m, 8)), tile(F.words(rr, 8)), tile(F.words(s, 8))
    fn = lambda: E.ecdsa_verify(ctx, dp, dm, dr, ds)
    assert bool(fn().all().item()), "a valid signature was refused"
    t = [timed(ctx, fn, calls) for _ in range(reps)]
    return dict(items=items, distinct_signatures=n, reps=reps, calls_per_window=calls, ecdsa_verify=rate(items, t))


def verdict_part(ctx, E, torch, items, reps, calls):
    seed = hashlib.sha256(b"exp_lindell_verdict").digest()
    x, _ = E.sample_scalar(ctx, items, seed, 1)
    nonce, _ = E.sample_scalar(ctx, items, seed, 2)
    b1, b2 = E.sample_bits(ctx, items, seed, 3, 256, 8), E.sample_bits(ctx, items, seed, 4, 256, 8)
    m = E.lindell_keygen_first_msg(ctx, x, nonce, b1, b2)
    m["z"][1::7, 0] ^= 1                                                   # a seventh of the proofs is wrong

    def fused():
        return E.lindell_keygen_verify_first_msg(ctx, m["pk_com"], m["pok_com"], b1, b2, m["Q1"], m["R"], m["z"])

    def composed():
        c1, c2 = E.hash_commit_point(ctx, m["Q1"], b1), E.hash_commit_point(ctx, m["R"], b2)
        return E.dlog_verify(ctx, m["Q1"], m["R"], m["z"]) & (c1 == m["pk_com"]).all(dim=1).to(torch.uint8) & (c2 == m["pok_com"]).all(dim=1).to(torch.uint8)

    ok_f, ok_c = fused(), composed()
    ctx.sync()
    assert torch.equal(ok_f, ok_c), "the two verdict paths disagree"
    refused = int((ok_f == 0).sum().item())
    assert refused == len(range(1, items, 7)), refused
    tf, tc = [], []
    for _ in range(reps):
        tf.append(timed(ctx, fused, calls))
        tc.append(timed(ctx, composed, calls))
    res = dict(items=items, reps=reps, calls_per_window=calls, refused=refused, verdict=rate(items, tf), composed=rate(items, tc))
    res["verdict_over_composed"] = round(res["verdict"]["items_per_s"] / res["composed"]["items_per_s"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "lindell_keygen.json"))
    ap.add_argument("--wallets", type=int, default=4096)
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--keygen-reps", type=int, default=None)
    ap.add_argument("--keygen-calls", type=int, default=None)
    a = ap.parse_args()
    import torch
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    res = dict(verify=verify_part(ctx, E, torch, a.items, a.reps, a.calls), verdict=verdict_part(ctx, E, torch, a.items, a.reps, a.calls))
    print(json.dumps(res), flush=True)
    res["keygen"] = keygen_part(ctx, E, a.wallets, a.keygen_reps or a.reps, a.keygen_calls or a.calls)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
