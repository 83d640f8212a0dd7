#!/usr/bin/env python3
"""Safe-prime search: the rate, the plain search beside it, a counted bound, a host yardstick.  Same run, same box.

    python tools/exp_safe_primes.py [--out profiles/r11/safe_primes.json] [--batches 64,1024,4096] [--windows 7] [--host-primes 16]
                                    [--kernel-stats FILE.csv --kernel-run FILE.json --kernel-trace FILE.csv] [--reduce-trace RAW.csv OUT.csv] [--resplit OUT.json] [--only-gpu BATCH] [--extra-pass-logs 20,26] [--parent COMMIT]

GPU: mpe_sample_safe_prime and mpe_sample_prime (1024 bits, default caps) at each batch, wall time of the whole call after a warm-up
call, `--windows` calls each (another stream id per call); the file holds the median and min..max.  Every call's counts come from
mpe_prime_search_counts (attempts sieved, the list length behind every stage).
--only-gpu BATCH runs one plain and one safe search and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`.  Its
kernel statistics (CSV) come back in through --kernel-stats, its trace through --kernel-trace (the mean time of each launch of a pass:
sieve / round 1 / rounds 2..8): the time by kernel and the counted bound
    safe primes/s <= 1 / (attempts per result / sieve candidate rate + exponentiations per result / exponentiation rate)
with both rates taken from the PLAIN search's kernels in that run (sieve_kernel: attempts / its time; mr_kernel<Cfg1024>: its
exponentiations / the time of its launches before the first safe launch in the trace) and both counts per result from the safe search's own lists (7 per entry of a rounds-2..8 list: a composite
that leaves early counts in full).
Host: "a GMP safe-prime search, not the same rule" — mpz_nextprime (orc_nextprime) from random starts until (p - 1) / 2 is prime too,
16 threads.  No test asserts a rate."""
import argparse
import csv
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = hashlib.sha256(b"exp_safe_primes").digest()


def gpu_search(ctx, E, batch, sid, safe):
    E.prime_search_counts(ctx, reset=True)
    t = time.perf_counter()
    out, attempt, fail = (E.sample_safe_prime if safe else E.sample_prime)(ctx, batch, SEED, sid)
    ctx.sync()
    dt = time.perf_counter() - t
    a = attempt.cpu().numpy()
    pre = "safe_" if safe else ""
    counts = {k[len(pre):]: v for k, v in E.prime_search_counts(ctx).items() if k.startswith("safe_") == safe}
    return dict(batch=batch, seconds=round(dt, 4), per_s=round(batch / dt, 2), failures=int(fail.cpu()[0]), mean_attempt=float(a.mean()), max_attempt=int(a.max()),
                counts=counts)


def windows(ctx, E, batch, n, safe, sid0):
    runs = [gpu_search(ctx, E, batch, sid0 + i, safe) for i in range(n)]
    rate = [r["per_s"] for r in runs]
    tot = {k: sum(r["counts"][k] for r in runs) for k in runs[0]["counts"]}
    results = batch * n - sum(r["failures"] for r in runs)
    o = dict(batch=batch, windows=n, per_s_median=statistics.median(rate), per_s_min=min(rate), per_s_max=max(rate),
             seconds_median=statistics.median(r["seconds"] for r in runs), failures=sum(r["failures"] for r in runs),
             mean_attempt=round(statistics.mean(r["mean_attempt"] for r in runs), 1), counts=tot)
    if safe:      # per result: attempts sieved (the passes' unused tails included) and Miller-Rabin exponentiations (one per round and number)
        exps = tot["sieve"] + tot["round1_c"] + 7 * tot["round1_half"] + 7 * tot["rounds2_8_c"]
        o.update(attempts_per_result=round(tot["attempts"] / results, 1), exponentiations_per_result=round(exps / results, 1),
                 sieve_survival=round(tot["sieve"] / tot["attempts"], 5), head_survival=round(tot["sieve_head"] / tot["attempts"], 5))
    else:
        exps = tot["sieve"] + 7 * tot["round1"]
        o.update(attempts_per_result=round(tot["attempts"] / results, 1), exponentiations_per_result=round(exps / results, 1))
    return o


def host_mint(count, threads=16):
    import numpy as np
    import fixtures as F
    import orc
    orc.lib.orc_nextprime.restype = None

    def nextprime(v):
        out = np.zeros(32, dtype=np.uint32)
        orc.lib.orc_nextprime(32, orc._p(F.words([v], 32)), orc._p(out))
        return F.ints(out.reshape(1, 32))[0]

    def one(i):
        p = int.from_bytes(hashlib.sha256(b"exp_safe_primes|%d" % i).digest() * 4, "big") | (1 << 1023) | 1
        walked = 0
        while True:
            p = nextprime(p)
            walked += 1
            h = (p - 1) // 2
            if h % 2 and h % 3 and nextprime(h - 1) == h:
                return walked
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        walked = list(ex.map(one, range(count)))
    dt = time.perf_counter() - t
    return dict(label="a GMP safe-prime search, not the same rule", safe_primes=count, threads=threads, seconds=round(dt, 2), per_s=round(count / dt, 3),
                mean_primes_walked=round(statistics.mean(walked), 1))


def reduce_trace(raw, out):
    """rocprofv3's kernel trace (CSV) -> the search kernels' dispatches alone: kind, start_ns, end_ns from the first of them (the form kept
    in profiles/)"""
    kind = lambda n: ("safe_sieve_head" if "safe_sieve_head" in n else "safe_sieve_tail" if "safe_sieve_tail" in n else
                      "mr_half" if "pr::mr_kernel" in n and ", true>" in n else "mr_c" if "pr::mr_kernel" in n else
                      "plain_sieve" if "pr::sieve_kernel" in n else "finalize" if "finalize_kernel" in n else None)
    rows = sorted(csv.DictReader(open(raw)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [(kind(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
    rows = [r for r in rows if r[0]]
    t0 = rows[0][1]
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kind", "start_ns", "end_ns"])
        w.writerows((k, a - t0, b - t0) for k, a, b in rows)


def read_trace(path):
    return [(r["kind"], int(r["start_ns"]), int(r["end_ns"])) for r in csv.DictReader(open(path))]


def kernel_split(path, plain, safe, trace=None):
    """rocprofv3's kernel statistics of an --only-gpu run -> time per kernel of the two searches, the rates of the plain kernels, the bound.
    mr_kernel<Cfg1024, false> runs in both searches: with the (reduced) trace the plain search's launches are those before the first
    launch of the safe sieve; without it the instantiation's time is shared out by exponentiations and the rate is the POOLED one"""
    rows = list(csv.DictReader(open(path)))
    ns = lambda *subs: sum(float(r["TotalDurationNs"]) for r in rows if all(x in r["Name"] for x in subs))
    # mr_kernel<Cfg1024, false> tests c (both searches), mr_kernel<Cfg1024, true> tests (c - 1) / 2
    t = dict(plain_sieve=ns("pr::sieve_kernel"), mr_c=ns("pr::mr_kernel", ", false>"), mr_half=ns("pr::mr_kernel", ", true>"), safe_sieve_head=ns("safe_sieve_head_kernel"),
             safe_sieve_tail=ns("safe_sieve_tail_kernel"), bookkeeping=ns("finalize_kernel") + ns("iota_kernel") + ns("giveup_kernel"))
    pc, sc = plain["counts"], safe["counts"]
    plain_exps = pc["sieve"] + 7 * pc["round1"]
    safe_c_exps = sc["sieve"] + 7 * sc["round1_half"]
    safe_half_exps = sc["round1_c"] + 7 * sc["rounds2_8_c"]
    if trace:
        first_safe = min(a for k, a, _ in trace if k == "safe_sieve_head")
        mr_plain = float(sum(b - a for k, a, b in trace if k == "mr_c" and a < first_safe))
        rate_from = "the plain search's own mr_kernel launches (those before the first safe launch in the trace)"
    else:
        mr_plain = t["mr_c"] * plain_exps / (plain_exps + safe_c_exps)
        rate_from = "POOLED: mr_kernel<Cfg1024, false> of both searches, shared out by exponentiations"
    mr_safe_c = t["mr_c"] - mr_plain
    sieve_rate = pc["attempts"] / (t["plain_sieve"] * 1e-9)
    exp_rate = plain_exps / (mr_plain * 1e-9)
    results = safe["batch"] - safe["failures"]
    a_per, e_per = sc["attempts"] / results, (safe_c_exps + safe_half_exps) / results
    bound = 1.0 / (a_per / sieve_rate + e_per / exp_rate)
    safe_ns = t["safe_sieve_head"] + t["safe_sieve_tail"] + mr_safe_c + t["mr_half"]
    return dict(source=os.path.basename(path), batch=safe["batch"], kernel_ms={k: round(v * 1e-6, 3) for k, v in t.items()},
                plain_sieve_candidates_per_s=round(sieve_rate), plain_exponentiations_per_s=round(exp_rate), exponentiation_rate_from=rate_from,
                plain_mr_ms=round(mr_plain * 1e-6, 3), attempts_per_result=round(a_per, 1),
                exponentiations_per_result=round(e_per, 1), bound_safe_primes_per_s=round(bound, 2), kernel_time_safe_primes_per_s=round(results / (safe_ns * 1e-9), 2))


def stage_split(path):
    """the reduced kernel trace of an --only-gpu run -> mean time of every launch of a safe pass, in the order of the pass"""
    short = {"safe_sieve_head": "head", "safe_sieve_tail": "tail", "mr_c": "mr", "mr_half": "mr", "finalize": "finalize"}
    seq = [(short[k], (e - a_) * 1e-6) for k, a_, e in read_trace(path) if k in short]
    names = ("sieve_head", "sieve_tail", "round1_c", "round1_half", "rounds2_8_c", "rounds2_8_half", "finalize")
    want = ("head", "tail", "mr", "mr", "mr", "mr", "finalize")
    acc, i = [[] for _ in names], 0
    while i + 7 <= len(seq):
        if tuple(k for k, _ in seq[i:i + 7]) == want:
            for j in range(7):
                acc[j].append(seq[i + j][1])
            i += 7
        else:
            i += 1
    mean = {n: statistics.mean(v) for n, v in zip(names, acc)}
    tot = sum(mean.values())
    return dict(source=os.path.basename(path), passes=len(acc[0]), mean_ms_per_pass={n: round(v, 3) for n, v in mean.items()}, pass_ms=round(tot, 2),
                share=dict(sieve=round((mean["sieve_head"] + mean["sieve_tail"]) / tot, 4), round1=round((mean["round1_c"] + mean["round1_half"]) / tot, 4),
                           rounds2_8=round((mean["rounds2_8_c"] + mean["rounds2_8_half"]) / tot, 4)))


def add_kernel_figures(res, a):
    if a.kernel_stats:
        run = json.load(open(a.kernel_run))
        res["kernel_split"] = kernel_split(a.kernel_stats, run["plain"], run["safe"], read_trace(a.kernel_trace) if a.kernel_trace else None)
        top = [s for s in res["safe"] if s["batch"] == res["kernel_split"]["batch"]]
        if top:
            res["kernel_split"]["achieved_over_bound"] = round(top[0]["per_s_median"] / res["kernel_split"]["bound_safe_primes_per_s"], 3)
    if a.kernel_trace:
        res["pass_stages"] = stage_split(a.kernel_trace)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "safe_primes.json"))
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host-primes", type=int, default=16)
    ap.add_argument("--kernel-stats", default="", help="rocprofv3's kernel statistics (CSV) of an --only-gpu run")
    ap.add_argument("--kernel-trace", default="", help="the reduced kernel trace of the same run (--reduce-trace): the time of a pass by stage, the plain launches")
    ap.add_argument("--reduce-trace", nargs=2, metavar=("RAW.csv", "OUT.csv"), help="rocprofv3's kernel trace -> the reduced form --kernel-trace reads")
    ap.add_argument("--resplit", default="", help="a result file of this tool: recompute its kernel figures from the three files above, no GPU")
    ap.add_argument("--kernel-run", default="", help="what that --only-gpu run wrote with --out")
    ap.add_argument("--extra-pass-logs", default="", help="safe_pass_log values to try beside the default, 3 calls each at batch 1024")
    ap.add_argument("--parent", default="", help="the commit this tree was made from, for the record")
    ap.add_argument("--only-gpu", type=int, default=0)
    a = ap.parse_args()
    if a.reduce_trace:
        reduce_trace(*a.reduce_trace)
        return
    if a.resplit:
        res = json.load(open(a.resplit))
        add_kernel_figures(res, a)
        with open(a.resplit, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: res[k] for k in ("kernel_split", "pass_stages") if k in res}))
        return
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    if a.only_gpu:
        out = dict(plain=gpu_search(ctx, E, a.only_gpu, 2, False), safe=gpu_search(ctx, E, a.only_gpu, 3, True))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return
    gpu_search(ctx, E, 256, 1, False)                                     # warm-up: module load, sieve table, workspace
    gpu_search(ctx, E, 8, 1, True)
    res = dict(note="medians of %d calls per batch, min..max beside them; one box; no test asserts a rate" % a.windows, parent_commit=a.parent, safe=[], plain=[])
    for i, b in enumerate(int(x) for x in a.batches.split(",")):
        res["safe"].append(windows(ctx, E, b, a.windows, True, 1000 * (i + 1)))
        print("safe", json.dumps(res["safe"][-1]), flush=True)
        res["plain"].append(windows(ctx, E, b, a.windows, False, 1000 * (i + 1)))
        print("plain", json.dumps(res["plain"][-1]), flush=True)
    if a.extra_pass_logs:
        default = ctx.get_option("safe_pass_log")
        res["pass_size"] = []
        for lg in [int(x) for x in a.extra_pass_logs.split(",")] + [default]:
            ctx.set_option("safe_pass_log", lg)
            w = windows(ctx, E, 1024, 3, True, 9000 + 10 * lg)
            res["pass_size"].append(dict(safe_pass_log=lg, **{k: w[k] for k in ("batch", "windows", "per_s_median", "per_s_min", "per_s_max", "seconds_median")}))
            print("pass size", json.dumps(res["pass_size"][-1]), flush=True)
        ctx.set_option("safe_pass_log", default)
    add_kernel_figures(res, a)
    res["host"] = host_mint(a.host_primes)
    res["gpu_over_host"] = round(max(s["per_s_median"] for s in res["safe"]) / res["host"]["per_s"], 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
