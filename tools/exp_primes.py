#!/usr/bin/env python3
"""Prime search: the device against the host, same run, same box.

    python tools/exp_primes.py [--out profiles/r07/primes.json] [--batches 4096,16384] [--host-primes 320] [--only-gpu BATCH]

GPU: mpe_sample_prime (1024-bit primes, default cap) at each batch size, wall time of the whole call after a warm-up call.
Host: mpz_nextprime (orc_nextprime, the way every fixture here is minted) on 16 threads (GMP releases the GIL inside ctypes).
--only-gpu BATCH runs one timed search and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`)."""
import argparse
import hashlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gpu_search(ctx, E, batch, sid):
    t = time.perf_counter()
    out, attempt, fail = E.sample_prime(ctx, batch, hashlib.sha256(b"exp_primes").digest(), sid)
    ctx.sync()
    dt = time.perf_counter() - t
    a = attempt.cpu().numpy()
    return dict(batch=batch, seconds=round(dt, 4), primes_per_s=round(batch / dt, 1), failures=int(fail.cpu()[0]), mean_attempt=float(a.mean()), max_attempt=int(a.max()))


def host_mint(count, threads=16):
    import numpy as np
    import fixtures as F
    import orc
    orc.lib.orc_nextprime.restype = None

    def one(i):
        start = int.from_bytes(hashlib.sha256(b"exp_primes|%d" % i).digest() * 4, "big") | (1 << 1023) | 1
        out = np.zeros(32, dtype=np.uint32)
        orc.lib.orc_nextprime(32, orc._p(F.words([start], 32)), orc._p(out))
        return int(out[0])
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(count)))
    dt = time.perf_counter() - t
    return dict(primes=count, threads=threads, seconds=round(dt, 3), primes_per_s=round(count / dt, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "primes.json"))
    ap.add_argument("--batches", default="4096,16384")
    ap.add_argument("--host-primes", type=int, default=320)
    ap.add_argument("--only-gpu", type=int, default=0)
    a = ap.parse_args()
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    gpu_search(ctx, E, 256, 1)                                            # warm-up: module load, sieve table, workspace
    if a.only_gpu:
        print(json.dumps(gpu_search(ctx, E, a.only_gpu, 2)))
        return
    res = dict(gpu=[gpu_search(ctx, E, int(b), 10 + i) for i, b in enumerate(a.batches.split(","))], host=host_mint(a.host_primes))
    res["gpu_over_host"] = round(max(g["primes_per_s"] for g in res["gpu"]) / res["host"]["primes_per_s"], 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
