#!/usr/bin/env python3
"""What per-session signer sets cost and save, one box, one job:

    python tools/exp_sigsets.py [--out profiles/r11/sigsets.json] [--parent DIR] [--bench-runs 3] [--sessions 16384] [--windows 7]

  uniform_path   (with --parent DIR, a built checkout of the parent commit) bench.py's headline config run in DIR and here, alternating,
                 `--bench-runs` runs each, every run a fresh process; who goes first alternates from pair to pair (a box's rate
                 drifts down by about half a percent over such a job: the later run of a pair is the slower one).  The yardstick is the parent's own min..max on this box: the change's
                 median is to lie inside it or above it.  --only uniform_path stops there.
  mixed          (t, n) = (1, 3), one key object with the three signer sets, `--sessions` sessions through mpe_gg20_sign_sets: all on set 0,
                 then the sets assigned round-robin, alternating, `--windows` windows each (a window = one call between two host
                 synchronisations; the nonces come from the device sampler with the same set assignment, outside the window).  The ladders
                 see the same units in another order of moduli: the expectation is a ratio near 1.
  memory         free HBM (hipMemGetInfo) before and after building one 3-set key object, against three one-set objects for the same
                 wallet; the difference is checked against the fixed-base tables of 2 K n bases counted once instead of three times."""
import argparse
import hashlib
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bench_once(where, steps, warmup):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=where, capture_output=True,
                       text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py in {where}: exit {p.returncode}\n{p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["value"])


def spread(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1), runs=[round(x, 1) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "sigsets.json"))
    ap.add_argument("--parent", default="")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--sessions", type=int, default=16384)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--commit", default="unlabelled")
    ap.add_argument("--only", default="", help="uniform_path: the two benchmarks alone")
    a = ap.parse_args()
    out = dict(host=socket.gethostname(), commit=a.commit)

    if a.parent:
        par, now = [], []
        for i in range(a.bench_runs):
            for who in (("parent", "change") if i % 2 == 0 else ("change", "parent")):
                (par if who == "parent" else now).append(bench_once(a.parent if who == "parent" else ROOT, a.bench_steps, 1))
            print(f"[uniform_path] parent {par[-1]:.1f}  change {now[-1]:.1f} signatures/s", flush=True)
        p, c = spread(par), spread(now)
        out["uniform_path"] = dict(unit="signatures/s", config=f"bench.py --gpus 1 --steps {a.bench_steps} --warmup 1", parent=p, change=c,
                                   change_median_over_parent_median=round(c["median"] / p["median"], 4),
                                   change_median_inside_or_above_parent_range=bool(c["median"] >= p["min"]))

    if a.only == "uniform_path":
        print(json.dumps(out["uniform_path"]))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
        return
    import torch
    import fixtures as F
    import fb_cases as FB
    import gg20_fixture as G
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    t, n, sets = 1, 3, [[0, 1], [0, 2], [1, 2]]
    lk = G.make_local_keys(F.load_keys(), t, n, sets[0])
    free = lambda: (ctx.sync(), torch.cuda.mem_get_info(0)[0])[1]

    # ---- memory: the objects are built on an idle context, before anything else allocates
    f0 = free()
    one = [E.Gg20Keys(ctx, t, n, s, lk["arrays"]) for s in sets]
    f1 = free()
    wb_one = [k.fb_window_bits() for k in one]
    for k in one:
        k.close()
    f2 = free()
    gk = E.Gg20Keys(ctx, t, n, None, lk["arrays"], signer_sets=sets)
    f3 = free()
    wb = gk.fb_window_bits()
    tables = FB.table_bytes(n, wb)
    out["memory"] = dict(three_one_set_objects_bytes=f0 - f1, one_three_set_object_bytes=f2 - f3, saved_bytes=(f0 - f1) - (f2 - f3),
                         fb_window_bits=wb, fb_window_bits_of_the_three=wb_one, table_bytes_of_one_object=tables, expected_saving_bytes=2 * tables,
                         freed_after_closing_the_three=f2 - f1)
    print("[memory]", json.dumps(out["memory"]), flush=True)

    # ---- mixed against uniform
    B = a.sessions
    seed = hashlib.sha256(b"exp_sigsets").digest()
    assign = {"uniform": torch.zeros((B,), dtype=torch.int32, device=ctx.device),
              "mixed": (torch.arange(B, dtype=torch.int32, device=ctx.device) % len(sets)).contiguous()}
    msg = E.sample_bits(ctx, B, seed, 99, 256, 8)
    ms = {k: [] for k in assign}
    counter = 1
    for w in range(a.windows + 1):                                   # window 0 warms both up
        for name, ds in assign.items():
            nonces, fail = E.gg20_sample_nonces(ctx, gk, B, seed, counter, sigset=ds, msg=msg)
            counter += 1
            ctx.sync()
            t0 = time.perf_counter()
            r, s, recid, status = E.gg20_sign(ctx, gk, nonces, B, sigset=ds)
            ctx.sync()
            dt = (time.perf_counter() - t0) * 1e3
            assert int(fail.item()) == 0 and not status.any().item(), name
            if w:
                ms[name].append(dt)
            del nonces
        print(f"[mixed] window {w}: " + "  ".join(f"{k} {v[-1]:.1f} ms" for k, v in ms.items() if v), flush=True)
    u, m = ms["uniform"], ms["mixed"]
    out["mixed"] = dict(sessions=B, sets=sets, unit="ms per mpe_gg20_sign_sets call", uniform=spread(u), mixed=spread(m),
                        mixed_over_uniform=round(statistics.median(m) / statistics.median(u), 4),
                        mixed_median_inside_uniform_range=bool(min(u) <= statistics.median(m) <= max(u)))
    print("[mixed]", json.dumps(out["mixed"]), flush=True)
    gk.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
