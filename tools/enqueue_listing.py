#!/usr/bin/env python3
"""Evidence that a host-side change queues the same work and runs as fast (profiles/r09):
  list <kernel_trace.csv> <out.txt>    per stream (per queue where the trace names no streams), in dispatch order, every launch of a
                                       rocprofv3 --kernel-trace CSV as kernel:grid; ids are renumbered by first use, so two runs compare
  compare <a.txt> <b.txt>              exit 0 when both listings hold the same streams with the same sequences; else the first difference
  ab <runs.jsonl>                      runs of {"case", "library": parent | new, "value"}: per case the medians, their ratio, and whether the
                                       new median stays within the parent's own spread (max - min) below the parent's median"""
import csv
import json
import re
import statistics
import sys


def listing(path):
    rows = list(csv.DictReader(open(path)))
    key = "Stream_Id" if rows and len({r.get("Stream_Id") for r in rows} - {None, ""}) > 1 else "Queue_Id"
    order = "Dispatch_Id" if rows and rows[0].get("Dispatch_Id") else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[order]))
    names, streams = {}, {}
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        kid = names.setdefault(name, len(names))
        streams.setdefault(r[key], []).append(f"{kid}:{r.get('Grid_Size_X') or r.get('Grid_Size')}")
    return key, order, names, list(streams.values())


def write_listing(src, dst):
    key, order, names, streams = listing(src)
    with open(dst, "w") as f:
        f.write(f"# one list per {key}, renumbered by first use; launches in {order} order as kernel:grid; {sum(map(len, streams))} launches\n")
        for name, kid in names.items():
            f.write(f"K {kid} {name}\n")
        for i, seq in enumerate(streams):
            f.write(f"S {i} {len(seq)}\n")
            for j in range(0, len(seq), 24):
                f.write(" ".join(seq[j:j + 24]) + "\n")
    print(f"{dst}: {len(streams)} lists by {key}, {sum(map(len, streams))} launches, {len(names)} kernels")


def read_listing(path):
    names, streams = {}, []
    for line in open(path):
        if line.startswith("#"):
            continue
        if line.startswith("K "):
            _, kid, name = line.rstrip("\n").split(" ", 2)
            names[kid] = name
        elif line.startswith("S "):
            streams.append([])
        else:
            streams[-1] += [(names[t.split(":")[0]], t.split(":")[1]) for t in line.split()]
    return streams


def compare(a, b):
    sa, sb = read_listing(a), read_listing(b)
    if len(sa) != len(sb):
        print(f"DIFFERENT: {len(sa)} lists against {len(sb)}")
        return 1
    for i, (x, y) in enumerate(zip(sa, sb)):
        if x != y:
            j = next((j for j, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            print(f"DIFFERENT: list {i} ({len(x)} against {len(y)} launches), first at launch {j}: {x[j:j + 1]} against {y[j:j + 1]}")
            return 1
    print(f"IDENTICAL: {len(sa)} lists, {sum(map(len, sa))} launches, the same (kernel, grid) sequence in each")
    return 0


def ab(path):
    runs = [json.loads(l) for l in open(path) if l.startswith("{")]
    bad = 0
    for case in dict.fromkeys(r["case"] for r in runs):
        v = {lib: [r["value"] for r in runs if r["case"] == case and r["library"] == lib] for lib in ("parent", "new")}
        mp, mn, spread = statistics.median(v["parent"]), statistics.median(v["new"]), max(v["parent"]) - min(v["parent"])
        ok = mn >= mp - spread
        bad += not ok
        print(json.dumps({"case": case, "parent": v["parent"], "new": v["new"], "median_parent": mp, "median_new": mn, "ratio": mn / mp,
                          "parent_spread": spread, "within_margin": ok}))
    return 1 if bad else 0


if __name__ == "__main__":
    cmd, args = sys.argv[1], sys.argv[2:]
    sys.exit(write_listing(*args) if cmd == "list" else compare(*args) if cmd == "compare" else ab(*args))
