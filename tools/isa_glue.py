"""Census of the instructions a pair ladder executes OUTSIDE its CIOS pass loops (sibling of tools/isa_blocks.py: the same -save-temps
ISA dump, instruction classes only).

The kernel's text is cut into basic blocks (at labels and after every branch) and linked into a graph.  The pass loops are the blocks
that are mostly v_mad_u64_u32: pass A stores the quotient digits (it holds ds_write), pass B with one
stream has pass A's MAC count, pass B with two streams has half as many again.  Three cycles of the steady state are then walked:

  squaring        pass A -> pass B (one stream) -> back to THAT pass A
  sq_then_mul1    the squaring's cycle as far as the end of its pass B, then a window multiplication (a block that fetches the table
                  row with 16-byte global loads -> pass A -> pass B with two streams) and back to the squaring's pass A;
                  `mul1_extra` = this cycle minus the squaring's
  half_squaring   pass A -> back to the same pass A without any pass B

Each leg is the path with the FEWEST instructions between its two ends that enters no other pass loop (Dijkstra over the block graph),
so every figure is a lower bound of what runs; the blocks of the path are listed with the branch that leaves each of them ("taken"
or "falls through").  The counts are those of the blocks outside the loops.

Where the phase machine offers several ways back to pass A, the shortest one need not be the squaring's: --via names the blocks it is
known to run through (read off the kernel's text; e.g. the block that writes the squaring's multiplier), and the file records them.

--kernel=modexp_kernel | fb_modexp_kernel (the montmul ladders of the main unit: one pass loop) reports one cycle, `multiplication`: the
loop and back to it.

Usage: python tools/isa_glue.py build/mpe_pair2048-...gfx950.s 'Cfg<2048,29,18,4>' true [out.json] [--via=squaring:.LBB10_84,...]"""
import heapq
import json
import re
import sys

BRANCH = ("s_cbranch_", "s_branch")
CLASSES = (("valu", ("v_",)), ("v_mov", ("v_mov_b32", "v_mov_b64", "v_accvgpr")), ("mad", ("v_mad_u64_u32",)), ("ds", ("ds_",)),
           ("global", ("global_", "buffer_", "flat_")), ("scratch", ("scratch_",)), ("s_waitcnt", ("s_waitcnt",)), ("s_nop", ("s_nop",)))


def count(ins):
    d = {"insts": len(ins)}
    for name, pre in CLASSES:
        d[name] = sum(1 for x in ins if x.startswith(pre))
    d["salu"] = sum(1 for x in ins if x.startswith("s_")) - d["s_waitcnt"] - d["s_nop"]
    return d


def kernel_blocks(path, cfg, slide, kernel="pair_modexp_kernel"):
    m = re.match(r"Cfg<(\d+),(\d+),(\d+),(\d+)>", cfg)
    tag = "CfgILi%sELi%sELi%sELi%sEEE" % m.groups() + ("Lb%dE" % (1 if slide else 0) if kernel == "pair_modexp_kernel" else "")
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN3mpe%d%sI" % (len(kernel), kernel)) and tag in l and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur, nth = [], {"name": "entry", "ins": []}, 0
    blocks.append(cur)
    for l in lines[start + 1:end]:
        if re.match(r"^\.LBB\d+_\d+:", l):
            cur, nth = {"name": l.split(":")[0], "ins": []}, 0
            blocks.append(cur)
        elif l.startswith("\t") and not l.strip().startswith((".", ";")):
            cur["ins"].append(l.strip().split(";")[0].strip())
            if cur["ins"][-1].startswith(BRANCH):
                nth += 1
                base = cur["name"].split("+")[0]
                cur = {"name": f"{base}+{nth}", "ins": []}
                blocks.append(cur)
    # a pass loop may leave from its middle (the one exit after STEPS steps), and the compiler may append the pass tail to it: the pieces
    # of one label up to the last that holds MACs stay ONE block where most of it is MACs, the way isa_blocks.py counts it
    nmad = lambda ins: sum(1 for x in ins if x.startswith("v_mad_u64_u32"))
    merged, i = [], 0
    while i < len(blocks):
        b = blocks[i]
        j = i + 1
        while j < len(blocks) and "+" in blocks[j]["name"]:
            j += 1
        heavy = [k for k in range(i, j) if nmad(blocks[k]["ins"]) >= 18]
        if "+" not in b["name"] and heavy:
            ins = [x for k in range(i, heavy[-1] + 1) for x in blocks[k]["ins"]]
            if 2 * nmad(ins) > len(ins) and nmad(ins) >= 100:
                merged.append({"name": b["name"], "ins": ins, "loop": True})
                i = heavy[-1] + 1
                continue
        merged.append(b)
        i += 1
    blocks = merged
    index = {b["name"]: i for i, b in enumerate(blocks)}
    for i, b in enumerate(blocks):
        last = b["ins"][-1] if b["ins"] else ""
        succ = [(index[x.split()[-1]], "taken") for x in b["ins"][:-1] if x.startswith(BRANCH)]       # (a merged loop's exits)
        if last.startswith(BRANCH):
            succ.append((index[last.split()[-1]], "taken"))
        if not last.startswith(("s_branch", "s_endpgm")) and i + 1 < len(blocks):
            succ.append((i + 1, "falls through"))
        b["succ"], b["n"] = succ, count(b["ins"])
    return blocks


def classify(blocks):
    """-> ({"A": [...], "B1": [...], "B2": [...]}: the pass-loop blocks, {block: its loop}: every loop with the few-instruction
    blocks that close its cycle (the compiler's latch beside a loop that leaves from its middle))"""
    loops = [i for i, b in enumerate(blocks) if b.get("loop")]
    if not loops:
        raise SystemExit("no pass loop found")
    base = min(blocks[i]["n"]["mad"] for i in loops)
    out, member = {"A": [], "B1": [], "B2": []}, {i: i for i in loops}
    for i in loops:
        n = blocks[i]["n"]
        two = 4 * n["mad"] > 5 * base
        out["B2" if two else ("A" if any(x.startswith("ds_write") for x in blocks[i]["ins"]) else "B1")].append(i)
        r = shortest(blocks, member, i, i, set(loops) - {i}, latch=True)
        if r and r[0] <= 8:
            member.update({j: i for j, _ in r[1]})
    return out, member


def shortest(blocks, member, src, dst, closed, latch=False):
    """fewest instructions from the exits of loop src to the entry of loop dst; the loops in `closed` are not entered"""
    best, heap = {}, []
    for m in [k for k, v in member.items() if v == src]:
        for s, how in blocks[m]["succ"]:
            if member.get(s) != src or (latch and m == src and s != src):
                heapq.heappush(heap, (0, s, ((m, how),)))
    while heap:
        cost, at, trail = heapq.heappop(heap)
        if member.get(at) == dst:
            return cost, trail
        if at in best or member.get(at) in closed:
            continue
        best[at] = cost
        for s, how in blocks[at]["succ"]:
            heapq.heappush(heap, (cost + blocks[at]["n"]["insts"], s, trail + ((at, how),)))
    return None


def walk(blocks, member, legs):
    """legs: [(src, dst)], each a pass loop or a block to pass through -> the counts and the trail of the whole walk, or None where
    a leg has no path"""
    trail, loops = [], set(member.values())
    for src, dst in legs:
        mem = dict(member)
        mem.setdefault(src, src)
        mem.setdefault(dst, dst)
        r = shortest(blocks, mem, src, dst, loops - {dst})
        if r is None:
            return None
        trail += r[1]
    glue = [i for i, _ in trail if i not in member]
    tot = count([x for i in glue for x in blocks[i]["ins"]])
    steps = [f"{blocks[i]['name']} ({'pass loop' if i in member else blocks[i]['n']['insts']}) {how}" for i, how in trail]
    return {"outside_loops": tot, "path": steps}


def best_walk(blocks, member, candidates):
    walks = [w for w in (walk(blocks, member, legs) for legs in candidates) if w]
    return min(walks, key=lambda w: w["outside_loops"]["insts"]) if walks else None


def census(path, cfg, slide, via=None, kernel="pair_modexp_kernel"):
    """via: {"squaring" | "half_squaring": [block names]} — blocks the way back to pass A is known to run through (read off the
    kernel: the phase machine's branches are data the graph does not hold); without it the shortest way counts"""
    blocks = kernel_blocks(path, cfg, slide, kernel)
    cl, member = classify(blocks)
    index = {b["name"]: i for i, b in enumerate(blocks)}
    via = {k: [index[x] for x in v] for k, v in (via or {}).items()}
    chain = lambda last, a, mid: list(zip([last] + mid, mid + [a]))
    rows = [i for i, b in enumerate(blocks) if any(x.startswith("global_load_dwordx4") for x in b["ins"])]
    res = {"kernel": f"pair_modexp_kernel<{cfg}, {'true' if slide else 'false'}>" if kernel == "pair_modexp_kernel" else f"{kernel}<{cfg}>",
           "via": {k: [blocks[i]["name"] for i in v] for k, v in via.items()},
           "pass_loops": {k: [dict(block=blocks[i]["name"], **blocks[i]["n"]) for i in v] for k, v in cl.items()},
           "largest_glue_blocks": sorted((dict(block=b["name"], **b["n"]) for i, b in enumerate(blocks) if i not in member),
                                         key=lambda d: -d["insts"])[:12]}
    if not cl["A"]:                                           # a montmul ladder (modexp_kernel, fb_modexp_kernel): one loop, one cycle
        res["multiplication"] = best_walk(blocks, member, [chain(a, a, via.get("multiplication", [])) for a in cl["B1"]])
        return res
    vs = via.get("squaring", [])
    sq = best_walk(blocks, member, [[(a, b)] + chain(b, a, vs) for a in cl["A"] for b in cl["B1"]])
    res["squaring"] = sq
    if sq:
        cands = []
        for a in cl["A"]:
            for b in cl["B1"]:
                for g in rows:
                    for a2 in cl["A"]:
                        for b2 in cl["B2"]:
                            cands.append([(a, b), (b, g), (g, a2), (a2, b2)] + chain(b2, a, vs))
        mul = best_walk(blocks, member, cands)
        if mul:
            mul["mul1_extra"] = {k: mul["outside_loops"][k] - sq["outside_loops"][k] for k in mul["outside_loops"]}
        res["sq_then_mul1"] = mul
    res["half_squaring"] = best_walk(blocks, member, [chain(a, a, via.get("half_squaring", vs)) for a in cl["A"]])
    return res


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    via, kernel = {}, "pair_modexp_kernel"
    for x in sys.argv[1:]:
        if x.startswith("--kernel="):
            kernel = x[len("--kernel="):]
        if x.startswith("--via="):
            name, names = x[len("--via="):].split(":")
            via[name] = names.split(",")
    path, cfg, slide = args[0], args[1], args[2] in ("true", "1")
    res = census(path, cfg, slide, via, kernel)
    for k in ("squaring", "sq_then_mul1", "half_squaring", "multiplication"):
        if k not in res:
            continue
        w = res[k]
        print(k, "-", json.dumps(w["outside_loops"]) if w else "no such path")
        if w:
            for s in w["path"]:
                print("    ", s)
            if "mul1_extra" in w:
                print("   mul1_extra", json.dumps(w["mul1_extra"]))
    if len(args) > 3:
        with open(args[3], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
