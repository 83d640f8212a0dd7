#!/usr/bin/env python3
"""GG18 signing on the device: signatures per second of the whole chain, what its heavy launches cost, and the bound the two Paillier
primitives imply — same run, same box.

    python tools/exp_gg18.py [--out profiles/r09/gg18_sign.json] [--sessions 1024,16384] [--reps 5] [--commit LABEL]

  chain      E.gg18_sign at (t, n) = (1, 3), signers [0, 2], both local, every draw by the device sampler INSIDE the timed call (a fresh
             counter per call).  A call ends in a device synchronise; figures are medians over `reps` calls, the spread is min..max.
  split      one more call under mpe_prof_*: the ladder launches in launch order (MessageA's r^N, MessageB's r^N c_a^b, the decryptions),
             the modular multiplications summed, and what is left of the call's time for the EC phases, the sampler and the glue.
  paillier   mpe_paillier_encrypt under the PEER's key (no CRT: what MessageB's r^N costs) at 6 x sessions items and
             mpe_paillier_decrypt (CRT) at 4 x sessions items, alone.
  bound      a two-signer session holds 6 exponentiations r^N mod N^2 (2 MessageA, 4 MessageB) and 4 CRT decryptions; its 4 c_a^b with
             256-bit exponents ride MessageB's ladders and are left out, and MessageA's two encryptions run through the CRT, faster than
             the rate used here — so: sessions/s <= 1 / (6 / encrypt_rate + 4 / decrypt_rate), an estimate from counts, and
             achieved_over_bound = chain / that."""
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


def rate(items, secs):
    return dict(items_per_s=round(items / statistics.median(secs), 1), ms_median=round(1e3 * statistics.median(secs), 3),
                ms_min=round(1e3 * min(secs), 3), ms_max=round(1e3 * max(secs), 3))


def timed(ctx, fn):
    ctx.sync()
    t = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "gg18_sign.json"))
    ap.add_argument("--sessions", default="1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="unlabelled")
    a = ap.parse_args()
    import torch
    import gg18_cases as K
    import ossl
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    lk, w, sg = K.wallet("t1n3")
    wal = E.Gg18Wallet(ctx, lk["t"], lk["n"], lk["arrays"])
    seed = hashlib.sha256(b"exp_gg18").digest()
    res = dict(box="%s / %s" % (socket.gethostname(), torch.cuda.get_device_name(0)), commit=a.commit, shape="(t, n) = (1, 3), signers [0, 2], both local",
               reps=a.reps, runs=[])
    counter = [0]
    for B in [int(x) for x in a.sessions.split(",")]:
        msg = E.sample_bits(ctx, B, seed, 99, 256, 8)
        last = {}

        def chain():
            counter[0] += 1
            last["out"] = E.gg18_sign(ctx, wal, sg, msg, B, seed=seed, counter=counter[0])

        chain()                                                                # warm-up, and the check that what is timed signs
        o = last["out"]
        assert not o["status"].any().item() and o["failures"] == 0
        npu = lambda t: t.cpu().numpy().view("uint32")
        chk = min(B, 256)
        assert ossl.ecdsa_verify(lk["arrays"]["y"][0], npu(msg)[:chk], npu(o["r"])[:chk], npu(o["s"])[:chk]).all()
        tc = [timed(ctx, chain) for _ in range(a.reps)]
        # the heavy launches of one call
        ctx.prof_enable(True)
        t_prof = timed(ctx, chain)
        recs = ctx.prof_collect()
        ctx.prof_enable(False)
        split = [{k: (round(v, 3) if k == "ms" else v) for k, v in r.items() if k in ("kind", "bits", "exp_words", "exp2_words", "batch", "ms")}
                 for r in recs if r["kind"] != 1]                               # the ladders, in launch order (kinds: include/mpecdsa_hip.h)
        mm = sum(r["ms"] for r in recs if r["kind"] == 1)
        heavy = sum(r["ms"] for r in recs)
        # the two primitives alone, at the item counts of the chain
        nE, nD = 6 * B, 4 * B
        kE = torch.tensor([sg[i % 2] for i in range(nE)], dtype=torch.int32, device=ctx.device)
        mE, _ = E.sample_below(ctx, nE, seed, 97, wal.N, 64, kE)
        rE, _ = E.sample_below(ctx, nE, seed, 98, wal.N, 64, kE)
        cE = torch.empty((nE, 128), dtype=torch.int32, device=ctx.device)
        enc = lambda: wal.pk.encrypt_device(mE, rE, kE, cE)
        kS = torch.tensor([sg[i % 2] for i in range(nD)], dtype=torch.int32, device=ctx.device)
        cD = wal.pk.encrypt_device(mE[:nD].contiguous(), rE[:nD].contiguous(), kS)
        mD = torch.empty((nD, 64), dtype=torch.int32, device=ctx.device)
        own = [wal.own.index(s) for s in sg]
        kD = torch.tensor([own[i % 2] for i in range(nD)], dtype=torch.int32, device=ctx.device)
        dec = lambda: wal.sk.decrypt_device(cD, kD, mD)
        enc(); dec()
        ctx.sync()
        assert torch.equal(mD, mE[:nD]), "decrypt(encrypt(m)) != m"
        te, td = [], []
        for _ in range(a.reps):                                                # alternating
            te.append(timed(ctx, enc))
            td.append(timed(ctx, dec))
        run = dict(sessions=B, chain=rate(B, tc), encrypt_public=rate(nE, te), decrypt_crt=rate(nD, td),
                   heavy_launches=split, modmul_ms=round(mm, 3), heavy_ms=round(heavy, 3), profiled_call_ms=round(1e3 * t_prof, 3),
                   other_ms=round(1e3 * t_prof - heavy, 3))
        run["signatures_per_s"] = run["chain"]["items_per_s"]
        bound = 1.0 / (6.0 / run["encrypt_public"]["items_per_s"] + 4.0 / run["decrypt_crt"]["items_per_s"])
        run["bound_signatures_per_s"] = round(bound, 1)
        run["achieved_over_bound"] = round(run["signatures_per_s"] / bound, 3)
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    wal.close()


if __name__ == "__main__":
    main()
