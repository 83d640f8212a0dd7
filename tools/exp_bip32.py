#!/usr/bin/env python3
"""What signing for BIP32 child keys costs, one box, one job:

    python tools/exp_bip32.py [--out profiles/r14/bip32.json] [--rows 65536] [--calls 256] [--sessions 16384] [--windows 7]

  derive   mpe_bip32_derive rows/s at `--rows` rows, depth 1 and depth 5 (one parent, random non-hardened paths)
  hmac     mpe_hmac_sha512 items/s at `--rows` items: a 32-byte key and the 37-byte message of one CKDpub level
           (both: a window = `--calls` calls between two host synchronisations, one warm-up window, median of `--windows` with min..max)
  sign     (t, n) = (1, 3), `--sessions` sessions through mpe_gg20_sign_tweaks with a distinct tweak per session (depth-2 children of the
           wallet's key, derived on the device) against the same call without tweaks, alternating in one process, `--windows` windows
           each after one warm-up window (a window = one call between two host synchronisations; the nonces come from the device
           sampler, outside the window).  The tweaked call adds one small kernel ((S + 1) comb multiplications per session) beside the
           ladders: the expectation is a ratio near 1."""
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


def spread(v, digits=1):
    return dict(median=round(statistics.median(v), digits), min=round(min(v), digits), max=round(max(v), digits), windows=[round(x, digits) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "bip32.json"))
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=256)
    ap.add_argument("--sessions", type=int, default=16384)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--commit", default="unlabelled")
    a = ap.parse_args()
    import numpy as np
    import torch
    import fixtures as F
    import gg20_fixture as G
    from multi_party_ecdsa_amd import engine as E
    ctx = E.Context(0)
    out = dict(host=socket.gethostname(), commit=a.commit, version=E.N_.lib.mpe_version().decode())
    t, n, sets = 1, 3, [[0, 1], [0, 2], [1, 2]]
    lk = G.make_local_keys(F.load_keys(), t, n, sets[0])
    d_pub = torch.from_numpy(np.ascontiguousarray(lk["arrays"]["y"]).view(np.int32)).to(ctx.device)
    cc = hashlib.sha256(b"exp_bip32 chain code").digest()
    seed = hashlib.sha256(b"exp_bip32").digest()

    def timed(call, items):
        """items/s per window of a.calls calls; window 0 warms up"""
        rates = []
        for w in range(a.windows + 1):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            ctx.sync()
            if w:
                rates.append(items * a.calls / (time.perf_counter() - t0))
        return rates

    # ---- derive
    R = a.rows
    out["derive"] = dict(rows=R, unit="rows/s", calls_per_window=a.calls)
    for depth in (1, 5):
        paths = (E.sample_bits(ctx, R * depth, seed, 10 + depth, 31, 1).reshape(R, depth)).contiguous()
        tw, child, ccs, st = E.bip32_derive(ctx, d_pub, cc, paths)
        assert not st.any().item()
        out["derive"][f"depth_{depth}"] = spread(timed(lambda: E.bip32_derive(ctx, d_pub, cc, paths), R), 0)
        print(f"[derive] depth {depth}:", json.dumps(out["derive"][f"depth_{depth}"]), flush=True)

    # ---- hmac
    key = E.sample_bits(ctx, R, seed, 20, 256, 8).view(torch.uint8).reshape(R, 32).contiguous()
    msg37 = E.sample_bits(ctx, R, seed, 21, 320, 10).view(torch.uint8).reshape(R, 40)[:, :37].contiguous()
    out["hmac"] = dict(items=R, key_bytes=32, msg_bytes=37, unit="items/s", calls_per_window=a.calls,
                       **spread(timed(lambda: E.hmac_sha512(ctx, key, msg37), R), 0))
    print("[hmac]", json.dumps(out["hmac"]), flush=True)

    # ---- sign: tweaked against plain
    B = a.sessions
    gk = E.Gg20Keys(ctx, t, n, None, lk["arrays"], signer_sets=sets)
    ds = torch.zeros((B,), dtype=torch.int32, device=ctx.device)
    paths = E.sample_bits(ctx, B * 2, seed, 30, 31, 1).reshape(B, 2).contiguous()
    tweaks, child, _, st = E.bip32_derive(ctx, d_pub, cc, paths)
    assert not st.any().item() and len({bytes(r) for r in tweaks.cpu().numpy().view(np.uint8).reshape(B, 32)}) == B
    msg = E.sample_bits(ctx, B, seed, 99, 256, 8)
    ms = dict(plain=[], tweaked=[])
    counter = 1
    for w in range(a.windows + 1):
        for name in (("plain", "tweaked") if w % 2 == 0 else ("tweaked", "plain")):
            nonces, fail = E.gg20_sample_nonces(ctx, gk, B, seed, counter, sigset=ds, msg=msg)
            counter += 1
            ctx.sync()
            t0 = time.perf_counter()
            r, s, recid, status = E.gg20_sign(ctx, gk, nonces, B, sigset=ds, tweaks=tweaks if name == "tweaked" else None)
            ctx.sync()
            dt = (time.perf_counter() - t0) * 1e3
            assert int(fail.item()) == 0 and not status.any().item(), name
            if w:
                ms[name].append(dt)
            del nonces
        print(f"[sign] window {w}: " + "  ".join(f"{k} {v[-1]:.1f} ms" for k, v in ms.items() if v), flush=True)
    # the last tweaked batch under OpenSSL, with the device's child keys
    import ossl
    u32 = lambda x: x.cpu().numpy().view(np.uint32)
    if name != "tweaked":
        nonces, _ = E.gg20_sample_nonces(ctx, gk, B, seed, counter, sigset=ds, msg=msg)
        r, s, recid, status = E.gg20_sign(ctx, gk, nonces, B, sigset=ds, tweaks=tweaks)
        ctx.sync()
    assert ossl.ecdsa_verify(u32(child), u32(msg), u32(r), u32(s), threads=16).all()
    p, q = ms["plain"], ms["tweaked"]
    out["sign"] = dict(sessions=B, shape=[t, n], unit="ms per call", plain=spread(p), tweaked=spread(q),
                       tweaked_over_plain=round(statistics.median(q) / statistics.median(p), 4),
                       tweaked_median_inside_plain_range=bool(min(p) <= statistics.median(q) <= max(p)),
                       verified_under_the_child_keys="OpenSSL, every signature of the last tweaked batch")
    print("[sign]", json.dumps(out["sign"]), flush=True)
    gk.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
