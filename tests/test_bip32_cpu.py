"""CPU tests of the BIP32 restatement (tests/pyref_bip32.py), of the rule the GG20 tweak rests on (adding a public tweak to every
Shamir share gives the child key's wallet), of the child-wallet builder and of the case table (tests/bip32_cases.py) the GPU test
runs; and of the new C boundary: the typed constants as a C compiler sees them, NULL handles refused before any HIP call."""
import ctypes as C
import hashlib
import hmac
import itertools
import os
import subprocess

import numpy as np

import bip32_cases as BC
import fixtures as F
import gg20_fixture as G
import pyref
import pyref_bip32 as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = pyref.Q
PARENTS, ROWS, NAMES = BC.table()          # searched at collection time


def test_child_private_key_times_G_is_the_child_public_key():
    """(x + tweak) G == child_pub along paths of depth 0..5, against the PRIVATE derivation level by level"""
    r = F.Rng("bip32-priv")
    for depth in range(6):
        x = r.below(Q - 1) + 1
        cc = r.bits(256).to_bytes(32, "big")
        path = [r.below(1 << 31) for _ in range(depth)]
        st, t, child, ccc = PB.derive([(pyref.ec_mul(x, pyref.G), cc)], 0, path + [0] * (5 - depth), depth, 5)
        assert st == 0
        assert pyref.ec_mul((x + t) % Q, pyref.G) == child
        xp, cp = x, cc
        for i in path:
            xp, cp = PB.ckd_priv(xp, cp, i)
        assert xp == (x + t) % Q and cp == ccc
        if depth == 0:
            assert t == 0 and ccc == cc and child == pyref.ec_mul(x, pyref.G)


def test_ser_p_is_33_bytes_whatever_x_is():
    assert PB.ser_p((1, 2)) == b"\x02" + bytes(31) + b"\x01" and PB.ser_p((1 << 255, 3))[0] == 3
    assert len(PB.ser_p((5, 7))) == 33


def _lagrange0(ids, i):
    num = den = 1
    for j in ids:
        if j != i:
            num = num * (j + 1) % Q
            den = den * ((j + 1) - (i + 1)) % Q
    return num * pow(den, -1, Q) % Q


def test_tweaked_shares_reconstruct_the_child_key_under_every_quorum():
    r = F.Rng("bip32-shamir")
    for t_, n in ((1, 3), (2, 5)):
        coef = [r.below(Q - 1) + 1 for _ in range(t_ + 1)]
        xs = [sum(c * pow(i + 1, e, Q) for e, c in enumerate(coef)) % Q for i in range(n)]
        for tw in (0, 1, Q - 1, r.below(Q)):
            for quorum in itertools.combinations(range(n), t_ + 1):
                got = sum(_lagrange0(quorum, i) * ((xs[i] + tw) % Q) for i in quorum) % Q
                assert got == (coef[0] + tw) % Q
                # ... and so do the public sides: sum lambda_i (X_i + t G) = y + t G
                acc = None
                for i in quorum:
                    acc = pyref.ec_add(acc, pyref.ec_mul(_lagrange0(quorum, i), pyref.ec_mul((xs[i] + tw) % Q, pyref.G)))
                assert acc == pyref.ec_mul((coef[0] + tw) % Q, pyref.G)


def test_child_wallet_builder():
    lk = G.make_local_keys(F.load_keys(), 1, 3, [0, 2])
    for tw in (0, 1, Q - 1, F.Rng("bip32-wallet").below(Q)):
        ch = PB.child_wallet(lk, tw)
        xs, cx = F.ints(lk["arrays"]["x"]), F.ints(ch["arrays"]["x"])
        assert cx == [(x + tw) % Q for x in xs]
        assert F.points(ch["arrays"]["X"]) == [pyref.ec_mul(x, pyref.G) for x in cx]
        assert F.points(ch["arrays"]["y"]) == [ch["y"]] and ch["y"] == pyref.ec_mul((lk["x"] + tw) % Q, pyref.G) and ch["x"] == (lk["x"] + tw) % Q
        for f in lk["arrays"]:
            if f not in ("x", "X", "y"):
                assert np.array_equal(ch["arrays"][f], lk["arrays"][f]) and ch["arrays"][f] is not lk["arrays"][f], f
        assert ch["keys"] is lk["keys"] and (ch["t"], ch["n"], ch["S"]) == (lk["t"], lk["n"], lk["S"])
        if tw == 0:
            assert np.array_equal(ch["arrays"]["x"], lk["arrays"]["x"]) and np.array_equal(ch["arrays"]["X"], lk["arrays"]["X"])


def test_case_table_holds_what_it_promises():
    want = BC.expected()
    pub = [(K, cc) for _, K, cc in PARENTS]
    assert len(ROWS) == BC.ROWS == 64 and {rw["parent"] for rw in ROWS} >= {0, 1}
    assert {rw["depth"] for rw, w in zip(ROWS, want) if w[0] == 0} == set(range(BC.MAX_DEPTH + 1))
    rw = ROWS[NAMES["leading zero byte"]]
    first = PB.ckd_pub(*pub[rw["parent"]], rw["path"][0])[1]
    assert first[0] >> 248 == 0 and rw["depth"] == 2 and want[NAMES["leading zero byte"]][0] == 0
    for name, parity in (("even y", 0), ("odd y", 1)):
        rw = ROWS[NAMES[name]]
        assert PB.ckd_pub(*pub[rw["parent"]], rw["path"][0])[1][1] & 1 == parity
    assert ROWS[NAMES["index 0"]]["path"][0] == 0 and ROWS[NAMES["index 2^31 - 1"]]["path"][0] == (1 << 31) - 1
    assert ROWS[NAMES["hardened"]]["path"][0] == 1 << 31
    for name, st in (("hardened", PB.STATUS_HARDENED), ("hardened below", PB.STATUS_HARDENED), ("over-deep", PB.STATUS_DEPTH),
                     ("negative depth", PB.STATUS_DEPTH), ("bad parent index", PB.STATUS_DEPTH), ("negative parent index", PB.STATUS_DEPTH)):
        assert want[NAMES[name]] == (st, PB.ALL_ONES, None, bytes(32)), name
    for name in ("after hardened", "after hardened below", "hardened beyond the depth", "after over-deep", "after bad parent index",
                 "depth 0", "full depth", "index 0", "index 2^31 - 1"):
        assert want[NAMES[name]][0] == 0, name
    st, t, child, cc = want[NAMES["depth 0"]]
    assert (t, child, cc) == (0, PARENTS[1][1], PARENTS[1][2])
    for (x, _, _), (st, t, child, _), rw in ((PARENTS[rw["parent"]], w, rw) for w, rw in zip(want, ROWS) if w[0] == 0):
        assert pyref.ec_mul((x + t) % Q, pyref.G) == child
    assert sum(1 for w in want if w[0]) == 6


def test_the_device_text_of_sha512_and_hmac_on_the_host():
    """csrc/mpe_sha512.h compiled for the host (tools/model/sha512_host.cpp) against hashlib / hmac at the lengths of the GPU test"""
    out = os.path.join(ROOT, "build", "libsha512_host.so")
    src = os.path.join(ROOT, "tools", "model", "sha512_host.cpp")
    inc = os.path.join(ROOT, "multi_party_ecdsa_amd", "csrc")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, os.path.join(inc, "mpe_sha512.h"))):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMPE_SHA512_HOST", "-I", inc, src, "-o", out])
    lib = C.CDLL(out)
    lib.sha512h_digest.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p]
    lib.sha512h_hmac.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p]
    lib.sha512h_digest.restype = lib.sha512h_hmac.restype = None
    data = lambda n, salt: bytes((i * 131 + 7 * salt + (i >> 8)) & 255 for i in range(n))
    buf = C.create_string_buffer(64)
    for n in (0, 1, 111, 112, 119, 120, 127, 128, 129, 239, 240, 256, 1024, 65536):
        m = data(n, n)
        lib.sha512h_digest(m, n, buf)
        assert buf.raw == hashlib.sha512(m).digest(), f"{n} bytes"
    for kl in (0, 1, 32, 64, 127, 128):
        for n in (0, 37, 111, 112, 128):
            k, m = data(kl, 100 + n), data(n, kl)
            lib.sha512h_hmac(k, kl, m, n, buf)
            assert buf.raw == hmac.new(k, m, hashlib.sha512).digest(), f"key {kl} bytes, message {n} bytes"


def test_constants_are_what_a_c_compiler_sees(tmp_path):
    from multi_party_ecdsa_amd import _native as N
    names = ["MPE_GG20_STATUS_BAD_TWEAK", "MPE_SHA512_MAX_MSG_BYTES", "MPE_BIP32_MAX_DEPTH", "MPE_BIP32_STATUS_HARDENED", "MPE_BIP32_STATUS_INVALID",
             "MPE_BIP32_STATUS_DEPTH"]
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include "mpecdsa_hip.h"\nint main(void) {\n'
                   + "\n".join(f'  printf("{n} %lld\\n", (long long){n});' for n in names) + "\n  return 0;\n}\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert {k: int(v) for k, v in seen.items()} == {n: getattr(N, n[len("MPE_"):]) for n in names}
    assert (N.GG20_STATUS_BAD_TWEAK, N.BIP32_STATUS_HARDENED, N.BIP32_STATUS_INVALID, N.BIP32_STATUS_DEPTH) == \
        (PB.BAD_TWEAK, PB.STATUS_HARDENED, PB.STATUS_INVALID, PB.STATUS_DEPTH)
    assert N.SHA512_MAX_MSG_BYTES >= 1024 and BC.MAX_DEPTH <= N.BIP32_MAX_DEPTH


def test_argument_errors_without_gpu():
    from multi_party_ecdsa_amd import _native as N
    L = N.lib
    assert L.mpe_sha512(None, 1, None, 0, None, None) == N.MPE_E_ARG
    assert L.mpe_hmac_sha512(None, 1, None, 0, None, 0, None, None) == N.MPE_E_ARG
    assert L.mpe_bip32_derive(None, 1, 1, None, None, None, None, None, 1, None, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_gg20_session_create_tweaks(None, None, 1, 1, None, None, None, 0, None, None, 0, None, None) == N.MPE_E_ARG
    assert L.mpe_gg20_session_rearm_tweaks(None, None, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_gg20_session_child_keys(None, None, None) == N.MPE_E_ARG
    assert L.mpe_gg20_sign_tweaks(None, None, 1, None, None, None, None, None, None, None, None, None, 0, 0, None) == N.MPE_E_ARG
