"""GPU: mpe_sha512 and mpe_hmac_sha512 against hashlib / hmac on both sides of every padding boundary, and mpe_bip32_derive over the
case table of tests/bip32_cases.py: tweak, child key, chain code and status equal the restatement (tests/pyref_bip32.py) exactly; a
refused row has the all-ones tweak and zero outputs, its neighbours are untouched."""
import hashlib
import hmac

import numpy as np
import pytest
import torch

import bip32_cases as BC
import fixtures as F
import pyref_bip32 as PB

pytestmark = pytest.mark.gpu

PARENTS, ROWS, NAMES = BC.table()          # searched on the CPU at collection time


def _data(n, salt):
    return bytes((i * 131 + 7 * salt + (i >> 8)) & 255 for i in range(n))


def _rows(t):
    return [bytes(r) for r in t.cpu().numpy()]


def test_sha512_on_both_sides_of_every_padding_boundary(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E, _native as N
    for n in (0, 1, 111, 112, 119, 120, 127, 128, 129, 239, 240, 256, N.SHA512_MAX_MSG_BYTES):
        msgs = [_data(n, b) for b in range(3 if n > 4096 else 67)]              # more than one workgroup at the short lengths
        got = _rows(E.sha512(gpu_ctx, msgs))
        assert got == [hashlib.sha512(m).digest() for m in msgs], f"{n} bytes"


def test_sha512_refuses_a_message_beyond_the_documented_maximum(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E, _native as N
    big = torch.zeros((1, N.SHA512_MAX_MSG_BYTES + 1), dtype=torch.uint8, device=gpu_ctx.device)
    with pytest.raises(N.MpeError, match=r"rc=-1\b"):
        E.sha512(gpu_ctx, big)


def test_hmac_sha512_key_and_message_lengths(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    for kl in (0, 1, 32, 64, 127, 128):
        for n in (0, 37, 111, 112, 128):
            keys_ = [_data(kl, 100 + b) for b in range(5)]
            msgs = [_data(n, b) for b in range(5)]
            got = _rows(E.hmac_sha512(gpu_ctx, keys_, msgs))
            assert got == [hmac.new(k, m, hashlib.sha512).digest() for k, m in zip(keys_, msgs)], f"key {kl} bytes, message {n} bytes"


def test_hmac_sha512_refuses_a_key_longer_than_a_block(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E, _native as N
    with pytest.raises(N.MpeError, match=r"rc=-1\b"):
        E.hmac_sha512(gpu_ctx, [bytes(129)], [b"x"])
    assert "128" in N.lib.mpe_last_error().decode()


def _derive(ctx):
    from multi_party_ecdsa_amd import engine as E
    d_pub = torch.from_numpy(F.point_words([K for _, K, _ in PARENTS]).view(np.int32)).to(ctx.device)
    out = E.bip32_derive(ctx, d_pub, [cc for _, _, cc in PARENTS], [rw["path"] for rw in ROWS], depth=[rw["depth"] for rw in ROWS],
                         parent_idx=[rw["parent"] for rw in ROWS])
    ctx.sync()
    tweak, child, cc, status = [o.cpu().numpy() for o in out]
    return F.ints(tweak.view(np.uint32)), F.points(child.view(np.uint32)), [bytes(r) for r in cc], list(status)


def test_bip32_derive_equals_the_restatement_row_by_row(gpu_ctx):
    want = BC.expected()
    tweak, child, cc, status = _derive(gpu_ctx)
    for b, (st, t, K, c) in enumerate(want):
        assert (status[b], tweak[b], child[b], cc[b]) == (st, t, K, c), f"row {b}: {ROWS[b]}"


def test_bip32_refused_rows_never_read_as_tweak_zero(gpu_ctx):
    tweak, child, cc, status = _derive(gpu_ctx)
    for name, st in (("hardened", PB.STATUS_HARDENED), ("hardened below", PB.STATUS_HARDENED), ("over-deep", PB.STATUS_DEPTH),
                     ("negative depth", PB.STATUS_DEPTH), ("bad parent index", PB.STATUS_DEPTH), ("negative parent index", PB.STATUS_DEPTH)):
        b = NAMES[name]
        assert status[b] == st and tweak[b] == PB.ALL_ONES >= PB.Q and child[b] is None and cc[b] == bytes(32), name
    for name in ("after hardened", "after hardened below", "hardened beyond the depth", "after over-deep", "after bad parent index"):
        b = NAMES[name]
        x = PARENTS[ROWS[b]["parent"]][0]
        assert status[b] == 0 and F.points(F.point_words([child[b]]))[0] == PB.pyref.ec_mul((x + tweak[b]) % PB.Q, PB.pyref.G), name


def test_bip32_defaults_mean_parent_0_and_the_full_depth(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    ctx = gpu_ctx
    d_pub = torch.from_numpy(F.point_words([PARENTS[0][1]]).view(np.int32)).to(ctx.device)
    paths = [[5, 6, 7], [0, 0, 0]]
    tweak, child, cc, status = E.bip32_derive(ctx, d_pub, PARENTS[0][2], paths)
    ctx.sync()
    for b, path in enumerate(paths):
        st, t, K, c = PB.derive([(PARENTS[0][1], PARENTS[0][2])], 0, path, 3, 3)
        assert (int(status[b]), F.ints(tweak[b:b + 1].cpu().numpy().view(np.uint32))[0], bytes(cc[b].cpu().numpy())) == (st, t, c)
        assert F.points(child[b:b + 1].cpu().numpy().view(np.uint32))[0] == K
