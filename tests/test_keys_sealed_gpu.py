"""GPU tests of sealed key shares (`mpe_gg20_keyshare_seal`, `mpe_gg20_keys_create_sealed`): `gg20_keygen(..., wrap=)` seals every
party's x_i, p, q on the device before anything is copied out, `Gg20Keys(sealed_shares=, wrap=)` unseals them on the device, and
the wallets sign exactly what the unsealed path signs from the same seed.  (t, n) = (1, 3), 2 wallets, 4 sessions; the Paillier /
N~ material is the golden file's (tests/golden/keys16.json, as tests/keygen_fixture.py reads it), so no prime search runs."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import fixtures as F
import keygen_fixture as KF                                               # noqa: F401  (the golden keys' reader: F.HERE / golden)
import pyref_seal as PS
import seal_cases as SC

pytestmark = pytest.mark.gpu

T, N_PARTIES, WALLETS, SESSIONS = 1, 3, 2, 4
SEED, COUNTER, NONCE_HI = b"\x33" * 32, 5, 0x1122334455667788


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _material(B, n):
    with open(os.path.join(F.HERE, "golden", "keys16.json")) as f:
        raw = json.load(f)["keys"]
    rows = [raw[i % len(raw)] for i in range(B * n)]
    w = lambda field, words: F.words([int(k[field], 16) for k in rows], words)
    return dict(p=w("p", 32), q=w("q", 32), pt=w("nt_p", 32), qt=w("nt_q", 32), h1=w("h1", 64), xi=w("xhi", 64))


@pytest.fixture(scope="module")
def made(gpu_ctx):
    """the same key generation twice from one seed: in the clear, and sealed under the wrapping key"""
    from multi_party_ecdsa_amd import engine as E
    wk = E.WrapKey(gpu_ctx, SC.KEY)
    mat = _material(WALLETS, N_PARTIES)
    clear = E.gg20_keygen(gpu_ctx, T, N_PARTIES, WALLETS, SEED, counter=COUNTER, material=mat)
    sealed = E.gg20_keygen(gpu_ctx, T, N_PARTIES, WALLETS, SEED, counter=COUNTER, material=mat, wrap=wk, nonce_hi=NONCE_HI)
    assert list(clear["ok"].cpu().numpy()) == [1] * WALLETS == list(sealed["ok"].cpu().numpy())
    yield wk, clear, sealed
    wk.close()


def _sign(ctx, gk, y):
    from multi_party_ecdsa_amd import engine as E
    import ossl
    keyset = np.repeat(np.arange(WALLETS, dtype=np.int32), SESSIONS // WALLETS)
    msg = F.words([int.from_bytes(hashlib.sha256(b"sealed keys %d" % b).digest(), "big") for b in range(SESSIONS)], 8)
    d_ks = torch.from_numpy(keyset).to(ctx.device)
    d_msg = torch.from_numpy(msg.view(np.int32)).to(ctx.device)
    nonces, fail = E.gg20_sample_nonces(ctx, gk, SESSIONS, b"\x5b" * 32, 9, keyset=d_ks, msg=d_msg)
    r, s, recid, status = E.gg20_sign(ctx, gk, nonces, SESSIONS, keyset=d_ks)
    ctx.sync()
    assert int(fail.item()) == 0 and list(status.cpu().numpy()) == [0] * SESSIONS
    for w in range(WALLETS):
        sel = keyset == w
        assert ossl.ecdsa_verify(y[w], msg[sel], _u32(r)[sel], _u32(s)[sel]).all(), w
    return _u32(r).copy(), _u32(s).copy(), recid.cpu().numpy().copy()


def test_keygen_with_a_wrapping_key_returns_no_clear_secret(made):
    wk, clear, sealed = made
    a = sealed["arrays"]
    assert not {"x", "p", "q"} & set(a) and set(a) == set(clear["arrays"]) - {"x", "p", "q"}
    for f in a:
        assert np.array_equal(a[f], clear["arrays"][f]), f
    sh = sealed["sealed_shares"]
    assert sh.shape == (WALLETS * N_PARTIES, 82) and sh.dtype == np.uint32 and "sealed_shares" not in clear
    # the sealed rows are the restatement's over x | p | q of the clear run
    c = clear["arrays"]
    for g in range(WALLETS * N_PARTIES):
        row = np.concatenate([c["x"][g], c["p"][g], c["q"][g]])
        assert [int(v) for v in sh[g]] == PS.seal_row(SC.KEY, PS.KIND_KEYSHARE, g, NONCE_HI, row), g


def test_sealed_wallets_sign_what_the_clear_wallets_sign(gpu_ctx, made):
    from multi_party_ecdsa_amd import engine as E
    wk, clear, sealed = made
    signers = [0, 2]
    gk = E.Gg20Keys(gpu_ctx, T, N_PARTIES, signers, clear["arrays"], nkeysets=WALLETS)
    want = _sign(gpu_ctx, gk, clear["arrays"]["y"])
    gk.close()
    gs = E.Gg20Keys(gpu_ctx, T, N_PARTIES, signers, sealed["arrays"], nkeysets=WALLETS, sealed_shares=sealed["sealed_shares"], wrap=wk)
    got = _sign(gpu_ctx, gs, sealed["arrays"]["y"])
    gs.close()
    for a, b, f in zip(got, want, ("r", "s", "recid")):
        assert np.array_equal(a, b), f
    # one party's secrets per object: the rows of `own` are picked out of the sealed shares
    g1 = E.Gg20Keys(gpu_ctx, T, N_PARTIES, signers, sealed["arrays"], nkeysets=WALLETS, own=[2], sealed_shares=sealed["sealed_shares"], wrap=wk)
    g1.close()


def test_one_flipped_bit_fails_the_call_and_creates_nothing(gpu_ctx, made):
    from multi_party_ecdsa_amd import _native as N
    from multi_party_ecdsa_amd import engine as E
    wk, clear, sealed = made
    other = E.WrapKey(gpu_ctx, SC.OTHER_KEY)
    for word, key in ((PS.HEAD + 3, wk), (PS.HEAD + 72, wk), (1, wk), (None, other)):
        sh = sealed["sealed_shares"].copy()
        if word is not None:
            sh[4, word] ^= np.uint32(1 << 7)                               # wallet 1, party 1
        gk = None
        with pytest.raises(N.MpeError, match="rc=-1.*refused"):
            gk = E.Gg20Keys(gpu_ctx, T, N_PARTIES, [0, 2], sealed["arrays"], nkeysets=WALLETS, sealed_shares=sh, wrap=key)
        assert gk is None
    other.close()
