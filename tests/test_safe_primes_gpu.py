"""GPU: mpe_sample_safe_prime / mpe_paillier_keygen_safe_primes / mpe_ntilde_generate_safe_primes and gg20_keygen(safe_primes=True)
against the restatement tests/pyref_safe_primes.py, whose results for the cases below are recorded in
tests/golden/safe_primes_expected.json (tests/golden/make_safe_primes.py; checked against the restatement by
tests/test_safe_primes_cpu.py): a safe prime costs ~380 000 attempts, seconds of Python each."""
import contextlib
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import fixtures as F
import orc
import pyref_primes as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(HERE, "golden", "safe_primes_expected.json")) as f:
        return json.load(f)


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _ints(t):
    return F.ints(t.cpu().numpy().view(np.uint32))


@contextlib.contextmanager
def _pass_log(ctx, lg):
    """the search under another pass size (option safe_pass_log), the default put back afterwards"""
    default = ctx.get_option("safe_pass_log")
    ctx.set_option("safe_pass_log", lg)
    try:
        yield
    finally:
        ctx.set_option("safe_pass_log", default)


def _search(ctx, case, batch, pass_log, **kw):
    from multi_party_ecdsa_amd import engine as E
    with _pass_log(ctx, pass_log):
        out, attempt, fail = E.sample_safe_prime(ctx, batch, bytes.fromhex(case["seed"]), case["sid"], **kw)
        ctx.sync()
    return _ints(out), list(attempt.cpu().numpy()), int(fail.cpu()[0])


# Attempts per item and pass are the largest power of two with items * attempts <= 2^safe_pass_log, at most 2^20.  At the default (24)
# every batch below takes 2^20 attempts per item and the fixture's winners (all below 2^20) fall into ONE pass; the smaller pass sizes
# are what makes items finish in different passes, the item list shrink, a0 advance and the block size grow from pass to pass.
@pytest.mark.parametrize("pass_log", [24, 20])
def test_search_parity(gpu_ctx, want, pass_log):
    """7 items, default cap: every safe prime and every attempt index is the restatement's.  pass_log 20: 2^17 attempts per item in the
    first pass; the winners (attempt ~2^14 .. ~2^19.5) finish in passes 1, 1, 1, 2, 3, 3 and 4, the block growing as items leave"""
    s = want["search"]
    assert sum(a <= 1 << 17 for a in s["attempts"]) >= 2 and max(s["attempts"]) >= 1 << 19
    primes, attempts, fail = _search(gpu_ctx, s, s["batch"], pass_log)
    assert attempts == s["attempts"]
    assert primes == [int(v, 16) for v in s["primes"]]
    assert fail == 0


@pytest.mark.parametrize("batch,pass_log", [(1, 24), (2, 24), (1, 16), (2, 16), (3, 20)])
def test_smaller_batches_equal_the_prefix(gpu_ctx, want, batch, pass_log):
    """the result of an item depends neither on the batch nor on the pass size: one pass of 2^20 attempts per item at the default;
    2^16 attempts per pass for a lone item (12 passes to its winner); 2^15 for two (item 1 leaves in pass 13, then 2^16: 18 passes);
    2^18 for three (two passes, the second of 2^19 for the two items left)"""
    s = want["search"]
    primes, attempts, fail = _search(gpu_ctx, s, batch, pass_log)
    assert attempts == s["attempts"][:batch] and primes == [int(v, 16) for v in s["primes"][:batch]] and fail == 0


@pytest.mark.parametrize("pass_log", [24, 20, 16])
def test_search_gives_up(gpu_ctx, want, pass_log):
    """max_attempts = 2^18 cuts the first pass short at the default; at pass_log 20 it is the end of the second pass, at 16 of the 22nd (three items have left by then)"""
    u = want["giveup"]
    assert 0 < u["fail"] < u["batch"]
    primes, attempts, fail = _search(gpu_ctx, u, u["batch"], pass_log, max_attempts=u["max_attempts"])
    assert attempts == u["attempts"]
    assert primes == [int(v, 16) for v in u["primes"]]                    # zero rows where the attempt is -1
    assert fail == u["fail"]


def test_bad_arguments_are_refused_with_a_context(gpu_ctx):
    """with a live context the range checks themselves answer (without one, the NULL context does: tests/test_safe_primes_cpu.py)"""
    from multi_party_ecdsa_amd import _native as N
    from multi_party_ecdsa_amd import engine as E
    seed = b"safe-primes-arguments".ljust(32, b".")
    for kw in (dict(bits=512), dict(bits=2048), dict(max_attempts=-1), dict(max_attempts=(1 << 24) + 1)):
        with pytest.raises(N.MpeError):
            E.sample_safe_prime(gpu_ctx, 1, seed, 0, **kw)
    for fn in (E.paillier_keygen, E.ntilde_generate):
        for counter, cap in ((1 << 56, 0), (0, -1), (0, (1 << 24) + 1)):
            with pytest.raises(N.MpeError):
                fn(gpu_ctx, 1, seed, counter, max_attempts=cap, safe_primes=True)
    for lg in (15, 27):
        with pytest.raises(N.MpeError):
            gpu_ctx.set_option("safe_pass_log", lg)
    assert gpu_ctx.get_option("safe_pass_log") == 24


def test_paillier_keygen_safe_primes(gpu_ctx, want):
    from multi_party_ecdsa_amd import engine as E
    k = want["keygen"]
    p, q, n, fail = E.paillier_keygen(gpu_ctx, k["nkeys"], bytes.fromhex(k["seed"]), k["counter"], safe_primes=True)
    gpu_ctx.sync()
    P, Q, N = _ints(p), _ints(q), _ints(n)
    assert P == [int(v, 16) for v in k["p"]] and Q == [int(v, 16) for v in k["q"]]
    assert N == [a * b for a, b in zip(P, Q)] == [int(v, 16) for v in k["N"]] and int(fail.cpu()[0]) == 0
    sk = E.PaillierKeys(gpu_ctx, p=p, q=q)
    r = F.Rng("safe-primes-paillier")
    idx = [i % k["nkeys"] for i in range(16)]
    m = [r.below(N[i]) for i in idx]
    rr = [r.below(N[i]) for i in idx]
    c = sk.encrypt(m, rr, key_idx=idx)
    Nw, Pw, Qw = F.words(N, 64), F.words(P, 32), F.words(Q, 32)
    assert c == F.ints(orc.paillier_encrypt(Nw, F.words(m, 64), F.words(rr, 64), idx))
    assert sk.decrypt(c, key_idx=idx) == m == F.ints(orc.paillier_decrypt(Pw, Qw, F.words(c, 128), idx))
    sigma = E.correct_key_prove(gpu_ctx, sk)
    ok = E.correct_key_verify(gpu_ctx, n, sigma)
    assert list(ok.cpu().numpy()) == [1] * k["nkeys"]


def test_ntilde_generate_safe_primes(gpu_ctx, want):
    from multi_party_ecdsa_amd import engine as E
    n = want["ntilde"]
    o = E.ntilde_generate(gpu_ctx, n["count"], bytes.fromhex(n["seed"]), n["counter"], safe_primes=True)
    gpu_ctx.sync()
    got = {f: _ints(o[f]) for f in ("Nt", "h1", "h2", "xhi", "xhi_inv")}
    for f, v in got.items():
        assert v == [int(x, 16) for x in n[f]], f
    assert int(o["fail"].cpu()[0]) == n["fail"] == 0
    r = F.Rng("safe-primes-ntilde")
    nonce = _dev(gpu_ctx, F.words([r.bits(512) for _ in range(n["count"])], 16))
    for g, ni, sec in ((o["h1"], o["h2"], o["xhi"]), (o["h2"], o["h1"], o["xhi_inv"])):
        x, y = E.composite_dlog_prove(gpu_ctx, o["Nt"], g, ni, sec, nonce)
        assert list(E.composite_dlog_verify(gpu_ctx, o["Nt"], g, ni, x, y).cpu().numpy()) == [1] * n["count"]


def test_gg20_keygen_safe_primes_makes_a_wallet_that_signs(gpu_ctx):
    """`Keys::create_safe_prime` for the three parties of one wallet: 6 safe primes at a batch of 3"""
    from multi_party_ecdsa_amd import engine as E
    import ossl
    t, n, B = 1, 3, 1
    seed, counter = b"\x33" * 32, 4
    res = E.gg20_keygen(gpu_ctx, t, n, B, seed, counter=counter, safe_primes=True)
    assert list(res["ok"].cpu().numpy()) == [1] and res["failures"] == 0
    assert list(res["bad1"].cpu().numpy()) == [0] == list(res["bad3"].cpu().numpy()) and not res["bad2"].cpu().numpy().any()
    a = res["arrays"]
    p, q, N, fail = E.paillier_keygen(gpu_ctx, n, seed, counter, safe_primes=True)
    gpu_ctx.sync()
    assert int(fail.cpu()[0]) == 0
    for f, t_ in (("p", p), ("q", q), ("N", N)):
        assert np.array_equal(np.asarray(a[f]).view(np.uint32).reshape(n, -1), t_.cpu().numpy().view(np.uint32)), f
    primes = _ints(p) + _ints(q)
    both = primes + [(c - 1) // 2 for c in primes]
    assert list(E.is_probable_prime(gpu_ctx, _dev(gpu_ctx, F.words(both, 32))).cpu().numpy()) == [1] * len(both)
    assert all(R.is_prime(v) for v in both) and len(set(primes)) == 2 * n
    # one signing session over the wallet
    msg = F.words([int.from_bytes(hashlib.sha256(b"safe-prime wallet").digest(), "big")], 8)
    gk = E.Gg20Keys(gpu_ctx, t, n, [0, 2], a, nkeysets=B)
    keyset = torch.zeros((1,), dtype=torch.int32, device=gpu_ctx.device)
    nonces, nfail = E.gg20_sample_nonces(gpu_ctx, gk, 1, b"\x5b" * 32, 200, keyset=keyset, msg=_dev(gpu_ctx, msg))
    r, s, recid, status = E.gg20_sign(gpu_ctx, gk, nonces, 1, keyset=keyset)
    gpu_ctx.sync()
    assert int(nfail.item()) == 0 and list(status.cpu().numpy()) == [0]
    assert ossl.ecdsa_verify(a["y"][0], msg, r.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint32)).all()
    gk.close()


def test_scratch_is_clean_after_safe_search_and_wipe(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    E.sample_safe_prime(gpu_ctx, 3, b"safe-primes-hygiene".ljust(32, b"."), 3, max_attempts=4096)
    gpu_ctx.sync()
    assert gpu_ctx.scratch_audit()[0] > 0                                 # the search leaves its lists behind ...
    gpu_ctx.wipe()
    assert gpu_ctx.scratch_audit()[0] == 0                                # ... and the wipe covers them
