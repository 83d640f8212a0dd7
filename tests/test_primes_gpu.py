"""GPU: mpe_is_probable_prime / mpe_sample_prime / mpe_paillier_keygen / mpe_ntilde_generate against the pure-Python restatement
tests/pyref_primes.py.  Its results for the cases below are recorded in tests/golden/primes_expected.json (tests/golden/make_primes.py;
checked against the restatement by tests/test_primes_cpu.py): a 1024-bit exponentiation costs Python ~3 ms, the cases ~10 000 of them."""
import json
import os

import numpy as np
import pytest
import torch

import fixtures as F
import orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(HERE, "golden", "primes_expected.json")) as f:
        return json.load(f)


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _ints(t):
    return F.ints(t.cpu().numpy().view(np.uint32))


@pytest.fixture(scope="module")
def search(gpu_ctx, want):
    """the 67-item search, run once for the tests that look at it"""
    from multi_party_ecdsa_amd import engine as E
    s = want["search"]
    out, attempt, fail = E.sample_prime(gpu_ctx, s["batch"], bytes.fromhex(s["seed"]), s["sid"])
    gpu_ctx.sync()
    return _ints(out), list(attempt.cpu().numpy()), int(fail.cpu()[0])


@pytest.mark.parametrize("batch", [1, 33, 67])
def test_is_probable_prime_curated(gpu_ctx, want, batch):
    """batches that are no multiple of the 32 candidates of a wave: the 1024-bit primes of keys16.json; 0, 1, 2, 3, 6361, 6373, 6373^2,
    6367 * 6373 (just below 6370^2: the table alone decides); p^2 and p (2p - 1) for 511-bit primes p; a 1011-bit prime times 6373 and
    times 6361 (the Miller-Rabin side and the table side of the bound — a 1013-bit prime times 6373 would have 1026 bits and not
    fit the 1024-bit rows); a prime k 2^64 + 1 (large s); an even 1024-bit number; 2^1024 - 1"""
    from multi_party_ecdsa_amd import engine as E
    c = want["isprime"]
    vals, expect = [int(v, 16) for v in c["values"]], c["expect"]
    assert len(vals) == 49 and 0 < sum(expect) < len(expect)
    # batch 1: a prime, a composite on the Miller-Rabin side and the large-s prime, one call each; else the list (wrapped round) in chunks
    chunks = [[5], [44], [46]] if batch == 1 else [[i % 49 for i in range(lo, lo + batch)] for lo in range(0, 49, batch)]
    for idx in chunks:
        got = E.is_probable_prime(gpu_ctx, _dev(gpu_ctx, F.words([vals[i] for i in idx], 32)), rounds=8)
        assert list(got.cpu().numpy()) == [expect[i] for i in idx], (batch, idx[0])


def test_is_probable_prime_one_round_and_sixteen(gpu_ctx, want):
    from multi_party_ecdsa_amd import engine as E
    c = want["isprime"]
    d = _dev(gpu_ctx, F.words([int(v, 16) for v in c["values"]], 32))
    for rounds in (1, 16):
        assert list(E.is_probable_prime(gpu_ctx, d, rounds=rounds).cpu().numpy()) == c["expect"]


def test_search_parity(search, want):
    """67 items, default cap: every prime and every attempt index is the restatement's; the expected values hold an item won at
    attempt <= 8 and one at attempt >= 1500, so the search takes several passes whatever the block size"""
    s = want["search"]
    assert min(s["attempts"]) <= 8 and max(s["attempts"]) >= 1500
    primes, attempts, fail = search
    assert attempts == s["attempts"]
    assert primes == [int(v, 16) for v in s["primes"]]
    assert fail == 0


def test_search_gives_up(gpu_ctx, want):
    from multi_party_ecdsa_amd import engine as E
    u = want["giveup"]
    assert 0 < u["fail"] < u["batch"]
    out, attempt, fail = E.sample_prime(gpu_ctx, u["batch"], bytes.fromhex(u["seed"]), u["sid"], max_attempts=u["max_attempts"])
    gpu_ctx.sync()
    assert list(attempt.cpu().numpy()) == u["attempts"]
    assert _ints(out) == [int(v, 16) for v in u["primes"]]               # zero rows where the attempt is -1
    assert int(fail.cpu()[0]) == u["fail"]


def test_search_items_are_independent(gpu_ctx, want, search):
    from multi_party_ecdsa_amd import engine as E
    s = want["search"]
    out, attempt, _ = E.sample_prime(gpu_ctx, 5, bytes.fromhex(s["seed"]), s["sid"])
    gpu_ctx.sync()
    assert _ints(out) == search[0][:5] and list(attempt.cpu().numpy()) == search[1][:5]
    other, _, _ = E.sample_prime(gpu_ctx, 5, bytes.fromhex(s["seed"]), s["sid"] + 1)
    gpu_ctx.sync()
    assert not set(_ints(other)) & set(search[0])


def test_paillier_keygen(gpu_ctx, want):
    from multi_party_ecdsa_amd import engine as E
    k = want["keygen"]
    p, q, n, fail = E.paillier_keygen(gpu_ctx, k["nkeys"], bytes.fromhex(k["seed"]), k["counter"])
    gpu_ctx.sync()
    P, Q, N = _ints(p), _ints(q), _ints(n)
    assert P == [int(v, 16) for v in k["p"]] and Q == [int(v, 16) for v in k["q"]]
    assert N == [a * b for a, b in zip(P, Q)] and int(fail.cpu()[0]) == 0
    sk = E.PaillierKeys(gpu_ctx, p=p, q=q)                               # the existing private key object, from the device arrays
    r = F.Rng("primes-paillier")
    idx = [i % k["nkeys"] for i in range(64)]
    m = [r.below(N[i]) for i in idx]
    rr = [r.below(N[i]) for i in idx]
    c = sk.encrypt(m, rr, key_idx=idx)
    Nw, Pw, Qw = F.words(N, 64), F.words(P, 32), F.words(Q, 32)
    assert c == F.ints(orc.paillier_encrypt(Nw, F.words(m, 64), F.words(rr, 64), idx))
    assert sk.decrypt(c, key_idx=idx) == m == F.ints(orc.paillier_decrypt(Pw, Qw, F.words(c, 128), idx))
    sigma = E.correct_key_prove(gpu_ctx, sk)
    ok = E.correct_key_verify(gpu_ctx, n, sigma)
    assert list(ok.cpu().numpy()) == [1] * k["nkeys"]


def test_ntilde_generate(gpu_ctx, want):
    from multi_party_ecdsa_amd import engine as E
    n = want["ntilde"]
    o = E.ntilde_generate(gpu_ctx, n["count"], bytes.fromhex(n["seed"]), n["counter"])
    gpu_ctx.sync()
    got = {f: _ints(o[f]) for f in ("Nt", "h1", "h2", "xhi", "xhi_inv")}
    for f, v in got.items():
        assert v == [int(x, 16) for x in n[f]], f
    assert int(o["fail"].cpu()[0]) == n["fail"] == 0
    for i in range(n["count"]):                                          # on the host: xi xi^-1 = 1 (mod phi), h2 = h1^xi
        phi, xi = int(n["phi"][i], 16), int(n["xi"][i], 16)
        assert xi == phi - got["xhi"][i] and xi * (phi - got["xhi_inv"][i]) % phi == 1
        assert got["h2"][i] == pow(got["h1"][i], xi, got["Nt"][i])
    r = F.Rng("primes-ntilde")
    nonce = _dev(gpu_ctx, F.words([r.bits(512) for _ in range(n["count"])], 16))
    for g, ni, sec in ((o["h1"], o["h2"], o["xhi"]), (o["h2"], o["h1"], o["xhi_inv"])):
        x, y = E.composite_dlog_prove(gpu_ctx, o["Nt"], g, ni, sec, nonce)
        assert list(E.composite_dlog_verify(gpu_ctx, o["Nt"], g, ni, x, y).cpu().numpy()) == [1] * n["count"]
    stm = E.Statements(gpu_ctx, o["Nt"], o["h1"], o["h2"])               # the existing statement table takes the device arrays
    assert stm.count == n["count"]
    stm.close()


def test_scratch_is_clean_after_search_and_wipe(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    E.sample_prime(gpu_ctx, 9, b"primes-hygiene".ljust(32, b"."), 3, max_attempts=256)
    E.ntilde_generate(gpu_ctx, 2, b"primes-hygiene".ljust(32, b"."), 4)
    gpu_ctx.sync()
    assert gpu_ctx.scratch_audit()[0] > 0                                 # the search leaves its lists behind ...
    gpu_ctx.wipe()
    assert gpu_ctx.scratch_audit()[0] == 0                                # ... and the wipe covers them
