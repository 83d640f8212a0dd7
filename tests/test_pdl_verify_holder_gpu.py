"""GPU: `mpe_pdl_verify` called by the HOLDER of the Paillier keys.  Where the call runs on one stream (a large batch, or a context
without forks: conftest's gpu_ctx_serial), a key object created with its primes sends the N^2 side of every item,
s2^N (c^-1)^e mod N^2, through p^2 | q^2 (mpe_paillier.h modexp_nn2_holder); a public key object, a private one on a context with the
option no_r5_self_crt, and a small batch on a default context (forked streams) keep the public ladders.  The ok flags must be the
same whichever route runs, and equal to the oracle's — on honest proofs from `pdl_prove` (whose acceptance needs the exact residue)
and on hostile s2 and c.  The profiler's launch records say which route ran.  64 items over 3 keys and 3 statements."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import fixtures as F
import orc
import pyref

pytestmark = pytest.mark.gpu

B = 64
NK = 3


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _npw(t):
    return np.ascontiguousarray(t.cpu().numpy().view(np.uint32))


def _oracle_verdicts(tabs, kidx, sidx, cw, Qw, Gw, pr):
    """orc.pdl_verify over the batch, eight items per host thread"""
    def part(lo):
        sl = slice(lo, lo + 8)
        return list(orc.pdl_verify(tabs["N"], tabs["Nt"], tabs["h1"], tabs["h2"], kidx[sl], sidx[sl], np.ascontiguousarray(cw[sl]),
                                   np.ascontiguousarray(Qw[sl]), np.ascontiguousarray(Gw[sl]), {f: np.ascontiguousarray(v[sl]) for f, v in pr.items()}))
    with ThreadPoolExecutor(8) as ex:
        return [int(v) for chunk in ex.map(part, range(0, B, 8)) for v in chunk]


@pytest.fixture(scope="module")
def case(gpu_ctx, keys):
    """honest proofs from pdl_prove (rows 0-1: nonces beta that are multiples of p and of q, so that an ACCEPTED proof has
    s2 = 0 mod p | q), the hostile values written over rows 8-14 (s2) and 20-24 (c); the oracle's verdicts, computed once"""
    from multi_party_ecdsa_amd import engine as E
    r = F.Rng("pdl-holder")
    ks = keys[:NK]
    kidx, sidx = [i % NK for i in range(B)], [(i // 5) % 3 for i in range(B)]
    tabs = dict(N=F.words([k.N for k in ks], 64), Nt=F.words([k.Nt for k in keys[4:7]], 64),
                h1=F.words([k.h1 for k in keys[4:7]], 64), h2=F.words([k.h2 for k in keys[4:7]], 64))
    x = [r.below(pyref.Q) for _ in range(B)]
    rr = [1 + r.below(keys[k].N - 1) for k in kidx]
    G = [pyref.ec_mul(1 + r.below(pyref.Q - 1), pyref.G) for _ in range(B)]
    Qp = [pyref.ec_mul(xx, g) for xx, g in zip(x, G)]
    c = [pyref.paillier_encrypt(keys[k].N, xx, y) for k, xx, y in zip(kidx, x, rr)]
    nn = [F.pdl_nonces(r, keys[k], keys[4 + s]) for k, s in zip(kidx, sidx)]
    nn[0]["beta"] = keys[kidx[0]].p * (1 + r.below(keys[kidx[0]].q - 1))
    nn[1]["beta"] = keys[kidx[1]].q * (1 + r.below(keys[kidx[1]].p - 1))
    nw = {f: F.words([n[f] for n in nn], w) for f, w in E.PDL_NONCE_WORDS.items()}
    cw, Qw, Gw = F.words(c, 128), F.point_words(Qp), F.point_words(G)
    ctx = gpu_ctx
    pk = E.PaillierKeys(ctx, p=[k.p for k in ks], q=[k.q for k in ks])
    stm = E.Statements(ctx, [k.Nt for k in keys[4:7]], [k.h1 for k in keys[4:7]], [k.h2 for k in keys[4:7]])
    di = lambda v: torch.tensor(v, dtype=torch.int32, device=ctx.device)
    pr = E.pdl_prove(ctx, pk, stm, _dev(ctx, cw), _dev(ctx, Qw), _dev(ctx, Gw), E.dev(ctx, x, 8), E.dev(ctx, rr, 64),
                     {f: _dev(ctx, v) for f, v in nw.items()}, di(kidx), di(sidx))
    ctx.sync()
    pr = {f: _npw(v) for f, v in pr.items()}
    stm.close()
    pk.close()
    s2 = F.ints(pr["s2"][:2])
    assert s2[0] % keys[kidx[0]].p == 0 and s2[1] % keys[kidx[1]].q == 0
    # s2 in {0, 1, p, q, N - 1, N, 2^2048 - 1}, c in {0, p, a multiple of q, N^2 - 1}, and a c that is not invertible
    K = lambda i: keys[kidx[i]]
    s2_vals = [lambda k: 0, lambda k: 1, lambda k: k.p, lambda k: k.q, lambda k: k.N - 1, lambda k: k.N, lambda k: (1 << 2048) - 1]
    for j, v in enumerate(s2_vals):
        pr["s2"][8 + j] = F.words([v(K(8 + j))], 64)[0]
    c_vals = [lambda k: 0, lambda k: k.p, lambda k: k.q * (1 + r.below(k.N)), lambda k: k.N * k.N - 1, lambda k: k.N * 3]
    for j, v in enumerate(c_vals):
        cw[20 + j] = F.words([v(K(20 + j))], 128)[0]
    hostile = list(range(8, 8 + len(s2_vals))) + list(range(20, 20 + len(c_vals)))
    want = _oracle_verdicts(tabs, kidx, sidx, cw, Qw, Gw, pr)
    assert [want[i] for i in range(B) if i not in hostile] == [1] * (B - len(hostile))          # rows 0 and 1 among them
    assert want[23] == 0 and want[24] == 0                       # c = N^2 - 1 is a unit but not the statement's; 3 N is not a unit
    return dict(kidx=kidx, sidx=sidx, c=cw, pr=pr, want=want, Q=Qw, G=Gw, rows=hostile)


def _verdicts(ctx, keys, case, private, options=None):
    """(ok flags, number of holder's two-base ladders mod p^2 | q^2 among the call's launch records: kind 3, 2048 bits, exp2_words 8)"""
    from multi_party_ecdsa_amd import engine as E
    if options:
        ctx = E.Context(0, options=options)
    ks = keys[:NK]
    pk = E.PaillierKeys(ctx, p=[k.p for k in ks], q=[k.q for k in ks]) if private else E.PaillierKeys(ctx, N=[k.N for k in ks])
    stm = E.Statements(ctx, [k.Nt for k in keys[4:7]], [k.h1 for k in keys[4:7]], [k.h2 for k in keys[4:7]])
    di = lambda v: torch.tensor(v, dtype=torch.int32, device=ctx.device)
    args = (_dev(ctx, case["c"]), _dev(ctx, case["Q"]), _dev(ctx, case["G"]), {f: _dev(ctx, v) for f, v in case["pr"].items()},
            di(case["kidx"]), di(case["sidx"]))
    ctx.sync()
    ctx.prof_enable(True)
    try:
        ok = E.pdl_verify(ctx, pk, stm, *args)
        ctx.sync()
        recs = ctx.prof_collect(4096)
    finally:
        ctx.prof_enable(False)
    holder = [r for r in recs if r["kind"] == 3 and r["bits"] == 2048 and r["exp2_words"] == 8]
    assert all(r["batch"] == 2 * B for r in holder), holder
    out = [int(v) for v in ok.cpu().numpy()]
    stm.close()
    pk.close()
    return out, len(holder)


@pytest.mark.parametrize("path", ["small_batch", "large_batch"])
def test_holder_and_public_key_objects_give_the_oracles_verdicts(gpu_ctx, gpu_ctx_serial, keys, case, path):
    ctx = gpu_ctx if path == "small_batch" else gpu_ctx_serial
    assert ctx.get_option("no_r5_self_crt") == 0
    holder, nh = _verdicts(ctx, keys, case, private=True)
    public, np_ = _verdicts(ctx, keys, case, private=False)
    print(path, "hostile rows", case["rows"], "holder", [holder[i] for i in case["rows"]], "oracle", [case["want"][i] for i in case["rows"]])
    assert (nh, np_) == ((1, 0) if path == "large_batch" else (0, 0))          # the holder's route runs where the call has one stream
    assert holder == case["want"]
    assert public == case["want"]


def test_the_option_sends_a_private_key_object_back_to_the_public_route(keys, case):
    ok, nh = _verdicts(None, keys, case, private=True, options={"no_par": 1, "no_adaptive_lanes": 1, "no_r5_self_crt": 1})
    assert nh == 0 and ok == case["want"]
