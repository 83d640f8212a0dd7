"""GPU: `mpe_gg20_sample_nonces_sets` — the device sampler for sessions that name their signer set.  Stream ids and item indices are
those of the uniform call; only the bound row an item reads follows the session's set.  So row b of a mixed draw equals row b of
today's uniform draw on a `Gg20Keys(signers=that set)` object under the same (seed, batch_counter)."""
import numpy as np
import pytest
import torch

import gg20_fixture as G
import sigset_cases as SC

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
COUNTER = 0x5e75


def hv(t):
    return t.cpu().numpy().view(np.uint32)


def _i32(ctx, vals):
    return torch.tensor([int(v) for v in vals], dtype=torch.int32, device=ctx.device)


def _rows(a, B, b):
    per = a.shape[0] // B
    return a.reshape(a.shape[0], -1)[b * per:(b + 1) * per]


@pytest.mark.parametrize("t,n,sigset", [(1, 3, [0, 1, 2, 2, 0, 1, 1]), (2, 5, [3, 9, 0, 7, 1, 8, 2, 6, 4, 5, 0])])
def test_row_b_of_a_mixed_draw_is_row_b_of_the_uniform_draw_with_that_set(gpu_ctx, keys, t, n, sigset):
    from multi_party_ecdsa_amd import engine as E
    ctx, S, B = gpu_ctx, t + 1, len(sigset)
    sets = SC.all_sets(n, S)
    lks, _ = SC.wallet(keys, t, n, sets)
    gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], signer_sets=sets)
    got, fail = E.gg20_sample_nonces(ctx, gk, B, SEED, COUNTER, sigset=_i32(ctx, sigset))
    assert int(fail.item()) == 0
    got = {f: hv(got[f]) for f in G.NONCE_FIELDS[:-1]}
    gk.close()
    differs = 0
    for k in sorted(set(sigset)):
        gu = E.Gg20Keys(ctx, t, n, sets[k], lks[k]["arrays"])
        uni, fail = E.gg20_sample_nonces(ctx, gu, B, SEED, COUNTER)
        assert int(fail.item()) == 0
        for f in G.NONCE_FIELDS[:-1]:
            u = hv(uni[f])
            for b in range(B):
                same = np.array_equal(_rows(got[f], B, b), _rows(u, B, b))
                if sigset[b] == k:
                    assert same, (f, b, k)
                else:
                    differs += not same
        gu.close()
    assert differs, "no field of any session depends on its signer set: the case shows nothing"


def test_one_party_by_index_draws_what_it_draws_in_lock_step(gpu_ctx, keys):
    """party 2 alone (local_party=2): its rows are the rows of its ordinal in the lock-step draw of each session's set"""
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, S, p = gpu_ctx, 1, 3, 2, 2
    sets = SC.all_sets(n, S)
    sigset = [1, 2, 2, 1, 2]                                      # the sets that hold party 2: {0, 2} and {1, 2}, ordinal 1 in both
    B = len(sigset)
    lks, _ = SC.wallet(keys, t, n, sets)
    gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], signer_sets=sets)
    ds = _i32(ctx, sigset)
    full, _ = E.gg20_sample_nonces(ctx, gk, B, SEED, COUNTER + 1, sigset=ds)
    mine, fail = E.gg20_sample_nonces(ctx, gk, B, SEED, COUNTER + 1, sigset=ds, local_party=p)
    assert int(fail.item()) == 0
    want = G.party_nonces({f: hv(full[f]) for f in G.NONCE_FIELDS[:-1]}, lks[1], 1)
    for f in G.NONCE_FIELDS[:-1]:
        assert np.array_equal(hv(mine[f]).reshape(want[f].shape), want[f]), f
    gk.close()
