"""Per-session signer sets, the parts that need no GPU: the packing of a set into one word (multi_party_ecdsa_amd/words.py, imported
without the native library), the rank-of-party rule of a local party named by its index, and the sanity of the oracle expectation the
GPU tests compare against (tests/sigset_cases.py)."""
import itertools

import numpy as np
import pytest

import gg20_fixture as G
import ossl
import sigset_cases as SC

W = SC.words


@pytest.mark.parametrize("t,n", [(1, 3), (2, 5), (3, 8)])
def test_packing_round_trips_every_set(t, n):
    S = t + 1
    sets = SC.all_sets(n, S)
    assert len(sets) == {3: 3, 5: 10, 8: 70}[n]
    seen = set()
    for s in sets:
        word = W.pack_signer_set(s)
        assert W.unpack_signer_set(word, S) == s
        assert word < 1 << (4 * S)
        for i, p in enumerate(s):
            assert (word >> (4 * i)) & 15 == p                         # ordinal i in nibble i
        assert W.signer_set_mask(s) == sum(1 << p for p in s)
        seen.add(word)
    assert len(seen) == len(sets)
    table = W.signer_set_table(sets, n)
    assert table.shape == (len(sets), S) and table.dtype == np.int32 and [list(r) for r in table] == sets


def test_party_7_and_set_69_land_where_they_belong():
    sets = SC.all_sets(8, 4)
    assert sets[69] == [4, 5, 6, 7] and sets[35] == [1, 2, 3, 4]
    assert W.pack_signer_set(sets[69]) == 0x7654                       # party 7 is ordinal 3: the fourth nibble
    assert W.pack_signer_set([0, 1, 2, 3, 4, 5, 6, 7]) == 0x76543210
    table = W.signer_set_table(sets, 8)
    assert list(table[69]) == [4, 5, 6, 7] and table.shape == (70, 4)


@pytest.mark.parametrize("bad", [[1, 0], [0, 0], [0, 8], [-1, 2], []])
def test_packing_refuses_what_the_library_refuses(bad):
    with pytest.raises(ValueError):
        W.pack_signer_set(bad)


def test_table_refuses_duplicates_ragged_rows_and_parties_beyond_n():
    with pytest.raises(ValueError):
        W.signer_set_table([[0, 1], [0, 2], [0, 1]], 3)
    with pytest.raises(ValueError):
        W.signer_set_table([[0, 1], [0, 1, 2]], 3)
    with pytest.raises(ValueError):
        W.signer_set_table([[0, 3]], 3)
    with pytest.raises(ValueError):
        W.signer_set_table([[0, 1]] * 0, 3)


@pytest.mark.parametrize("n,S", [(3, 2), (5, 3), (8, 4)])
def test_rank_of_party_is_its_position_in_the_ascending_set(n, S):
    for s in itertools.combinations(range(n), S):
        for p in range(n):
            want = sorted(s).index(p) if p in s else -1                # the plain restatement
            assert W.rank_in_set(list(s), p) == want


@pytest.fixture(scope="module")
def mixed13(keys):
    t, n, sets = 1, 3, SC.all_sets(3, 2)
    sigset = [0, 1, 2, 2, 0, 1, 1]
    lks, per_wallet = SC.wallet(keys, t, n, sets)
    nonces = SC.mixed_nonces(per_wallet, sigset, seed="sigsets-cpu")
    return lks, per_wallet, nonces, sigset, SC.oracle_mixed(lks, nonces, sigset)


def test_the_oracle_expectation_of_a_mixed_batch_signs_under_the_wallets_key(mixed13):
    """every session has status 0 and a signature OpenSSL accepts under y: the Lagrange weights at each set's own indices sum the
    shares to x"""
    lks, _, nonces, sigset, want = mixed13
    assert not want["status"].any() and not want["party_status"].any() and not want["party_bad"].any()
    for lk in lks[1:]:
        assert np.array_equal(lk["arrays"]["y"], lks[0]["arrays"]["y"]) and np.array_equal(lk["arrays"]["x"], lks[0]["arrays"]["x"])
    assert ossl.ecdsa_verify(lks[0]["arrays"]["y"][0], nonces["msg"], want["r"], want["s"]).all()
    for rnd in G.ROUNDS:
        assert want["slabs"][rnd].any(axis=(0, 2)).all(), f"round {rnd}: a session left no record"


def test_a_session_equals_the_uniform_run_of_its_set(mixed13):
    """row b of the mixed expectation is row b of the oracle's uniform run with that set on the nonces drawn for that set"""
    lks, per_wallet, nonces, sigset, want = mixed13
    B = len(sigset)
    for k in range(len(lks)):
        uni = G.oracle_sign_ex(lks[k], G.make_nonces(lks[k], B, seed="sigsets-cpu"), B)
        for b in [b for b in range(B) if sigset[b] == k]:
            assert np.array_equal(uni["r"][b], want["r"][b]) and np.array_equal(uni["s"][b], want["s"][b])
            for rnd in G.ROUNDS:
                assert np.array_equal(uni["slabs"][rnd][:, b], want["slabs"][rnd][:, b])


def test_the_same_party_in_two_sets_uses_two_different_w_i(keys):
    """party 0 is ordinal 0 of {0, 1} and of {0, 2}: with the same nonce seed its w_i = lambda_i x_i differs, and with it the
    b_proof.pk = w_i G of round 1's WI MessageB"""
    t, n, sets = 1, 3, SC.all_sets(3, 2)
    lks, per_wallet = SC.wallet(keys, t, n, sets)
    B = 2
    pk = SC.wire.field("M1", "b_pk", 1 * SC.wire.SUB1)                 # sub-record 2 jj + v = 1: the w_i MessageB to the only peer
    runs = [G.oracle_sign_ex(lks[k], G.make_nonces(lks[k], B, seed="same-seed"), B) for k in (0, 1)]
    for b in range(B):
        a, c = runs[0]["slabs"][1][0, b, pk], runs[1]["slabs"][1][0, b, pk]
        assert a.any() and c.any() and not np.array_equal(a, c)
