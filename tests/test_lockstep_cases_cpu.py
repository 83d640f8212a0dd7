"""The case table of tests/lockstep_cases.py against the oracle ALONE: the conditions without which the GPU tests of
tests/test_lockstep_failures_gpu.py would be vacuous (a table whose sessions all sign, or all fail, or fail with one status only,
would pass there whatever the lock-step signer does with a verdict computed ahead).  Conditions on the inputs, checked against the
reference implementation; nothing here touches the product."""
import numpy as np
import pytest

import fixtures as F
import lockstep_cases as LC
import pyref


@pytest.fixture(scope="module")
def table(keys):
    bs = LC.batches(keys)
    return {nm: (bt, LC.expected(bt)) for nm, bt in bs.items()}


def test_the_table_reaches_every_status_the_gpu_tests_are_about(table):
    seen = set()
    for bt, want in table.values():
        seen |= {int(x) for x in want["status"]}
    assert {0, 91, 101, 201, 202, 301, 602} <= seen, sorted(seen)
    # the key-borne failures hit single sessions of ONE launch; every recipe of the two-signer table sits in a session of its own
    assert {0, 101, 202, 602} <= {int(x) for x in table["multi-wallet"][1]["status"]}
    two = table["two signers"][0]
    assert sorted(two.recipes.values()) == sorted(LC.TWO_SIGNER_RECIPES) and len(set(two.recipes)) == len(LC.TWO_SIGNER_RECIPES)
    assert {91, 101, 201, 301} <= {int(x) for x in table["two signers"][1]["status"]}
    # three signers: the 91 party is refused by BOTH peers, the non-unit ciphertext is judged by both
    ps = table["three signers"][1]["party_status"]
    assert sorted(int(x) for x in ps[:, 1]) == [91, 101, 101] and sorted(int(x) for x in ps[:, 3])[:2] == [101, 101]
    # the sampler's give-up path: some sessions of the batch, not all
    st = table["sampled"][1]["status"]
    assert 0 < int((st == 91).sum()) < st.shape[0] and LC.sampled_batch(F.load_keys())[2] > 0


def test_at_least_half_of_every_batch_signs_and_failing_sessions_have_clean_neighbours(table):
    assert set(LC.EXEMPT) <= set(table)
    for nm, (bt, want) in table.items():
        st = [int(x) for x in want["status"]]
        assert len(st) == bt.B
        # a session marked degenerate that signs (the wide pdl_alpha) counts as clean; a session that fails must be a marked one —
        # except in the sampled batch, whose give-ups come from the seed
        assert nm == "sampled" or all(b in bt.recipes for b in range(bt.B) if st[b]), nm
        if nm in LC.EXEMPT:
            continue
        assert 2 * sum(1 for x in st if x == 0) >= bt.B, (nm, st)
        for b in range(bt.B):
            if st[b]:
                assert (b == 0 or st[b - 1] == 0) and (b == bt.B - 1 or st[b + 1] == 0), (nm, b, st)


def test_the_two_exempt_batches_are_what_their_names_say(table):
    bt, want = table["every session fails"]
    assert all(int(x) != 0 for x in want["status"])
    bt, want = table["chunking"]
    c = bt.kw["chunk"]
    chunks = [[int(x) for x in want["status"][i:i + c]] for i in range(0, bt.B, c)]
    assert any(all(ch) for ch in chunks) and any(not any(ch) for ch in chunks[:-1]) and 0 < len(chunks[-1]) < c and any(chunks[-1])
    assert any(any(ch) and not all(ch) for ch in chunks)


def test_failed_sessions_have_no_signature_in_the_oracles_output(table):
    for nm, (bt, want) in table.items():
        bad = [b for b in range(bt.B) if want["status"][b]]
        assert not want["r"][bad].any() and not want["s"][bad].any() and not want["recid"][bad].any(), nm


def test_clean_sessions_verify_under_the_wallets_public_key(table):
    for nm, (bt, want) in table.items():
        for b in range(bt.B):
            if want["status"][b] == 0:
                m, r, s = (F.ints(a[b:b + 1])[0] for a in (bt.nonces["msg"], want["r"], want["s"]))
                assert pyref.ecdsa_verify(bt.public_key(b), m, r, s), (nm, b)


def test_the_fullsize_sample_holds_every_failing_session_and_both_its_neighbours():
    pick = LC.fullsize_sample()
    for b in LC.FULLSIZE_FAILING:
        assert {x for x in (b - 1, b, b + 1) if 0 <= x < LC.FULLSIZE_B} <= set(pick)
    assert pick == sorted(set(pick)) and len(pick) < LC.FULLSIZE_B // 8
    assert np.all(np.diff(pick) > 0)
