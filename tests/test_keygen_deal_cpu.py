"""CPU: the pure-Python restatement of the dealing side of keygen and of its round-3 verdict (tests/keygen_deal_cases.py) against the
oracle's existing pieces, the literal verdict lists of its case tables, and the three new entry points at the ABI boundary."""
import ctypes
import os
import re

import numpy as np
import pytest

import fixtures as F
import keygen_deal_cases as KD
import orc
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mpe_vss_share", "mpe_keygen_construct_keypair", "mpe_keygen_verify_round3"]


@pytest.mark.parametrize("t,n", KD.DEAL_SHAPES)
def test_every_dealt_share_passes_the_oracles_validate_share(t, n):
    c = KD.deal_case(t, n)
    B = KD.DEAL_BATCH
    commits = np.ascontiguousarray(np.repeat(c["commits"], n, axis=0))                   # one row of commitments per (dealer, receiver)
    index = np.array([j + 1 for _ in range(B) for j in range(n)], dtype=np.int32)
    ok = np.zeros(B * n, dtype=np.uint8)
    orc.lib.orc_vss_validate_share(B * n, t + 1, orc._p(commits), orc._p(np.ascontiguousarray(c["shares"].reshape(B * n, 8))), orc._p(index), orc._p(ok))
    assert list(ok) == [1] * (B * n)          # the oracle takes a neutral row as the point it is; the device refuses it (c["valid"], mpecdsa_hip.h)
    assert c["valid"].count(0) == n and not any(c["valid"][KD.DEAL_ZERO_DEALER * n:(KD.DEAL_ZERO_DEALER + 1) * n])
    # the special rows are what they claim to be
    assert F.ints(c["commits"][0:1, :16]) == F.ints(F.point_words([pyref.G]))
    assert F.points(c["commits"][KD.DEAL_ZERO_DEALER, t * 16:(t + 1) * 16].reshape(1, 16)) == [None]
    assert F.ints(c["coef"][2:3, :8])[0] >= pyref.Q


@pytest.mark.parametrize("n", KD.CONSTRUCT_SHAPES)
def test_construct_cases_hold_their_edge_rows_and_their_proofs_verify(n):
    c = KD.construct_case(n)
    x, pk, ysum = F.ints(c["x"]), F.points(c["pk"]), F.points(c["ysum"])
    assert x[0] == (n * (pyref.Q - 1)) % pyref.Q and x[1] == 0 and pk[1] is None
    ys = F.points(c["y"].reshape(-1, 16))
    assert ys[2 * n] == ys[2 * n + 1] and ys[3 * n + 1] == pyref.ec_neg(ys[3 * n]) and ysum[4] is None
    keep = [i for i in range(KD.CONSTRUCT_BATCH) if i != 1]                                # the neutral pk: refused by the device as a point
    ok = orc.dlog_verify(np.ascontiguousarray(c["pk"][keep]), np.ascontiguousarray(c["R"][keep]), np.ascontiguousarray(c["z"][keep]))
    assert list(ok) == [1] * len(keep)
    assert not KD.dlog_verify(pk[1], F.points(c["R"])[1], F.ints(c["z"])[1])
    for i in (0, 2, 3, 4, 66):
        acc = None
        for p in ys[i * n:(i + 1) * n]:
            acc = pyref.ec_add(acc, p)
        assert acc == ysum[i]


@pytest.mark.parametrize("t,n", sorted(KD.ROUND3_WANT))
def test_round3_tables_yield_the_literal_verdicts_and_agree_with_the_oracle(t, n):
    c = KD.round3_case(t, n)
    want_ok, want_bad = KD.ROUND3_WANT[(t, n)]
    assert c["ok"] == want_ok and c["bad"] == want_bad
    S, t1 = len(want_bad), t + 1
    # xi_commit == the sum over the dealers of the oracle's get_point_commitment, for every session whose commitments are points
    bad_s = KD.ROUND3_OFFCURVE_SESSION[(t, n)]
    items, index = [], []
    for s in range(S):
        for i in range(n):
            for j in range(n):
                items.append(c["commits"][s * n + j])
                index.append(i + 1)
    out = orc.u32((len(items), 16))
    orc.lib.orc_vss_point_commitment(len(items), t1, orc._p(np.ascontiguousarray(np.stack(items))), orc._p(np.array(index, dtype=np.int32)), orc._p(out))
    pts = F.points(out)
    xi = F.points(c["xi"])
    for s in range(S):
        for i in range(n):
            if s == bad_s:
                assert xi[s * n + i] is None
                continue
            acc = None
            for j in range(n):
                acc = pyref.ec_add(acc, pts[(s * n + i) * n + j])
            assert acc == xi[s * n + i], (s, i)
    # DLogProof::verify alone: the oracle accepts the foreign and the swapped proofs the VSS comparison refuses
    dl = list(orc.dlog_verify(c["pk"], c["R"], c["z"]))
    if (t, n) == (1, 3):
        assert dl == [1, 1, 1,  1, 0, 1,  1, 1, 1,  1, 1, 1,  1, 1, 1,  1, 1, 1,  1, 1, 1,  0, 1, 1]
    else:
        assert dl == [1, 1, 1, 1, 1,  1, 0, 1, 1, 0,  1, 1, 1, 1, 1,  1, 1, 1, 1, 1]


def test_the_three_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mpecdsa_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mpe_[a-z0-9_]+)\s*\(", hdr))
    from multi_party_ecdsa_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED and getattr(_native.lib, name).argtypes is not None, name
    from multi_party_ecdsa_amd import engine as E
    for f in ("vss_share", "keygen_construct_keypair", "keygen_verify_round3", "gg20_keygen"):
        assert callable(getattr(E, f))


def test_lagrange_helper_reconstructs_a_shared_secret():
    coef = [12345, 678]
    _, shares = KD.vss_share(coef, 3)
    assert KD.lagrange_at_zero(shares, [0, 1]) == KD.lagrange_at_zero(shares, [1, 2]) == KD.lagrange_at_zero(shares, [0, 2]) == 12345
