"""GG18 signing without a GPU: the Python restatement (tests/pyref_gg18.py) signs at the reference's shapes and every signature passes
OpenSSL and pyref.ecdsa_verify; every row of the tamper / hostile table (tests/gg18_cases.py) gives its status code and the untouched
sessions beside it sign; the header declares the mpe_gg18_* calls and the built library exports them."""
import ctypes
import os
import re

import numpy as np
import pytest

import fixtures as F
import gg18_cases as K
import pyref as R
import pyref_gg18 as P18

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GG18_CALLS = ["mpe_gg18_sign_keys", "mpe_gg18_message_b", "mpe_gg18_phase2", "mpe_gg18_phase4", "mpe_gg18_phase5a", "mpe_gg18_phase5c",
              "mpe_gg18_phase5d", "mpe_gg18_output_signature"]


@pytest.fixture(scope="module")
def signed():
    """one session per shape, all three in one reference() call (they run side by side)"""
    shapes = ["t1n3", "t2n5", "t4n8"]
    res = K.reference([K.jobs_for(s, 1)[0] for s in shapes])
    return dict(zip(shapes, res))


@pytest.mark.parametrize("shape", ["t1n3", "t2n5", "t4n8"])       # (1, 3, [0, 2]); test.rs:50; test.rs:54
def test_restatement_signs(signed, shape):
    import ossl
    lk, w, signers = K.wallet(shape)
    res = signed[shape]
    assert res["status"] == [0] * len(signers)
    assert len(set(res["sig"])) == 1                                # every party outputs the same signature
    r, s, recid = res["sig"][0]
    assert 0 < s <= R.Q // 2 and recid in (0, 1)
    assert R.ecdsa_verify(w["y"], res["msg"] % R.Q, r, s)
    assert ossl.ecdsa_verify(lk["arrays"]["y"][0], F.words([res["msg"]], 8), F.words([r], 8), F.words([s], 8)).all()
    # the recovery id names R: x = r, parity of y as the flip rule left it
    Rp, s_sum = res["R"][0], sum(res["msgs"]["s_i"]) % R.Q
    assert Rp[0] % R.Q == r and s == min(s_sum, R.Q - s_sum) and recid == (Rp[1] & 1) ^ (s_sum > R.Q - s_sum)


def test_two_signer_session_is_the_mta_it_claims(signed):
    """delta = k gamma and sigma = k w over the sums: the MtA shares add up (party_i.rs:426-444)"""
    res = signed["t1n3"]
    _, w, signers = K.wallet("t1n3")
    d = res["draws"]
    k, gamma = sum(d["k"]) % R.Q, sum(d["gamma"]) % R.Q
    assert sum(res["msgs"]["delta"]) % R.Q == k * gamma % R.Q
    x = sum(res["state"]["w"]) % R.Q
    assert R.ec_mul(x, R.G) == w["y"]
    assert sum(res["state"]["sigma"]) % R.Q == k * x % R.Q


@pytest.fixture(scope="module")
def matrix():
    return K.matrix_plan(), K.reference(K.matrix_jobs())


def test_tamper_matrix_codes(matrix):
    import ossl
    plan, res = matrix
    lk, w, signers = K.wallet("t1n3s3")
    assert {K.ROWS[r][1] for r in plan if r is not None} == {91, 201, 202, 301, 401, 402, 531, 541, 542, 601}
    for k, (row, out) in enumerate(zip(plan, res)):
        if row is None:
            assert out["status"] == [0] * len(signers), (k, out["status"])
            r, s, _ = out["sig"][0]
            assert ossl.ecdsa_verify(lk["arrays"]["y"][0], F.words([out["msg"]], 8), F.words([r], 8), F.words([s], 8)).all()
            continue
        name, code, rnd, _ = K.ROWS[row]
        assert code in out["status"], (name, out["status"])
        # the first failure of the session is the row's: nobody failed in an earlier phase (the hundreds name the phase)
        assert all(st == 0 or st // 100 >= code // 100 for st in out["status"]), (name, out["status"])
        assert all((sg is None) == (st != 0) for sg, st in zip(out["sig"], out["status"])), name


def test_402_and_the_panics_are_codes():
    """a neutral R is status 402 where the reference's unwrap() panics; phase3_reconstruct_delta's expect is 301"""
    with pytest.raises(P18.Gg18Error) as e:
        P18.LocalSignature.phase5_local_sig(1, 2, None, 3, R.G, 4, 5)
    assert P18.STATUS[e.value.what] == 402
    with pytest.raises(P18.Gg18Error) as e:
        P18.SignKeys.phase3_reconstruct_delta([5, R.Q - 5])
    assert P18.STATUS[e.value.what] == 301


def test_verify_has_no_low_s_rule():
    """party_i.rs:714-737 accepts the high-s twin of a signature (party_one::verify, Lindell's, refuses it)"""
    x, k, m = 0x1234, 0x5678, 0x9abc
    y, Rp = R.ec_mul(x, R.G), R.ec_mul(pow(k, -1, R.Q), R.G)
    r = Rp[0] % R.Q
    s = k * (m + r * x) % R.Q
    assert P18.verify((r, s), y, m) and P18.verify((r, R.Q - s), y, m)
    assert not P18.verify((r, (s + 1) % R.Q), y, m) and not P18.verify((r, 0), y, m)


def test_header_declares_and_library_exports_the_gg18_calls():
    hdr = open(os.path.join(ROOT, "include", "mpecdsa_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mpe_gg18_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(GG18_CALLS)
    path = os.path.join(ROOT, "multi_party_ecdsa_amd", "libmpecdsa_hip.so")
    if not os.path.exists(path):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(path)
    for name in GG18_CALLS:
        assert hasattr(lib, name), name
    # bad arguments are refused before any HIP call
    lib.mpe_gg18_phase2.restype = ctypes.c_int
    assert lib.mpe_gg18_phase2(*([None] * 21)) == -1
    assert lib.mpe_gg18_message_b(*([None] * 15)) == -1


def test_packing_round_trips():
    res = K.reference(K.jobs_for("t1n3", 1))
    flat = K.flat_session(res[0]["msgs"])
    assert K.flat_session(K.unflat_session(flat)) == flat
    packed = K.pack_msgs(res)
    assert packed["mb_c"].shape == (2, 1, 2, 1, 128) and packed["V"].shape == (2, 1, 16)
    assert F.ints(packed["delta"][:, 0]) == res[0]["msgs"]["delta"]
    assert np.any(packed["heg_T"]) and np.any(packed["dlog_z"])
