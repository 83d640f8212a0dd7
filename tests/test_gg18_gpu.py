"""GPU tests of GG18 signing (mpe_gg18.h, engine.gg18_sign) against the Python restatement tests/pyref_gg18.py: every new call alone on
the restatement's values, byte for byte, under two encoding profiles at 67 items (one full 64-lane workgroup and a ragged second);
the chain with given draws at the reference's shapes, every message of every round; the tamper / hostile matrix; seed to signature;
workspace hygiene.  The restatement's sessions come from gg18_cases.reference (computed once, shared)."""
import numpy as np
import pytest
import torch

import enc_profiles as EP
import fixtures as F
import gg18_cases as K
import pyref as R

pytestmark = pytest.mark.gpu
B67 = 67


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _np(t):
    return t.cpu().numpy().view(np.uint32)


def _ctx_for(gpu_ctx, profile):
    from multi_party_ecdsa_amd import engine as E
    return gpu_ctx if profile == "default" else E.Context(0, encoding=EP.PROFILES[profile].as_dict())


def _wallet(ctx, shape, own=None):
    from multi_party_ecdsa_amd import engine as E
    lk, w, signers = K.wallet(shape)
    return E.Gg18Wallet(ctx, lk["t"], lk["n"], lk["arrays"], own=own), lk, w, signers


def _case(shape, B, profile="default"):
    res = K.reference(K.jobs_for(shape, B, EP.PROFILES[profile]))
    assert all(r["status"] == [0] * len(r["status"]) for r in res)
    return res


def _msgs_equal(got, want, rows=None):
    for f in K.MSG_FIELDS:
        g, w = _np(got[f]), want[f]
        if rows is not None:
            g, w = g[rows], w[rows]
        assert np.array_equal(g, w), f


# ---- 1. every new call alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["default", "all-alt"])
def test_phase_by_phase(gpu_ctx, profile):
    from multi_party_ecdsa_amd import engine as E
    ctx = _ctx_for(gpu_ctx, profile)
    res = _case("t1n3", B67, profile)
    wal, lk, w, sg = _wallet(ctx, "t1n3")
    S, B, loc = 2, B67, [0, 1]
    m, z = K.pack_msgs(res), {f: _dev(ctx, v) for f, v in K.pack_draws(res).items()}
    d = {f: _dev(ctx, v) for f, v in m.items()}
    st = lambda f, w_, kind="int": K.pack_list([[r["state"][f][i] for r in res] for i in range(S)], w_, kind)
    zero = lambda: torch.zeros((S, B), dtype=torch.int32, device=ctx.device)
    # SignKeys::create
    x_i = _dev(ctx, np.repeat(lk["arrays"]["x"][sg][:, None, :], B, axis=1))
    pk_vec = _dev(ctx, np.repeat(lk["arrays"]["X"][None], B, axis=0))
    o = E.gg18_sign_keys(ctx, lk["t"], lk["n"], sg, loc, x_i, pk_vec, z["k"], z["gamma"])
    assert np.array_equal(_np(o["w_i"]), st("w", 8)) and np.array_equal(_np(o["g_w_i"]), st("g_w_i", 16, "pt"))
    assert np.array_equal(_np(o["g_gamma_i"]), m["g_gamma"]) and np.array_equal(_np(o["g_w"]), st("g_w", 16, "pt"))
    assert not _np(o["status"].to(torch.int32)).any()
    bad_k = z["k"].clone()
    bad_k[1, 5] = 0                                                            # zero, and q itself: neither is a Scalar::random()
    bad_k[0, 66] = _dev(ctx, F.words([R.Q], 8))[0]
    o2 = E.gg18_sign_keys(ctx, lk["t"], lk["n"], sg, loc, x_i, pk_vec, bad_k, z["gamma"])
    st2 = o2["status"].cpu().numpy()
    assert st2[1, 5] == 91 and st2[0, 66] == 91 and (st2 != 0).sum() == 2 and not _np(o2["g_gamma_i"])[1, 5].any()
    # MessageB::b(.., &[]): items [2, L, S-1, B]
    n_mb = 2 * S * B
    b_sel = torch.stack([z["gamma"], o["w_i"]]).reshape(2, S, 1, B, 8)
    ca = torch.stack([d["c_a"][1], d["c_a"][0]]).reshape(1, S, 1, B, 128).expand(2, S, 1, B, 128).contiguous()
    key = torch.tensor([sg[1], sg[0]], dtype=torch.int32, device=ctx.device).reshape(1, S, 1, 1).expand(2, S, 1, B).contiguous()
    mb = E.gg18_message_b(ctx, wal.pk, b_sel.reshape(n_mb, 8).contiguous(), ca.reshape(n_mb, 128), z["mb_r"].reshape(n_mb, 64), z["mb_beta_tag"].reshape(n_mb, 64),
                          z["mb_nonce_b"].reshape(n_mb, 8), z["mb_nonce_bt"].reshape(n_mb, 8), key.reshape(-1))
    sent = lambda t: _np(t).reshape(2, S, 1, B, -1).transpose(1, 2, 0, 3, 4)
    for f, t in (("mb_c", mb["c"]), ("mb_b_pk", mb["b_proof"]["pk"]), ("mb_b_R", mb["b_proof"]["R"]), ("mb_b_z", mb["b_proof"]["z"]),
                 ("mb_bt_pk", mb["beta_tag_proof"]["pk"]), ("mb_bt_R", mb["beta_tag_proof"]["R"]), ("mb_bt_z", mb["beta_tag_proof"]["z"])):
        assert np.array_equal(sent(t), m[f]), f
    beta = K.pack_list([[r["state"]["beta"][i][0][v] for r in res] for v in range(2) for i in range(S)], 8).reshape(2, S, 1, B, 8)
    assert np.array_equal(_np(mb["beta"]).reshape(2, S, 1, B, 8), beta)
    # phase2_delta_i / phase2_sigma_i with the verdicts of the alphas
    alpha = K.pack_list([[r["state"]["alpha"][i][0] for r in res] for i in range(S)], 8).reshape(S, 1, B, 8)
    miu = K.pack_list([[r["state"]["miu"][i][0] for r in res] for i in range(S)], 8).reshape(S, 1, B, 8)
    ones = torch.ones((S, 1, B), dtype=torch.uint8, device=ctx.device)
    w_pk = _dev(ctx, np.stack([m["mb_b_pk"][1, 0, 1], m["mb_b_pk"][0, 0, 1]]).reshape(S, 1, B, 16))
    status = zero()
    delta_i, sigma_i = E.gg18_phase2(ctx, sg, loc, z["k"], z["gamma"], o["w_i"], _dev(ctx, alpha), _dev(ctx, beta[0]), _dev(ctx, miu), _dev(ctx, beta[1]),
                                     ones, ones, w_pk, o["g_w"], status)
    assert np.array_equal(_np(delta_i), m["delta"]) and np.array_equal(_np(sigma_i), st("sigma", 8)) and not status.cpu().numpy().any()
    status2, ok_bad, pk_bad = zero(), ones.clone(), w_pk.clone()
    ok_bad[0, 0, 3] = 0
    pk_bad[1, 0, 64] = w_pk[0, 0, 64]                                          # the receiver's OWN g_w_i, what test.rs:278 compares with
    dl2, _ = E.gg18_phase2(ctx, sg, loc, z["k"], z["gamma"], o["w_i"], _dev(ctx, alpha), _dev(ctx, beta[0]), _dev(ctx, miu), _dev(ctx, beta[1]), ones, ok_bad,
                           pk_bad, o["g_w"], status2)
    s2 = status2.cpu().numpy()
    assert s2[0, 3] == 201 and s2[1, 64] == 202 and (s2 != 0).sum() == 2 and not _np(dl2)[0, 3].any() and np.array_equal(_np(dl2)[1, 63], m["delta"][1, 63])
    # phase3_reconstruct_delta / phase4
    b_pk = _dev(ctx, np.stack([m["mb_b_pk"][1, 0, 0], m["mb_b_pk"][0, 0, 0]]).reshape(S, 1, B, 16))
    Rw = K.pack_list([[r["R"][i] for r in res] for i in range(S)], 16, "pt")
    status = zero()
    Rd = E.gg18_phase4(ctx, sg, loc, d["delta"], b_pk, d["g_gamma"], d["blind"], d["com"], status)
    assert np.array_equal(_np(Rd), Rw) and not status.cpu().numpy().any()
    # phase5_local_sig / phase5a_broadcast_5b_zkproof
    msg = _dev(ctx, F.words([r["msg"] for r in res], 8))
    a5 = E.gg18_phase5a(ctx, sg, loc, z["k"], sigma_i, msg, Rd, z["l"], z["rho"], z["blind5a"], z["heg_s1"], z["heg_s2"], z["dlog_nonce"], status)
    assert np.array_equal(_np(a5["s_i"]), m["s_i"])
    for f, t in (("V", a5["V"]), ("A", a5["A"]), ("B", a5["B"]), ("com5a", a5["com"]), ("heg_T", a5["heg"]["T"]), ("heg_A3", a5["heg"]["A3"]),
                 ("heg_z1", a5["heg"]["z1"]), ("heg_z2", a5["heg"]["z2"]), ("dlog_pk", a5["dlog"]["pk"]), ("dlog_R", a5["dlog"]["R"]), ("dlog_z", a5["dlog"]["z"])):
        assert np.array_equal(_np(t), m[f]), f
    # phase5c
    y = wal.y.expand(B, 16).contiguous()
    bc = dict(V=d["V"], A=d["A"], B=d["B"], blind=d["blind5a"], com=d["com5a"], T=d["heg_T"], A3=d["heg_A3"], z1=d["heg_z1"], z2=d["heg_z2"],
              dlog_pk=d["dlog_pk"], dlog_R=d["dlog_R"], dlog_z=d["dlog_z"])
    u, t_, com5c = E.gg18_phase5c(ctx, sg, loc, msg, y, Rd, z["l"], z["rho"], z["blind5c"], bc, status)
    assert np.array_equal(_np(u), m["u"]) and np.array_equal(_np(t_), m["t"]) and np.array_equal(_np(com5c), m["com5c"]) and not status.cpu().numpy().any()
    # phase5d, clean and with one commitment that does not open
    E.gg18_phase5d(ctx, sg, loc, d["u"], d["t"], d["blind5c"], d["com5c"], d["B"], status)
    assert not status.cpu().numpy().any()
    com_bad, status3 = d["com5c"].clone(), zero()
    com_bad[1, 65, 0] ^= 1
    E.gg18_phase5d(ctx, sg, loc, d["u"], d["t"], d["blind5c"], com_bad, d["B"], status3)
    s3 = status3.cpu().numpy()
    assert (s3[:, 65] == 541).all() and (s3 != 0).sum() == S
    # output_signature
    r_, s_, recid = E.gg18_output_signature(ctx, sg, loc, a5["s_i"], d["s_i"], Rd, msg, y, status)
    ctx.sync()
    for i in range(S):
        wr, ws, wrec = K.pack_sigs(res, i)
        assert np.array_equal(_np(r_)[i], wr) and np.array_equal(_np(s_)[i], ws) and np.array_equal(recid.cpu().numpy()[i], wrec)
    assert not status.cpu().numpy().any()
    wal.close()


# ---- 2. the chain with given draws ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", [("t1n3", B67), ("t2n5", 5), ("t4n8", 2)])
def test_chain_matches_the_restatement(gpu_ctx, shape, B):
    from multi_party_ecdsa_amd import engine as E
    import ossl
    res = _case(shape, B)
    wal, lk, w, sg = _wallet(gpu_ctx, shape)
    msg = F.words([r["msg"] for r in res], 8)
    out = E.gg18_sign(gpu_ctx, wal, sg, _dev(gpu_ctx, msg), B, draws=K.pack_draws(res))
    assert not out["status"].cpu().numpy().any() and out["failures"] == 0
    _msgs_equal(out["msgs"], K.pack_msgs(res))
    for i in range(len(sg)):
        wr, ws, wrec = K.pack_sigs(res, i)
        assert np.array_equal(_np(out["r_all"])[i], wr) and np.array_equal(_np(out["s_all"])[i], ws) and np.array_equal(out["recid_all"].cpu().numpy()[i], wrec)
    assert np.array_equal(_np(out["R"]), K.pack_list([[r["R"][i] for r in res] for i in range(len(sg))], 16, "pt"))
    assert ossl.ecdsa_verify(lk["arrays"]["y"][0], msg, _np(out["r"]), _np(out["s"])).all()
    wal.close()


def test_one_local_signer_among_restated_peers(gpu_ctx):
    """the per-party view: signer ordinal 2 of (2, 5, [0, 2, 3, 4]) here, holding only its own secrets; the peers' messages of
    every round come from the restatement"""
    from multi_party_ecdsa_amd import engine as E
    B, me = 5, 2
    res = _case("t2n5", B)
    lk, w, sg = K.wallet("t2n5")
    wal = E.Gg18Wallet(gpu_ctx, lk["t"], lk["n"], lk["arrays"], own=[sg[me]])
    want = K.pack_msgs(res)
    peers = [j for j in range(len(sg)) if j != me]

    def relay(rnd, msgs):
        for f, (r_, _, _) in K.MSG_FIELDS.items():
            if r_ == rnd:
                msgs[f][peers] = _dev(gpu_ctx, want[f][peers])
    msg = F.words([r["msg"] for r in res], 8)
    out = E.gg18_sign(gpu_ctx, wal, sg, _dev(gpu_ctx, msg), B, draws=K.pack_draws(res, local=[me]), local=[me], _fault=relay)
    assert not out["status"].cpu().numpy().any()
    _msgs_equal(out["msgs"], want, rows=[me])
    wr, ws, wrec = K.pack_sigs(res, me)
    assert np.array_equal(_np(out["r"]), wr) and np.array_equal(_np(out["s"]), ws) and np.array_equal(out["recid"].cpu().numpy(), wrec)
    wal.close()


# ---- 3. the tamper and hostile matrix: session k carries row k --------------------------------------------------------------------
def test_tamper_and_hostile_matrix(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    import ossl
    plan, res = K.matrix_plan(), K.reference(K.matrix_jobs())
    wal, lk, w, sg = _wallet(gpu_ctx, "t1n3s3")
    B = len(plan)
    msg = F.words([r["msg"] for r in res], 8)
    out = E.gg18_sign(gpu_ctx, wal, sg, _dev(gpu_ctx, msg), B, draws=K.pack_draws(res), _fault=K.device_hook(plan, dict(w=w, signers=sg)))
    gpu_ctx.sync()                                                             # the run completes without a HIP error
    status = out["status"].cpu().numpy()
    assert status.tolist() == [r["status"] for r in res]
    _msgs_equal(out["msgs"], K.pack_msgs(res))
    clean = [k for k, row in enumerate(plan) if row is None]
    assert len(clean) >= 5 and not status[clean].any()
    assert ossl.ecdsa_verify(lk["arrays"]["y"][0], msg[clean], _np(out["r"])[clean], _np(out["s"])[clean]).all()
    for i in range(len(sg)):
        wr, ws, wrec = K.pack_sigs(res, i)
        assert np.array_equal(_np(out["r_all"])[i], wr) and np.array_equal(_np(out["s_all"])[i], ws)
    assert not _np(out["r_all"])[status.T != 0].any() and not _np(out["s_all"])[status.T != 0].any()
    wal.close()


# ---- 4. seed to signature ---------------------------------------------------------------------------------------------------------
def test_seed_to_signature(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    import ossl
    import pyref_gg18 as P18
    B = 128
    wal, lk, w, sg = _wallet(gpu_ctx, "t1n3")
    seed = b"gg18 seed to signature".ljust(32, b".")
    msgs = [K.session_msg("seeded-%d" % b) for b in range(B)]
    msg = F.words(msgs, 8)
    a = E.gg18_sign(gpu_ctx, wal, sg, _dev(gpu_ctx, msg), B, seed=seed, counter=3)
    assert not a["status"].cpu().numpy().any() and a["failures"] == 0
    assert ossl.ecdsa_verify(lk["arrays"]["y"][0], msg, _np(a["r"]), _np(a["s"])).all()
    b = E.gg18_sign(gpu_ctx, wal, sg, _dev(gpu_ctx, msg), B, seed=seed, counter=3)
    assert np.array_equal(_np(a["r"]), _np(b["r"])) and np.array_equal(_np(a["s"]), _np(b["s"])) and torch.equal(a["recid"], b["recid"])
    for f in K.MSG_FIELDS:
        assert torch.equal(a["msgs"][f], b["msgs"][f]), f
    c = E.gg18_sign(gpu_ctx, wal, sg, _dev(gpu_ctx, msg), B, seed=seed, counter=4)
    assert not c["status"].cpu().numpy().any() and not (_np(a["r"]) == _np(c["r"])).all(axis=1).any()
    # the draws are what the sampler's rules give: scalars in [1, q), values below the right modulus
    dr = {f: _np(v) for f, v in a["draws"].items()}
    assert all(0 < x < R.Q for x in F.ints(dr["k"].reshape(-1, 8))) and all(x < w["N"][sg[0]] for x in F.ints(dr["r_a"][0]))
    assert all(x < w["N"][sg[1]] for x in F.ints(dr["mb_beta_tag"][0, 0, 0])) and all(x < w["N"][sg[0]] for x in F.ints(dr["mb_r"][1, 1, 0]))
    # the first 8 sessions again through the restatement, from the draws the device returned
    for k in range(8):
        d = {f: [F.ints(dr[f][i, k:k + 1])[0] for i in range(2)] for f in K.DRAW_WORDS if not f.startswith("mb_")}
        for f in ("mb_beta_tag", "mb_r", "mb_nonce_b", "mb_nonce_bt"):
            d[f] = [[[F.ints(dr[f][v, i, 0, k:k + 1])[0] for v in range(2)]] for i in range(2)]
        ref = P18.sign_session(w, sg, msgs[k], d)
        assert ref["status"] == [0, 0]
        assert ref["sig"][0] == (F.ints(_np(a["r"])[k:k + 1])[0], F.ints(_np(a["s"])[k:k + 1])[0], int(a["recid"][k]))
    wal.close()


# ---- 5. hygiene ---------------------------------------------------------------------------------------------------------------------
def test_workspace_hygiene(gpu_ctx):
    """the intermediates of the new calls (beta_tag mod q, the ladders' tables, the plaintexts of the decryptions) live in the context's
    scratch: the audit sees them, the wipe clears them"""
    from multi_party_ecdsa_amd import engine as E
    wal, lk, w, sg = _wallet(gpu_ctx, "t1n3")
    msg = F.words([K.session_msg("hygiene-%d" % b) for b in range(4)], 8)
    out = E.gg18_sign(gpu_ctx, wal, sg, _dev(gpu_ctx, msg), 4, seed=b"gg18 hygiene".ljust(32, b"."), counter=1)
    assert not out["status"].cpu().numpy().any()
    assert gpu_ctx.scratch_audit()[0] > 0
    gpu_ctx.wipe()
    assert gpu_ctx.scratch_audit()[0] == 0
    wal.close()
