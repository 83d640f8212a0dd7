"""GPU: GG20 sessions that sign for BIP32 child keys (`mpe_gg20_session_create_tweaks`, `_rearm_tweaks`, `mpe_gg20_sign_tweaks`,
`mpe_gg20_session_child_keys`).  B = 8 sessions of the (1, 3) wallet, signer sets mixed over its three quorums, tweaks
[0, 1, q - 1] and five from mpe_bip32_derive.  The comparator is the CPU oracle run on CHILD WALLETS built in Python
(tests/pyref_bip32.py: x_i + t, X_i + t G, y + t G, Paillier keys and statements shared), one per session, through its multi-wallet
path (`keyset=` of G.oracle_sign_ex) — sampler bounds and nonces are the same on both sides.
 a. lock-step: status, r, s, recid equal the oracle's; OpenSSL accepts every signature under the child key and, for t != 0, refuses it
    under the parent's
 b. one party per object, by party index: every round's slab is byte-identical to the oracle's
 c. t = 0 rows are the untweaked entry point's, byte for byte; no tweaks through `_tweaks` is `_sets`
 d. t = q and the all-ones tweak: status 93 at round 0, zero records, no signature; the other six sign
 e. re-arming with new tweaks equals a fresh session
 f. round 2's check of b_proof.pk against g_w is live: records made for the parent key are refused (202) where t != 0
 g. what is refused: depositing into a presignature pool, the blame openings, re-arming an untweaked session with tweaks"""
import ctypes as C

import numpy as np
import pytest
import torch

import fixtures as F
import gg20_fixture as G
import ossl
import pyref
import pyref_bip32 as PB
import sigset_cases as SC

pytestmark = pytest.mark.gpu

Q = pyref.Q
B, T, N_PARTIES, S = 8, 1, 3, 2
SIGSET = [0, 1, 2, 2, 0, 1, 1, 0]
CHAIN_CODE = bytes(range(100, 132))
PATHS = [[0, 0, 0], [(1 << 31) - 1, 3, 0], [11, 12, 13], [7, 0, 0], [65536, (1 << 31) - 2, 0]]
DEPTHS = [1, 2, 3, 1, 2]


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _i32(ctx, vals):
    return torch.tensor([int(v) for v in vals], dtype=torch.int32, device=ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _tw(ctx, tweaks):
    return _dev(ctx, F.words(tweaks, 8))


def _rounds(ctx, sess, msg, upto=8, start=0, prev=None):
    """rounds start..upto of a session object with every signer local: ({round: [L, B, W] numpy}, the last outgoing device tensor)"""
    slabs = {}
    for rnd in range(start, upto + 1):
        out = sess.round(rnd, d_in=prev, msg=msg if rnd == 7 else None)
        if rnd in G.ROUNDS:
            slabs[rnd] = _u32(out)
            prev = out
    return slabs, prev


def _result(ctx, sess, signature=True):
    res = sess.result(signature=signature)
    ctx.sync()
    return {f: (_u32(v) if f in ("r", "s", "R", "bad_actors") else v.cpu().numpy()) for f, v in res.items()}


def oracle_children(children, nonces, sigset):
    """The oracle on one child wallet per session: the sessions of one signer set run as ONE multi-wallet call (key set k = the k-th of
    them, `keyset=`), their rows scattered back.  Returns what G.oracle_sign_ex returns, over the whole batch."""
    nb = len(sigset)
    out = None
    for k in sorted(set(sigset)):
        sessions = [b for b in range(nb) if sigset[b] == k]
        arrays = {f: np.concatenate([children[b]["arrays"][f] for b in sessions]) for f in SC.KEY_FIELDS}
        arrays["signers"] = children[sessions[0]]["arrays"]["signers"]
        lk = dict(children[sessions[0]], arrays=arrays, nkeysets=len(sessions))
        got = G.oracle_sign_ex(lk, SC.session_rows(nonces, nb, sessions), len(sessions), keyset=np.arange(len(sessions), dtype=np.int32))
        if out is None:
            out = dict(slabs={rnd: np.zeros((S, nb, v.shape[2]), dtype=np.uint32) for rnd, v in got["slabs"].items()},
                       r=np.zeros((nb, 8), dtype=np.uint32), s=np.zeros((nb, 8), dtype=np.uint32), recid=np.zeros(nb, dtype=np.int32),
                       R=np.zeros((nb, 16), dtype=np.uint32), status=np.full(nb, -1, dtype=np.int32))
        for rnd, v in got["slabs"].items():
            out["slabs"][rnd][:, sessions] = v
        for f in ("r", "s", "recid", "R", "status"):
            out[f][sessions] = got[f]
    return out


class Case:
    def __init__(self, ctx, keys):
        from multi_party_ecdsa_amd import engine as E
        self.sets = SC.all_sets(N_PARTIES, S)
        self.lks, per_wallet = SC.wallet(keys, T, N_PARTIES, self.sets)
        self.parent = self.lks[0]["y"]
        self.nonces = SC.mixed_nonces(per_wallet, SIGSET, seed="gg20-tweaks")
        tw, child, _, st = E.bip32_derive(ctx, _dev(ctx, F.point_words([self.parent])), CHAIN_CODE, PATHS, depth=DEPTHS)
        ctx.sync()
        derived, kids = F.ints(_u32(tw)), F.points(_u32(child))
        for row, (path, depth) in enumerate(zip(PATHS, DEPTHS)):
            assert (int(st[row]), derived[row], kids[row]) == PB.derive([(self.parent, CHAIN_CODE)], 0, path, depth, 3)[:3]
        self.tweaks = [0, 1, Q - 1] + derived
        self.children = [PB.child_wallet(self.lks[SIGSET[b]], self.tweaks[b]) for b in range(B)]
        assert [c["y"] for c in self.children[3:]] == kids and self.children[0]["y"] == self.parent
        self.child_pub = F.point_words([c["y"] for c in self.children])
        self.want = oracle_children(self.children, self.nonces, SIGSET)
        assert not self.want["status"].any()
        self.gk = E.Gg20Keys(ctx, T, N_PARTIES, None, self.lks[0]["arrays"], signer_sets=self.sets)
        self.dn = {f: _dev(ctx, v) for f, v in self.nonces.items()}
        self.ds, self.dt = _i32(ctx, SIGSET), _tw(ctx, self.tweaks)


@pytest.fixture(scope="module")
def case(gpu_ctx, keys):
    c = Case(gpu_ctx, keys)
    yield c
    c.gk.close()


def _same_signatures(r, s, recid, want, rows=None):
    rows = list(range(B)) if rows is None else rows
    assert np.array_equal(r[rows], want["r"][rows]) and np.array_equal(s[rows], want["s"][rows]) and list(recid[rows]) == list(want["recid"][rows])


# ---- a ---------------------------------------------------------------------------------------------------------------------------
def test_a_lockstep_signs_for_the_child_keys(gpu_ctx, case):
    from multi_party_ecdsa_amd import engine as E
    c, ctx = case, gpu_ctx
    r, s, recid, status, R = [o.cpu().numpy() for o in E.gg20_sign(ctx, c.gk, c.dn, B, want_R=True, sigset=c.ds, tweaks=c.dt)]
    assert not status.any()
    _same_signatures(r.view(np.uint32), s.view(np.uint32), recid, c.want)
    assert np.array_equal(R.view(np.uint32), c.want["R"])
    msg = c.nonces["msg"]
    assert ossl.ecdsa_verify(c.child_pub, msg, r.view(np.uint32), s.view(np.uint32)).all(), "OpenSSL refuses a signature under its child key"
    under_parent = ossl.ecdsa_verify(F.point_words([c.parent])[0], msg, r.view(np.uint32), s.view(np.uint32))
    assert list(under_parent) == [t == 0 for t in c.tweaks], "a signature for a child key verifies under the parent's"
    r2, s2, recid2, status2 = [o.cpu().numpy() for o in E.gg20_sign(ctx, c.gk, c.dn, B, dedup_verify=True, chunk=3, sigset=c.ds, tweaks=c.dt)]
    assert not status2.any()
    _same_signatures(r2.view(np.uint32), s2.view(np.uint32), recid2, c.want)


# ---- b ---------------------------------------------------------------------------------------------------------------------------
def test_b_one_party_per_object_every_slab_equals_the_oracles(gpu_ctx, case):
    """Three objects, one per party, each holding only its own secrets and the sessions whose set contains it; the test is the relay."""
    from multi_party_ecdsa_amd import engine as E
    c, ctx = case, gpu_ctx
    parties = []
    for p in range(N_PARTIES):
        mine = [g for g in range(B) if p in c.sets[SIGSET[g]]]
        ordinal = [SC.words.rank_in_set(c.sets[SIGSET[g]], p) for g in mine]
        parts = [G.party_nonces(SC.session_rows(c.nonces, B, [g]), c.lks[SIGSET[g]], i) for g, i in zip(mine, ordinal)]
        zp = {f: np.ascontiguousarray(np.concatenate([q[f] for q in parts])) for f in parts[0]}
        gk = E.Gg20Keys(ctx, T, N_PARTIES, None, c.lks[0]["arrays"], own=[p], signer_sets=c.sets)
        dn = {f: _dev(ctx, v) for f, v in zp.items()}
        sess = E.Gg20Session(ctx, gk, len(mine), None, dn, sigset=_i32(ctx, [SIGSET[g] for g in mine]), local_party=p,
                             tweaks=_tw(ctx, [c.tweaks[g] for g in mine]))
        assert np.array_equal(_u32(sess.child_keys()), c.child_pub[mine])
        parties.append(dict(mine=mine, ordinal=ordinal, gk=gk, dn=dn, sess=sess))
    prev = None
    for rnd in range(9):
        W = G.msg_words(S, N_PARTIES, rnd) if rnd in G.ROUNDS else 0
        slab = np.zeros((S, B, W), dtype=np.uint32)
        for q in parties:
            d_in = None if prev is None or rnd == 7 else _dev(ctx, prev[:, q["mine"]])
            out = q["sess"].round(rnd, d_in=d_in, msg=q["dn"]["msg"] if rnd == 7 else None)
            if W:
                o = _u32(out)
                for row, (g, i) in enumerate(zip(q["mine"], q["ordinal"])):
                    slab[i, g] = o[0, row]
        if W:
            assert np.array_equal(slab, c.want["slabs"][rnd]), f"round {rnd}"
            prev = slab
    for q in parties:
        res = _result(ctx, q["sess"])
        assert not res["status"].any()
        _same_signatures(res["r"][0], res["s"][0], res["recid"][0], {f: c.want[f][q["mine"]] for f in ("r", "s", "recid")}, rows=list(range(len(q["mine"]))))
        q["sess"].close()
        q["gk"].close()


# ---- c ---------------------------------------------------------------------------------------------------------------------------
def test_c_tweak_zero_and_no_tweaks_are_the_untweaked_entry_points(gpu_ctx, case):
    from multi_party_ecdsa_amd import engine as E, _native as N
    c, ctx = case, gpu_ctx
    got = {}
    for name, kw in (("tweaked", dict(tweaks=c.dt)), ("plain", dict())):
        sess = E.Gg20Session(ctx, c.gk, B, list(range(S)), c.dn, sigset=c.ds, **kw)
        got[name] = (_rounds(ctx, sess, c.dn["msg"])[0], _result(ctx, sess), _u32(sess.child_keys()))
        sess.close()
    slabs_t, res_t, keys_t = got["tweaked"]
    slabs_p, res_p, keys_p = got["plain"]
    zero = [b for b in range(B) if c.tweaks[b] == 0]
    assert zero == [0] and not res_p["status"].any() and not res_t["status"].any()
    for rnd in G.ROUNDS:
        assert np.array_equal(slabs_t[rnd], c.want["slabs"][rnd]), f"round {rnd}: the ordinals form against the oracle"
        assert np.array_equal(slabs_t[rnd][:, zero], slabs_p[rnd][:, zero]), f"round {rnd}: t = 0 against the untweaked session"
    for f in ("r", "s", "recid", "R"):
        assert np.array_equal(res_t[f][:, zero], res_p[f][:, zero]), f
    assert np.array_equal(keys_t, c.child_pub) and np.array_equal(keys_p, np.repeat(F.point_words([c.parent]), B, axis=0))
    # no tweaks through mpe_gg20_sign_tweaks is mpe_gg20_sign_sets, for the whole batch
    plain = [o.cpu().numpy() for o in E.gg20_sign(ctx, c.gk, c.dn, B, want_R=True, sigset=c.ds)]
    r, s, R = (torch.zeros((B, w), dtype=torch.int32, device=ctx.device) for w in (8, 8, 16))
    recid, status = (torch.full((B,), -1, dtype=torch.int32, device=ctx.device) for _ in range(2))
    nn = E._struct(N.Gg20Nonces, c.dn)
    N.check(N.lib.mpe_gg20_sign_tweaks(ctx.h, c.gk.h, B, None, E._ptr(c.ds), None, C.byref(nn), E._ptr(r), E._ptr(s), E._ptr(recid), E._ptr(R),
                                       E._ptr(status), 0, 0, ctx.stream()), "mpe_gg20_sign_tweaks")
    ctx.sync()
    for a, b in zip(plain, (r, s, recid, status, R)):
        assert np.array_equal(a, b.cpu().numpy())
    assert not plain[3].any()


# ---- d ---------------------------------------------------------------------------------------------------------------------------
def test_d_a_bad_tweak_stops_its_session_alone(gpu_ctx, case):
    from multi_party_ecdsa_amd import engine as E
    c, ctx = case, gpu_ctx
    tweaks = list(c.tweaks)
    tweaks[2], tweaks[5] = Q, PB.ALL_ONES
    bad, good = [2, 5], [0, 1, 3, 4, 6, 7]
    dt = _tw(ctx, tweaks)
    sess = E.Gg20Session(ctx, c.gk, B, list(range(S)), c.dn, sigset=c.ds, tweaks=dt)
    out0 = _u32(sess.round(0))
    st0 = _result(ctx, sess, signature=False)["status"]
    assert (st0[:, bad] == PB.BAD_TWEAK).all() and not st0[:, good].any() and not out0[:, bad].any(), "round 0"
    slabs, _ = _rounds(ctx, sess, c.dn["msg"], start=1, prev=_dev(ctx, out0))
    slabs[0] = out0
    res = _result(ctx, sess)
    keys_ = _u32(sess.child_keys())
    sess.close()
    for rnd in G.ROUNDS:
        assert not slabs[rnd][:, bad].any(), f"round {rnd}: a refused session emitted a record"
        assert np.array_equal(slabs[rnd][:, good], c.want["slabs"][rnd][:, good]), f"round {rnd}: the neighbours"
    assert (res["status"][:, bad] == PB.BAD_TWEAK).all() and not res["status"][:, good].any()
    assert not res["r"][:, bad].any() and not res["s"][:, bad].any() and not res["recid"][:, bad].any()
    assert not keys_[bad].any() and np.array_equal(keys_[good], c.child_pub[good])
    for i in range(S):
        _same_signatures(res["r"][i], res["s"][i], res["recid"][i], c.want, rows=good)
    r, s, recid, status = [o.cpu().numpy() for o in E.gg20_sign(ctx, c.gk, c.dn, B, sigset=c.ds, tweaks=dt)]
    assert list(status[bad]) == [PB.BAD_TWEAK] * 2 and not status[good].any()
    assert not r[bad].any() and not s[bad].any() and not recid[bad].any()
    _same_signatures(r.view(np.uint32), s.view(np.uint32), recid, c.want, rows=good)


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def test_e_rearm_with_new_tweaks_equals_a_fresh_session(gpu_ctx, case):
    from multi_party_ecdsa_amd import engine as E
    c, ctx = case, gpu_ctx
    sess = E.Gg20Session(ctx, c.gk, B, list(range(S)), c.dn, sigset=c.ds, tweaks=_tw(ctx, [5] * B))
    first = _u32(sess.round(0))
    assert np.array_equal(_u32(sess.child_keys()), F.point_words([pyref.ec_add(c.parent, pyref.ec_mul(5, pyref.G))] * B))
    sess.abort()
    sess.rearm(c.dn, sigset=c.ds, tweaks=c.dt)
    slabs, _ = _rounds(ctx, sess, c.dn["msg"])
    res = _result(ctx, sess)
    assert np.array_equal(_u32(sess.child_keys()), c.child_pub)
    for rnd in G.ROUNDS:
        assert np.array_equal(slabs[rnd], c.want["slabs"][rnd]), f"round {rnd}"
    assert np.array_equal(first, c.want["slabs"][0]), "round 0 does not depend on the key share"
    assert not res["status"].any()
    _same_signatures(res["r"][0], res["s"][0], res["recid"][0], c.want)
    # ... and without tweaks the same object is an untweaked session again
    sess.rearm(c.dn, sigset=c.ds)
    assert np.array_equal(_u32(sess.child_keys()), np.repeat(F.point_words([c.parent]), B, axis=0))
    sess.close()


# ---- f ---------------------------------------------------------------------------------------------------------------------------
def test_f_records_made_for_the_parent_key_are_refused_in_round_2(gpu_ctx, case):
    """A sender that runs UNTWEAKED proves knowledge of w_i for the parent key in its round-1 MessageB; a tweaked receiver compares
    b_proof.pk with ITS g_w table (rounds.rs:281) and answers 202 — in exactly the sessions with t != 0."""
    from multi_party_ecdsa_amd import engine as E
    c, ctx = case, gpu_ctx
    recv = E.Gg20Session(ctx, c.gk, B, list(range(S)), c.dn, sigset=c.ds, tweaks=c.dt)
    send = E.Gg20Session(ctx, c.gk, B, list(range(S)), c.dn, sigset=c.ds)
    r0, s0 = recv.round(0), send.round(0)
    assert torch.equal(r0, s0)
    recv.round(1, d_in=r0)
    s1 = send.round(1, d_in=s0)
    recv.round(2, d_in=s1)
    st = _result(ctx, recv, signature=False)["status"]
    for b in range(B):
        assert list(st[:, b]) == [202 if c.tweaks[b] else 0] * S, f"session {b}"
    recv.close()
    send.close()


# ---- g ---------------------------------------------------------------------------------------------------------------------------
def test_g_what_a_session_with_tweaks_is_refused(gpu_ctx, case):
    from multi_party_ecdsa_amd import engine as E, _native as N
    c, ctx = case, gpu_ctx
    sess = E.Gg20Session(ctx, c.gk, B, list(range(S)), c.dn, sigset=c.ds, tweaks=c.dt)
    slabs, prev = _rounds(ctx, sess, c.dn["msg"], upto=6)
    pool = E.PresigPool(ctx, c.gk, list(range(S)), B)
    before = pool.audit()
    with pytest.raises(N.MpeError, match=r"rc=-1\b.*tweaks"):
        pool.deposit(sess)
    assert pool.audit() == before and before["READY"] == 0 and pool.free_slots() == B
    with pytest.raises(N.MpeError, match=r"rc=-1\b.*tweaks"):
        sess.blame6_state(_dev(ctx, F.words([1] * (B * S), 8)))
    # the refusals left the session where it was: it signs
    more, _ = _rounds(ctx, sess, c.dn["msg"], start=7, prev=prev)
    res = _result(ctx, sess)
    assert np.array_equal(more[7], c.want["slabs"][7]) and not res["status"].any()
    _same_signatures(res["r"][0], res["s"][0], res["recid"][0], c.want)
    sess.close()
    pool.close()
    plain = E.Gg20Session(ctx, c.gk, B, list(range(S)), c.dn, sigset=c.ds)
    with pytest.raises(N.MpeError, match=r"rc=-1\b.*tweaks"):
        plain.rearm(c.dn, sigset=c.ds, tweaks=c.dt)
    plain.close()
