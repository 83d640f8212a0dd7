"""GPU: one GG20 key object that signs for any quorum of its wallet (`mpe_gg20_keys_create_sets`, `mpe_gg20_session_create_sets`,
`mpe_gg20_sign_sets`): every session of a batch names its signer set, and every message, signature, status and bad_actors word equals
the oracle's run of THAT session with THAT set (tests/sigset_cases.py).
 a. lock-step batches over all sets of (1,3), (2,5), (3,8); the existing entry points on a many-set object mean set 0, byte for byte
 b. wallets and sets varying together
 c. one party per object, named by its party index; the test is the relay
 d. refusals: MPE_GG20_STATUS_BAD_SET on the device, MPE_E_ARG on the host
 e. fault injection and blame keep signer ORDINALS of each session's own set"""
import numpy as np
import pytest
import torch

import fixtures as F
import gg20_fixture as G
import pyref
import sigset_cases as SC

pytestmark = pytest.mark.gpu

SHAPES = {"1of3": (1, 3, [0, 1, 2, 2, 0, 1, 1]),
          "2of5": (2, 5, [3, 9, 0, 7, 1, 8, 2, 6, 4, 5, 0]),                    # all ten sets, not in order
          "3of8": (3, 8, [69, 0, 35])}


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _i32(ctx, vals):
    return torch.tensor([int(v) for v in vals], dtype=torch.int32, device=ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _rounds(ctx, sess, msg, first_in=None):
    """all rounds of a session object with every signer local; returns ({round: [L, B, W] numpy}, result dict of numpy arrays)"""
    slabs, prev = {}, first_in
    for rnd in range(9):
        out = sess.round(rnd, d_in=prev, msg=msg if rnd == 7 else None)
        if rnd in G.ROUNDS:
            slabs[rnd] = _u32(out)
            prev = out
    res = sess.result()
    ctx.sync()
    return slabs, {f: (_u32(v) if f in ("r", "s", "R", "bad_actors") else v.cpu().numpy()) for f, v in res.items()}


class Case:
    def __init__(self, keys, name):
        self.t, self.n, self.sigset = SHAPES[name]
        self.S, self.B = self.t + 1, len(self.sigset)
        self.sets = SC.all_sets(self.n, self.S)
        self.lks, self.per_wallet = SC.wallet(keys, self.t, self.n, self.sets)
        self.nonces = SC.mixed_nonces(self.per_wallet, self.sigset, seed=f"sigsets-{name}")
        self.want = SC.oracle_mixed(self.lks, self.nonces, self.sigset)
        assert not self.want["status"].any()


@pytest.fixture(scope="module", params=list(SHAPES))
def case(request, keys):
    return Case(keys, request.param)


@pytest.fixture(scope="module")
def case13(keys):
    return Case(keys, "1of3")


def _check_signatures(res, want, S):
    assert not res["status"].any() and not res["bad_actors"].any()
    for i in range(S):
        assert np.array_equal(res["r"][i], want["r"]) and np.array_equal(res["s"][i], want["s"])
        assert list(res["recid"][i]) == list(want["recid"]) and np.array_equal(res["R"][i], want["R"])


# ---- a. lock-step, byte parity ---------------------------------------------------------------------------------------------------
def test_a_mixed_batch_equals_the_oracle_session_by_session(gpu_ctx, case):
    from multi_party_ecdsa_amd import engine as E
    c, ctx = case, gpu_ctx
    gk = E.Gg20Keys(ctx, c.t, c.n, None, c.lks[0]["arrays"], signer_sets=c.sets)
    dn, ds = {f: _dev(ctx, v) for f, v in c.nonces.items()}, _i32(ctx, c.sigset)
    sess = E.Gg20Session(ctx, gk, c.B, list(range(c.S)), dn, sigset=ds)
    slabs, res = _rounds(ctx, sess, dn["msg"])
    sess.close()
    for rnd in G.ROUNDS:
        for b in range(c.B):
            assert np.array_equal(slabs[rnd][:, b], c.want["slabs"][rnd][:, b]), f"round {rnd}, session {b} (set {c.sets[c.sigset[b]]})"
    _check_signatures(res, c.want, c.S)
    r, s, recid, status, R = [o.cpu().numpy() for o in E.gg20_sign(ctx, gk, dn, c.B, want_R=True, sigset=ds)]
    assert not status.any()
    assert np.array_equal(r.view(np.uint32), c.want["r"]) and np.array_equal(s.view(np.uint32), c.want["s"])
    assert list(recid) == list(c.want["recid"]) and np.array_equal(R.view(np.uint32), c.want["R"])
    r, s, recid, status = [o.cpu().numpy() for o in E.gg20_sign(ctx, gk, dn, c.B, dedup_verify=True, sigset=ds)]
    assert not status.any()
    assert np.array_equal(r.view(np.uint32), c.want["r"]) and np.array_equal(s.view(np.uint32), c.want["s"])
    gk.close()


def test_a_large_batch_code_paths(gpu_ctx_serial, case13):
    """the kernels large batches take (one item per lane in the EC rounds, no forks): the same bytes"""
    from multi_party_ecdsa_amd import engine as E
    c, ctx = case13, gpu_ctx_serial
    gk = E.Gg20Keys(ctx, c.t, c.n, None, c.lks[0]["arrays"], signer_sets=c.sets)
    dn, ds = {f: _dev(ctx, v) for f, v in c.nonces.items()}, _i32(ctx, c.sigset)
    sess = E.Gg20Session(ctx, gk, c.B, list(range(c.S)), dn, sigset=ds)
    slabs, res = _rounds(ctx, sess, dn["msg"])
    sess.close()
    for rnd in G.ROUNDS:
        assert np.array_equal(slabs[rnd], c.want["slabs"][rnd]), f"round {rnd}"
    _check_signatures(res, c.want, c.S)
    gk.close()


def test_a_existing_entry_points_on_a_many_set_object_mean_set_0(gpu_ctx, case):
    """no sigset anywhere: gg20_sign and Gg20Session on the many-set object and on a Gg20Keys(signers=set 0) object, byte for byte"""
    from multi_party_ecdsa_amd import engine as E
    c, ctx, B = case, gpu_ctx, 2
    nonces = G.make_nonces(c.lks[0], B, seed="sigsets-set0")
    dn = {f: _dev(ctx, v) for f, v in nonces.items()}
    got = []
    for kw in (dict(signer_sets=c.sets), dict()):
        gk = E.Gg20Keys(ctx, c.t, c.n, None if kw else c.sets[0], c.lks[0]["arrays"], **kw)
        sign = [o.cpu().numpy() for o in E.gg20_sign(ctx, gk, dn, B, want_R=True)]
        sess = E.Gg20Session(ctx, gk, B, list(range(c.S)), dn)
        slabs, res = _rounds(ctx, sess, dn["msg"])
        sess.close()
        gk.close()
        got.append((sign, slabs, res))
    (sign_m, slabs_m, res_m), (sign_1, slabs_1, res_1) = got
    assert not sign_1[3].any()
    for a, b in zip(sign_m, sign_1):
        assert np.array_equal(a, b)
    for rnd in G.ROUNDS:
        assert np.array_equal(slabs_m[rnd], slabs_1[rnd]), f"round {rnd}"
    for f in res_1:
        assert np.array_equal(res_m[f], res_1[f]), f


# ---- b. wallets and sets together ------------------------------------------------------------------------------------------------
def test_b_key_set_and_signer_set_vary_independently(gpu_ctx, keys):
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, S, B = gpu_ctx, 1, 3, 2, 8
    sets = SC.all_sets(n, S)
    keyset, sigset = [0, 1, 1, 0, 1, 0, 0, 1], [2, 2, 0, 1, 1, 0, 2, 0]
    lks, per_wallet = SC.wallet(keys, t, n, sets, nwallets=2)
    nonces = SC.mixed_nonces(per_wallet, sigset, seed="sigsets-wallets", keyset=keyset)
    want = SC.oracle_mixed(lks, nonces, sigset, keyset=keyset)
    assert not want["status"].any()
    gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], nkeysets=2, signer_sets=sets)
    dn, ds, dk = {f: _dev(ctx, v) for f, v in nonces.items()}, _i32(ctx, sigset), _i32(ctx, keyset)
    sess = E.Gg20Session(ctx, gk, B, list(range(S)), dn, keyset=dk, sigset=ds)
    slabs, res = _rounds(ctx, sess, dn["msg"])
    sess.close()
    for rnd in G.ROUNDS:
        assert np.array_equal(slabs[rnd], want["slabs"][rnd]), f"round {rnd}"
    _check_signatures(res, want, S)
    r, s, recid, status = [o.cpu().numpy() for o in E.gg20_sign(ctx, gk, dn, B, keyset=dk, sigset=ds)]
    assert not status.any() and np.array_equal(r.view(np.uint32), want["r"]) and np.array_equal(s.view(np.uint32), want["s"])
    gk.close()


# ---- c. one party per object, by party index -------------------------------------------------------------------------------------
def test_c_one_party_per_object_named_by_its_index(gpu_ctx, keys):
    """Three objects, one per party of a 2-of-3 wallet, each holding only its own secrets; six global sessions, two per set.  Each
    object's batch is made of the global sessions whose set contains its party; the test routes the records."""
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, S = gpu_ctx, 1, 3, 2
    sets = SC.all_sets(n, S)
    sigset = [0, 2, 1, 1, 0, 2]
    Bg = len(sigset)
    lks, per_wallet = SC.wallet(keys, t, n, sets)
    nonces = SC.mixed_nonces(per_wallet, sigset, seed="sigsets-by-party")
    want = SC.oracle_mixed(lks, nonces, sigset)
    assert not want["status"].any()
    parties = []
    for p in range(n):
        mine = [g for g in range(Bg) if p in sets[sigset[g]]]
        assert len(mine) == 4
        ordinal = [SC.words.rank_in_set(sets[sigset[g]], p) for g in mine]
        parts = [G.party_nonces(SC.session_rows(nonces, Bg, [g]), lks[sigset[g]], i) for g, i in zip(mine, ordinal)]
        zp = {f: np.ascontiguousarray(np.concatenate([q[f] for q in parts])) for f in parts[0]}
        gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], own=[p], signer_sets=sets)
        dn = {f: _dev(ctx, v) for f, v in zp.items()}
        sess = E.Gg20Session(ctx, gk, len(mine), None, dn, sigset=_i32(ctx, [sigset[g] for g in mine]), local_party=p)
        parties.append(dict(p=p, mine=mine, ordinal=ordinal, gk=gk, dn=dn, sess=sess))
    prev = None
    for rnd in range(9):
        W = G.msg_words(S, n, rnd) if rnd in G.ROUNDS else 0
        slab = np.zeros((S, Bg, W), dtype=np.uint32)
        for q in parties:
            d_in = None if prev is None or rnd == 7 else _dev(ctx, prev[:, q["mine"]])          # [sender ordinal][my sessions][W]
            out = q["sess"].round(rnd, d_in=d_in, msg=q["dn"]["msg"] if rnd == 7 else None)
            if W:
                o = _u32(out)
                for row, (g, i) in enumerate(zip(q["mine"], q["ordinal"])):
                    slab[i, g] = o[0, row]
        if W:
            assert np.array_equal(slab, want["slabs"][rnd]), f"round {rnd}"
            prev = slab
    for q in parties:
        res = q["sess"].result()
        ctx.sync()
        assert not res["status"].cpu().numpy().any()
        assert np.array_equal(_u32(res["r"])[0], want["r"][q["mine"]]) and np.array_equal(_u32(res["s"])[0], want["s"][q["mine"]])
        assert list(res["recid"].cpu().numpy()[0]) == list(want["recid"][q["mine"]])
        q["sess"].close()
        q["gk"].close()


# ---- d. refusals -----------------------------------------------------------------------------------------------------------------
def test_d_a_set_index_out_of_range_stops_that_session_alone(gpu_ctx, keys):
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, S = gpu_ctx, 1, 3, 2
    sets = SC.all_sets(n, S)
    named = [0, len(sets), 1, -1, 2]                              # sessions 1 and 3 name no set of the key object
    bad = [b for b, k in enumerate(named) if not 0 <= k < len(sets)]
    good = [b for b in range(len(named)) if b not in bad]
    drawn_for = [k if 0 <= k < len(sets) else 0 for k in named]
    B = len(named)
    lks, per_wallet = SC.wallet(keys, t, n, sets)
    nonces = SC.mixed_nonces(per_wallet, drawn_for, seed="sigsets-refused")
    want = SC.oracle_mixed(lks, nonces, drawn_for)
    gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], signer_sets=sets)
    dn, ds = {f: _dev(ctx, v) for f, v in nonces.items()}, _i32(ctx, named)
    sess = E.Gg20Session(ctx, gk, B, list(range(S)), dn, sigset=ds)
    slabs, res = _rounds(ctx, sess, dn["msg"])
    sess.close()
    for rnd in G.ROUNDS:
        assert not slabs[rnd][:, bad].any(), f"round {rnd}: a refused session emitted a record"
        assert np.array_equal(slabs[rnd][:, good], want["slabs"][rnd][:, good]), f"round {rnd}: the neighbours"
    assert (res["status"][:, bad] == SC.BAD_SET).all() and not res["status"][:, good].any()
    assert not res["r"][:, bad].any() and not res["s"][:, bad].any() and not res["recid"][:, bad].any()
    for i in range(S):
        assert np.array_equal(res["r"][i, good], want["r"][good]) and np.array_equal(res["s"][i, good], want["s"][good])
    r, s, recid, status = [o.cpu().numpy() for o in E.gg20_sign(ctx, gk, dn, B, sigset=ds)]
    assert list(status[bad]) == [SC.BAD_SET] * len(bad) and not status[good].any()
    assert not r[bad].any() and not s[bad].any() and not recid[bad].any()
    assert np.array_equal(r.view(np.uint32)[good], want["r"][good]) and np.array_equal(s.view(np.uint32)[good], want["s"][good])
    gk.close()


def test_d_a_local_party_outside_the_sessions_set(gpu_ctx, keys):
    from multi_party_ecdsa_amd import engine as E
    ctx, t, n, S, p = gpu_ctx, 1, 3, 2, 2
    sets = SC.all_sets(n, S)
    sigset = [0, 1, 2]                                            # {0, 1} does not hold party 2; in {0, 2} and {1, 2} it is ordinal 1
    lks, per_wallet = SC.wallet(keys, t, n, sets)
    nonces = SC.mixed_nonces(per_wallet, sigset, seed="sigsets-outsider")
    want = SC.oracle_mixed(lks, nonces, sigset)
    parts = [G.party_nonces(SC.session_rows(nonces, 3, [g]), lks[sigset[g]], 1) for g in range(3)]
    zp = {f: np.ascontiguousarray(np.concatenate([q[f] for q in parts])) for f in parts[0]}
    gk = E.Gg20Keys(ctx, t, n, None, lks[0]["arrays"], own=[p], signer_sets=sets)
    dn = {f: _dev(ctx, v) for f, v in zp.items()}
    sess = E.Gg20Session(ctx, gk, 3, None, dn, sigset=_i32(ctx, sigset), local_party=p)
    out = _u32(sess.round(0))
    st = sess.result(signature=False)["status"].cpu().numpy()
    assert list(st[0]) == [SC.BAD_SET, 0, 0]
    assert not out[0, 0].any()
    assert np.array_equal(out[0, 1], want["slabs"][0][1, 1]) and np.array_equal(out[0, 2], want["slabs"][0][1, 2])
    sess.close()
    gk.close()


def test_d_what_the_host_refuses(gpu_ctx, keys):
    from multi_party_ecdsa_amd import engine as E, _native as N
    ctx, t, n, S, B = gpu_ctx, 1, 3, 2, 2
    sets = SC.all_sets(n, S)
    lks, _ = SC.wallet(keys, t, n, sets)
    A = lks[0]["arrays"]
    dn = {f: _dev(ctx, v) for f, v in G.make_nonces(lks[0], B, seed="sigsets-host").items()}
    ds = _i32(ctx, [0, 1])

    def refused(what, f):
        with pytest.raises(N.MpeError, match=r"rc=-1\b"):
            f()
    refused("two equal sets", lambda: E.Gg20Keys(ctx, t, n, None, A, signer_sets=[[0, 1], [0, 2], [0, 1]]))
    refused("an unsorted set", lambda: E.Gg20Keys(ctx, t, n, None, A, signer_sets=[[0, 1], [2, 0]]))
    refused("a party index beyond n", lambda: E.Gg20Keys(ctx, t, n, None, A, signer_sets=[[0, 1], [1, 3]]))
    gk = E.Gg20Keys(ctx, t, n, None, A, own=[0, 1], signer_sets=sets)        # party 2 is a member of two sets, its secrets are elsewhere
    refused("lock-step without a member's secrets", lambda: E.Gg20Session(ctx, gk, B, [0, 1], dn, sigset=ds))
    refused("lock-step sign without a member's secrets", lambda: E.gg20_sign(ctx, gk, dn, B, sigset=ds))
    refused("two local parties by index", lambda: E.Gg20Session(ctx, gk, B, [0, 1], dn, sigset=ds, local_party=0))
    refused("a by-index party whose secrets are elsewhere", lambda: E.Gg20Session(ctx, gk, B, None, dn, sigset=ds, local_party=2))
    sess = E.Gg20Session(ctx, gk, B, [0, 1], dn)                             # set 0 = {0, 1} alone: its secrets are all here
    refused("re-arming with sets a session that was made without", lambda: sess.rearm(dn, sigset=ds))
    sess.close()
    gk.close()


# ---- e. faults keep their ordinals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [5, 6, 7])
def test_e_fault_injection_and_blame_name_the_ordinal_of_each_sessions_own_set(gpu_ctx, case13, step):
    from multi_party_ecdsa_amd import engine as E
    c, ctx, mask = case13, gpu_ctx, 0b10
    S, B, P1 = c.S, c.B, c.S - 1
    want_st, want_bad = SC.oracle_mixed_faults(c.lks, c.nonces, c.sigset, step, [1])
    assert (want_st == {5: 502, 6: 602, 7: 701}[step]).all()
    gk = E.Gg20Keys(ctx, c.t, c.n, None, c.lks[0]["arrays"], signer_sets=c.sets)
    dn, ds = {f: _dev(ctx, v) for f, v in c.nonces.items()}, _i32(ctx, c.sigset)
    sess = E.Gg20Session(ctx, gk, B, list(range(S)), dn, sigset=ds)
    sess.fault_inject(step, mask)
    slabs, res = _rounds(ctx, sess, dn["msg"])
    assert np.array_equal(res["status"], want_st) and np.array_equal(res["bad_actors"], want_bad)
    tr = lambda a: np.ascontiguousarray(np.transpose(a, (1, 0, 2)).reshape(B * S, a.shape[2]))
    if step == 5:
        o = G.blame5_opened(c.lks[0], c.nonces, slabs, B)
        got = E.gg20_blame5(ctx, gk, B, {f: _dev(ctx, v) for f, v in o.items()}, sigset=ds)
        assert list(_u32(got)) == [mask] * B
    elif step == 6:
        en = F.words([F.Rng("sigsets-ecddh").below(pyref.Q - 1) + 1 for _ in range(B * S)], 8)
        miu, a1, a2, z = sess.blame6_state(_dev(ctx, en))
        cb = G.blame6_cb(c.lks[0], slabs, B)
        # every key holder opens the w_i ciphertexts it received (Paillier::open) under ITS key: the party at that ordinal of the session's set
        sk_all = E.PaillierKeys(ctx, p=[k.p for k in c.lks[0]["keys"]], q=[k.q for k in c.lks[0]["keys"]])
        kx = _i32(ctx, [c.sets[c.sigset[r // (S * P1)]][(r // P1) % S] for r in range(B * S * P1)])
        om, orr = E.paillier_open(ctx, sk_all, _dev(ctx, cb), kx)
        o = dict(k=c.nonces["k"], k_rand=c.nonces["r_a"], miu=_u32(om), miu_rand=_u32(orr), a1=tr(_u32(a1)), a2=tr(_u32(a2)), z=tr(_u32(z)),
                 S=tr(slabs[5][:, :, 0:16]), c_a=tr(slabs[0][:, :, c.n * 256:c.n * 256 + 128]), c_b=cb, R=res["R"][0])
        assert np.array_equal(tr(_u32(miu).reshape(S, B, -1)).reshape(-1, 64), o["miu"])
        got = E.gg20_blame6(ctx, gk, B, {f: _dev(ctx, v) for f, v in o.items()}, sigset=ds)
        assert list(_u32(got)) == [mask] * B
    sess.close()
    gk.close()
