"""Independent pure-Python restatement of GG18 threshold signing, function by function, written from the reference text
(ZenGo-X/multi-party-ecdsa v0.8.1; citations relative to /root/reference/src unless they name examples/):

  SignKeys / LocalSignature / verify    protocols/multi_party_ecdsa/gg_2018/party_i.rs:384-737
  MessageA / MessageB with `&[]`        utilities/mta/mod.rs:62-179
  the ten rounds of one signer          examples/gg18_sign_client.rs:99-503

Python ints and (x, y) tuples over pyref.py / pyref_gg20.py; it imports nothing from multi_party_ecdsa_amd.  Every value the reference
draws from OsRng is an argument.  `sign_session` plays gg18_sign_client.rs for all signers of ONE session and keeps every message.

Where the reference cannot reach a state (it panics, or curv refuses to deserialise a point) the rule is written at the place:
  * a point that is not on the curve, not canonical or neutral fails the check that reads it (`pt_valid`);
  * a party that has failed goes on in lock step but every word it sends afterwards is zero (a zero point is the neutral encoding,
    which no receiver accepts)."""
import pyref as R
import pyref_gg20 as PG

Q, G, P = R.Q, R.G, R.P


class Gg18Error(Exception):
    """Error::{InvalidKey, InvalidCom, InvalidSig} of the reference, or a panic (`what` says which)"""

    def __init__(self, what):
        super().__init__(what)
        self.what = what


def pt_valid(p):
    """what curv's Point deserialisation accepts: canonical coordinates, on y^2 = x^3 + 7, not the neutral point"""
    return p is not None and 0 <= p[0] < P and 0 <= p[1] < P and (p[1] * p[1] - p[0] ** 3 - 7) % P == 0


def scalar_ok(x):
    """a value Scalar::random() can return"""
    return 0 < x < Q


def points_digest(pts):
    """Sha256::new().chain_points(pts).result_bigint(): not reduced mod q"""
    import hashlib
    h = hashlib.sha256()
    for p in pts:
        h.update(R.chain_point_bytes(p))
    return int.from_bytes(h.digest(), "big")


def commit(m, blind):
    """HashCommitment::create_commitment_with_user_defined_randomness(m, blind)"""
    return R.hash_bigints([m, blind])


def x_mod_q(pt):
    """Scalar::from(&R.x_coord().unwrap().mod_floor(group_order))"""
    return pt[0] % Q


# ---- utilities/mta/mod.rs with an empty statement set ------------------------------------------------------------------
def message_a(a, N, r):
    """MessageA::a_with_predefined_randomness(a, ek, r, &[])  mta/mod.rs:62-87: no range proof"""
    return R.paillier_encrypt(N, a % Q, r)                                              # :68-75


def message_b(b, N, c_a, r, beta_tag, nonce_b, nonce_bt):
    """MessageB::b_with_predefined_randomness(b, ek, m_a, r, beta_tag, &[])  mta/mod.rs:111-158 -> (m_b, beta)"""
    NN = N * N                                                                          # :119-131 hold trivially: both lists are empty
    beta_tag_fe = beta_tag % Q                                                          # :132
    c_beta_tag = R.paillier_encrypt(N, beta_tag, r)                                     # :133-137
    c_b = pow(c_a, b % Q, NN) * c_beta_tag % NN                                         # :139-145
    beta = (-beta_tag_fe) % Q                                                           # :146
    return dict(c=c_b, b_proof=R.dlog_prove(b % Q, nonce_b % Q), beta_tag_proof=R.dlog_prove(beta_tag_fe, nonce_bt % Q)), beta   # :147-148


def verify_proofs_get_alpha(m_b, p, q, a):
    """MessageB::verify_proofs_get_alpha(dk, a)  mta/mod.rs:160-179 -> alpha, or InvalidKey"""
    bp, btp = m_b["b_proof"], m_b["beta_tag_proof"]
    if not all(pt_valid(x) for x in (bp[0], bp[1], btp[0], btp[1])):
        raise Gg18Error("InvalidKey")
    alpha = R.paillier_decrypt_textbook(p, q, m_b["c"]) % Q                             # :165-167
    ba_btag = R.ec_add(R.ec_mul(a, bp[0]), btp[0])                                      # :169
    if R.dlog_verify(*bp) and R.dlog_verify(*btp) and ba_btag == R.ec_mul(alpha, G):    # :170-173
        return alpha
    raise Gg18Error("InvalidKey")                                                       # :177


# ---- gg_2018/party_i.rs:384-484 ----------------------------------------------------------------------------------------------
class SignKeys:
    @classmethod
    def create(cls, x_i, index, s, k_i, gamma_i):
        """SignKeys::create(private, vss_scheme, index, s)  :385-406; index = the position of this party in s"""
        self = cls()
        li = PG.lagrange(s, index)                                                      # :391-392 map_share_to_new_params
        self.w_i = li * x_i % Q                                                         # :393
        self.g_w_i = R.ec_mul(self.w_i, G)                                              # :395
        self.gamma_i = gamma_i % Q                                                      # :396
        self.g_gamma_i = R.ec_mul(self.gamma_i, G)                                      # :397
        self.k_i = k_i % Q                                                              # :402
        return self

    def phase1_broadcast(self, blind_factor):
        """:408-424 -> (SignBroadcastPhase1.com, SignDecommitPhase1)"""
        com = commit(R.pt_as_bigint(self.g_gamma_i), blind_factor)                      # :412-415
        return com, dict(blind_factor=blind_factor, g_gamma_i=self.g_gamma_i)

    def phase2_delta_i(self, alpha_vec, beta_vec):
        assert len(alpha_vec) == len(beta_vec)                                          # :431
        return (self.k_i * self.gamma_i + sum(alpha_vec) + sum(beta_vec)) % Q           # :432-433

    def phase2_sigma_i(self, miu_vec, ni_vec):
        assert len(miu_vec) == len(ni_vec)                                              # :441
        return (self.k_i * self.w_i + sum(miu_vec) + sum(ni_vec)) % Q                   # :442-443

    @staticmethod
    def phase3_reconstruct_delta(delta_vec):
        tot = sum(delta_vec) % Q                                                        # :447-450
        if tot == 0:
            raise Gg18Error("panic: sum of deltas is zero")                             # :451
        return pow(tot, -1, Q)

    @staticmethod
    def phase4(delta_inv, b_proof_vec, phase1_decommit_vec, bc1_vec):
        """:454-483 -> R of the decommitments handed in, or InvalidKey"""
        if not all(pt_valid(d["g_gamma_i"]) for d in phase1_decommit_vec):
            raise Gg18Error("InvalidKey")                                               # no SignDecommitPhase1 can hold such a point
        ok = all(b_proof_vec[i][0] == phase1_decommit_vec[i]["g_gamma_i"] and
                 commit(R.pt_as_bigint(phase1_decommit_vec[i]["g_gamma_i"]), phase1_decommit_vec[i]["blind_factor"]) == bc1_vec[i]
                 for i in range(len(b_proof_vec)))                                      # :463-469
        if not ok:
            raise Gg18Error("InvalidKey")                                               # :481
        gamma_sum = None
        for d in phase1_decommit_vec:
            gamma_sum = R.ec_add(gamma_sum, d["g_gamma_i"])                             # :473-476
        return R.ec_mul(delta_inv, gamma_sum) if gamma_sum is not None else None        # :478


# ---- gg_2018/party_i.rs:486-737 ----------------------------------------------------------------------------------------------
class LocalSignature:
    @classmethod
    def phase5_local_sig(cls, k_i, message, Rp, sigma_i, pubkey, l_i, rho_i):
        """:487-511; a neutral R: x_coord().unwrap() panics"""
        if Rp is None:
            raise Gg18Error("panic: R is the point at infinity")                        # :496-497
        self = cls()
        m_fe = message % Q                                                              # :494
        r = x_mod_q(Rp)                                                                 # :495-499
        self.s_i = (m_fe * k_i + r * sigma_i) % Q                                       # :500
        self.l_i, self.rho_i = l_i % Q, rho_i % Q                                       # :501-502
        self.R, self.m, self.y = Rp, message, pubkey
        return self

    def phase5a_broadcast_5b_zkproof(self, blind_factor, s1, s2, nonce):
        """:513-559 -> (Phase5Com1.com, Phase5ADecom1, HomoELGamalProof, DLogProof)"""
        A_i = R.ec_mul(self.rho_i, G)                                                   # :523
        B_i = R.ec_mul(self.l_i * self.rho_i % Q, G)                                    # :524-525
        V_i = R.ec_add(R.ec_mul(self.s_i, self.R), R.ec_mul(self.l_i, G))               # :526
        com = commit(points_digest([V_i, A_i, B_i]), blind_factor)                      # :527-533
        # witness {r: l_i, x: s_i}; statement {G: A_i, H: R, Y: g, D: V_i, E: B_i}      :534-544
        proof = PG.heg_prove(self.s_i, self.l_i, s1 % Q, s2 % Q, A_i, self.R, G, V_i, B_i)     # :546
        dlog_proof_rho = R.dlog_prove(self.rho_i, nonce % Q)                            # :545
        return com, dict(V_i=V_i, A_i=A_i, B_i=B_i, blind_factor=blind_factor), proof, dlog_proof_rho

    def phase5c(self, decom_vec, com_vec, elgamal_proofs, dlog_proofs_rho, v_i, Rp, blind_factor):
        """:561-636 -> (Phase5Com2.com, Phase5DDecom2), or InvalidCom"""
        assert len(decom_vec) == len(com_vec)                                           # :570
        pts = [v_i, Rp, self.y]
        for d, e, dl in zip(decom_vec, elgamal_proofs, dlog_proofs_rho):
            pts += [d["V_i"], d["A_i"], d["B_i"], e["T"], e["A3"], dl[0], dl[1]]
        if not all(pt_valid(x) for x in pts):
            raise Gg18Error("InvalidCom")                                               # none of these deserialises
        ok = all(commit(points_digest([d["V_i"], d["A_i"], d["B_i"]]), d["blind_factor"]) == c and
                 PG.heg_verify(e, d["A_i"], Rp, G, d["V_i"], d["B_i"]) and R.dlog_verify(*dl)
                 for d, c, e, dl in zip(decom_vec, com_vec, elgamal_proofs, dlog_proofs_rho))          # :573-592
        v, a = v_i, None
        for d in decom_vec:
            v = R.ec_add(v, d["V_i"])                                                   # :594-597
            a = R.ec_add(a, d["A_i"])                                                   # :595,599
        r = x_mod_q(self.R)                                                             # :601-607
        v = R.ec_add(R.ec_add(v, R.ec_neg(R.ec_mul(self.m % Q, G))), R.ec_neg(R.ec_mul(r, self.y)))   # :608-612
        u_i = R.ec_mul(self.rho_i, v) if v is not None else None                        # :613
        t_i = R.ec_mul(self.l_i, a) if a is not None else None                          # :614
        com = commit(points_digest([u_i, t_i]), blind_factor)                           # :615-620
        if not ok:
            raise Gg18Error("InvalidCom")                                               # :634
        return com, dict(u_i=u_i, t_i=t_i, blind_factor=blind_factor)

    def phase5d(self, decom_vec2, com_vec2, decom_vec1):
        """:638-673 -> s_i, or InvalidCom / InvalidKey"""
        assert len(decom_vec2) == len(decom_vec1) == len(com_vec2)                      # :644-645
        if not all(pt_valid(x) for d2, d1 in zip(decom_vec2, decom_vec1) for x in (d2["u_i"], d2["t_i"], d1["B_i"])):
            raise Gg18Error("InvalidCom")
        test_com = all(commit(points_digest([d["u_i"], d["t_i"]]), d["blind_factor"]) == c for d, c in zip(decom_vec2, com_vec2))   # :647-655
        tb = G
        for d in decom_vec2:
            tb = R.ec_add(tb, d["t_i"])
        for d in decom_vec1:
            tb = R.ec_add(tb, d["B_i"])                                                 # :657-662
        us = None
        for d in decom_vec2:
            us = R.ec_add(us, d["u_i"])
        if not test_com:
            raise Gg18Error("InvalidCom")                                               # :671
        if R.ec_add(tb, R.ec_neg(us)) != G:
            raise Gg18Error("InvalidKey")                                               # :668
        return self.s_i

    def output_signature(self, s_vec):
        """:674-712 -> (r, s, recid), or InvalidSig"""
        if not pt_valid(self.R) or not pt_valid(self.y):
            raise Gg18Error("InvalidSig")                                               # :682
        s = (self.s_i + sum(s_vec)) % Q                                                 # :675
        r = x_mod_q(self.R)                                                             # :678-684
        recid = (self.R[1] % Q) & 1                                                     # :685-698
        s_tag = Q - s                                                                   # :699
        if s > s_tag:
            s, recid = s_tag % Q, recid ^ 1                                             # :700-703
        if not verify((r, s), self.y, self.m):                                          # :705
            raise Gg18Error("InvalidSig")
        return r, s, recid


def verify(sig, y, message):
    """:714-737: no low-s rule; x compared modulo q"""
    r, s = sig
    if s % Q == 0:
        return False                                                                    # :715
    b = pow(s, -1, Q)
    u1, u2 = (message % Q) * b % Q, r * b % Q                                           # :716-718
    pt = R.ec_add(R.ec_mul(u1, G), R.ec_mul(u2, y))                                     # :720-722
    return pt is not None and pt[0] % Q == r                                            # :725-731


# ---- examples/gg18_sign_client.rs for every signer of one session -------------------------------------------------------------
STATUS = {"InvalidKey@alpha": 201, "pk@w": 202, "panic: sum of deltas is zero": 301, "InvalidKey@phase4": 401,
          "panic: R is the point at infinity": 402, "InvalidCom@5c": 531, "InvalidCom@5d": 541, "InvalidKey@5d": 542, "InvalidSig": 601}
ZERO_DLOG = (None, None, 0)
ZERO_HEG = dict(T=None, A3=None, z1=0, z2=0)
ZERO_MB = dict(c=0, b_proof=ZERO_DLOG, beta_tag_proof=ZERO_DLOG)
DRAW_FIELDS = ("k", "gamma", "blind", "r_a", "mb_beta_tag", "mb_r", "mb_nonce_b", "mb_nonce_bt", "l", "rho", "blind5a", "heg_s1", "heg_s2",
               "dlog_nonce", "blind5c")


def ind_of(i, jj):
    """peer slot jj of signer ordinal i -> that peer's ordinal (test.rs:213)"""
    return jj if jj < i else jj + 1


def slot_of(i, ind):
    """the slot signer ordinal i has among the peers of ordinal `ind`"""
    return i if i < ind else i - 1


def sign_session(wallet, signers, message, draws, tamper=None):
    """wallet: dict(n, x[n], p[n], q[n], N[n], X[n] (pk_vec), y).  draws: per signer ordinal, DRAW_FIELDS; the mb_* fields are
    [S][S-1][2] (peer slot, then 0 = gamma side / 1 = w side), the others [S].  tamper(round, msgs, draws) may edit the messages of
    round 1..9 (and the draws) in place before anybody reads them.
    Returns dict(msgs, status [S], sig [S] (r, s, recid) or None, R [S]).  msgs fields are indexed by SENDER ordinal:
      1 com, c_a | 2 mb [S][S-1][2] | 3 delta | 4 blind, g_gamma | 5 com5a | 6 V, A, B, blind5a, heg, dlog | 7 com5c |
      8 u, t, blind5c | 9 s_i
    Every party reads every broadcast value, its own included, from msgs (the layout of the batched calls: own value included)."""
    S = len(signers)
    status = [0] * S
    msgs = {}
    hook = (lambda rnd: tamper(rnd, msgs, draws)) if tamper else (lambda rnd: None)
    alive = lambda i: status[i] == 0

    def fail(i, code):
        if status[i] == 0:
            status[i] = code

    N = lambda j: wallet["N"][signers[j]]
    # SignKeys::create (client :101-106); a k_i / gamma_i that Scalar::random() cannot return stops the party: status 91
    keys = []
    for i in range(S):
        if not (scalar_ok(draws["k"][i]) and scalar_ok(draws["gamma"][i])):
            fail(i, 91)
        keys.append(SignKeys.create(wallet["x"][signers[i]], i, signers, draws["k"][i], draws["gamma"][i]))
    g_w = [R.ec_mul(PG.lagrange(signers, j), wallet["X"][signers[j]]) if pt_valid(wallet["X"][signers[j]]) else None
           for j in range(S)]                                                           # Keys::update_commitments_to_xi (client :235-240)
    # round 1 (client :110-147)
    own_decommit = []
    msgs["com"], msgs["c_a"] = [0] * S, [0] * S
    for i in range(S):
        if not alive(i):
            own_decommit.append(dict(blind_factor=0, g_gamma_i=None))
            continue
        msgs["com"][i], dec = keys[i].phase1_broadcast(draws["blind"][i])
        own_decommit.append(dec)
        msgs["c_a"][i] = message_a(keys[i].k_i, N(i), draws["r_a"][i])
    hook(1)
    # round 2 (client :151-195): two MessageB per peer
    beta = [[[0, 0] for _ in range(S - 1)] for _ in range(S)]
    msgs["mb"] = [[[dict(ZERO_MB), dict(ZERO_MB)] for _ in range(S - 1)] for _ in range(S)]
    for i in range(S):
        for jj in range(S - 1):
            ind = ind_of(i, jj)
            for v, b in enumerate((keys[i].gamma_i, keys[i].w_i)):
                mb, bt = message_b(b, N(ind), msgs["c_a"][ind], draws["mb_r"][i][jj][v], draws["mb_beta_tag"][i][jj][v],
                                   draws["mb_nonce_b"][i][jj][v], draws["mb_nonce_bt"][i][jj][v])
                beta[i][jj][v] = bt
                if alive(i):
                    msgs["mb"][i][jj][v] = mb
    hook(2)
    # client :218-247
    msgs["delta"] = [0] * S
    sigma = [0] * S
    b_pk_gamma = [[None] * (S - 1) for _ in range(S)]
    alpha_all, miu_all = [None] * S, [None] * S
    for i in range(S):
        me = signers[i]
        alpha_vec, miu_vec = [], []
        for jj in range(S - 1):
            ind = ind_of(i, jj)
            pair = msgs["mb"][ind][slot_of(i, ind)]
            b_pk_gamma[i][jj] = pair[0]["b_proof"][0]
            try:
                alpha_vec.append(verify_proofs_get_alpha(pair[0], wallet["p"][me], wallet["q"][me], keys[i].k_i))      # :226-228
                miu_vec.append(verify_proofs_get_alpha(pair[1], wallet["p"][me], wallet["q"][me], keys[i].k_i))        # :230-232
            except Gg18Error:
                fail(i, 201)
                break
            if pair[1]["b_proof"][0] != g_w[ind]:                                       # :241
                fail(i, 202)
                break
        alpha_all[i], miu_all[i] = alpha_vec, miu_vec
        if alive(i):
            msgs["delta"][i] = keys[i].phase2_delta_i(alpha_vec, [b[0] for b in beta[i]])     # :246
            sigma[i] = keys[i].phase2_sigma_i(miu_vec, [b[1] for b in beta[i]])               # :247
    hook(3)
    # round 4 (client :276-309)
    msgs["blind"] = [own_decommit[i]["blind_factor"] if alive(i) else 0 for i in range(S)]
    msgs["g_gamma"] = [own_decommit[i]["g_gamma_i"] if alive(i) else None for i in range(S)]
    hook(4)
    Rv = [None] * S
    for i in range(S):
        if not alive(i):
            continue
        try:
            delta_inv = SignKeys.phase3_reconstruct_delta(msgs["delta"])                # :272
            decommit_vec = [dict(blind_factor=msgs["blind"][j], g_gamma_i=msgs["g_gamma"][j]) for j in range(S)]
            decomm_i = decommit_vec.pop(i)                                              # :300
            bc1_vec = [msgs["com"][j] for j in range(S) if j != i]                      # :301
            b_proof_vec = [(b_pk_gamma[i][jj],) for jj in range(S - 1)]                 # :302-304
            if not pt_valid(decomm_i["g_gamma_i"]):
                raise Gg18Error("InvalidKey")
            Rp = SignKeys.phase4(delta_inv, b_proof_vec, decommit_vec, bc1_vec)         # :305
            Rp = R.ec_add(Rp, R.ec_mul(delta_inv, decomm_i["g_gamma_i"]))               # :309
            if Rp is None:
                raise Gg18Error("panic: R is the point at infinity")
            Rv[i] = Rp
        except Gg18Error as e:
            fail(i, STATUS.get(e.what, STATUS.get(e.what + "@phase4")))
    # 5A (client :313-343), 5B (:346-378)
    local, out5 = [None] * S, [None] * S
    for i in range(S):
        if alive(i):
            local[i] = LocalSignature.phase5_local_sig(keys[i].k_i, message, Rv[i], sigma[i], wallet["y"], draws["l"][i], draws["rho"][i])
            out5[i] = local[i].phase5a_broadcast_5b_zkproof(draws["blind5a"][i], draws["heg_s1"][i], draws["heg_s2"][i], draws["dlog_nonce"][i])
    msgs["com5a"] = [out5[i][0] if alive(i) else 0 for i in range(S)]
    hook(5)
    for f, z in (("V", None), ("A", None), ("B", None), ("blind5a", 0), ("heg", ZERO_HEG), ("dlog", ZERO_DLOG)):
        msgs[f] = [z if not isinstance(z, dict) else dict(z) for _ in range(S)]
    for i in range(S):
        if alive(i):
            _, dec, heg, dl = out5[i]
            msgs["V"][i], msgs["A"][i], msgs["B"][i], msgs["blind5a"][i] = dec["V_i"], dec["A_i"], dec["B_i"], dec["blind_factor"]
            msgs["heg"][i], msgs["dlog"][i] = {f: heg[f] for f in ("T", "A3", "z1", "z2")}, dl
    hook(6)
    # 5C (client :379-427): the draws are read again, a tamper may have changed l_i after 5A
    out5c = [None] * S
    for i in range(S):
        if not alive(i):
            continue
        local[i].l_i = draws["l"][i] % Q
        peers = [j for j in range(S) if j != i]
        decom = [dict(V_i=msgs["V"][j], A_i=msgs["A"][j], B_i=msgs["B"][j], blind_factor=msgs["blind5a"][j]) for j in peers]
        try:
            out5c[i] = local[i].phase5c(decom, [msgs["com5a"][j] for j in peers], [msgs["heg"][j] for j in peers],
                                        [msgs["dlog"][j] for j in peers], msgs["V"][i], Rv[i], draws["blind5c"][i])     # :392-401
        except Gg18Error:
            fail(i, 531)
    msgs["com5c"] = [out5c[i][0] if alive(i) else 0 for i in range(S)]
    hook(7)
    msgs["u"] = [out5c[i][1]["u_i"] if alive(i) else None for i in range(S)]
    msgs["t"] = [out5c[i][1]["t_i"] if alive(i) else None for i in range(S)]
    msgs["blind5c"] = [out5c[i][1]["blind_factor"] if alive(i) else 0 for i in range(S)]
    hook(8)
    # 5D (client :455-483)
    msgs["s_i"] = [0] * S
    for i in range(S):
        if not alive(i):
            continue
        d2 = [dict(u_i=msgs["u"][j], t_i=msgs["t"][j], blind_factor=msgs["blind5c"][j]) for j in range(S)]
        d1 = [dict(B_i=msgs["B"][j]) for j in range(S)]
        try:
            msgs["s_i"][i] = local[i].phase5d(d2, msgs["com5c"], d1)                    # :462-468
        except Gg18Error as e:
            fail(i, STATUS[e.what + "@5d"])
    hook(9)
    sig = [None] * S
    for i in range(S):
        if not alive(i):
            continue
        try:
            sig[i] = local[i].output_signature([msgs["s_i"][j] for j in range(S) if j != i])      # :485-488
        except Gg18Error:
            fail(i, 601)
    # what the parties keep to themselves, for the tests that feed one call at a time
    state = dict(w=[k.w_i for k in keys], g_w_i=[k.g_w_i for k in keys], g_gamma=[k.g_gamma_i for k in keys], g_w=g_w, beta=beta, alpha=alpha_all, miu=miu_all, sigma=sigma,
                 s_i=[loc.s_i if loc else 0 for loc in local])
    return dict(msgs=msgs, status=status, sig=sig, R=Rv, state=state)
