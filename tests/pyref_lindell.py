"""Pure-Python restatement of Lindell'17 key generation, the ephemeral exchange, the signature check and key rotation, written from
the reference text (ZenGo-X/multi-party-ecdsa v0.8.1, src/protocols/two_party_ecdsa/lindell_2017/{party_one,party_two}.rs) on Python
integers and hashlib, over the pieces pyref.py / pyref_gg20.py already restate (DLogProof, ECDDHProof, HashCommitment, Paillier,
PDLwSlackProof, CompositeDLogProof, NiCorrectKeyProof).  It is the checker of the device's mpe_lindell_keygen.h; the CPU tests pin
it against the C oracle wherever the oracle has the piece.

Sampled values are arguments of the per-message functions.  `keygen`, `eph_exchange` and `rotate` replay the device sampler's
streams (orc.sample_* expand the same seed: oracle/sampler_oracle.c), field f of a call = stream counter | f << 56."""
import hashlib
import math

import numpy as np

import orc
import pyref as R
import pyref_gg20 as RG

Q, G, H2, P = R.Q, R.G, R.H2, R.P

# stream fields of the chains (DESIGN.md §12 lists them beside the key-material fields 0..7)
F_PT, F_QT, F_H1, F_XHI = 6, 7, 14, 15                                                     # mpe_lindell_ntilde_generate
F_X1, F_X2, F_BLIND_PK, F_BLIND_POK, F_NONCE1, F_NONCE2 = 16, 17, 18, 19, 20, 21           # the long-term first messages
F_ENC_R, F_CDLOG_R, F_PDL_ALPHA, F_PDL_BETA, F_PDL_RHO, F_PDL_GAMMA = 22, 23, 24, 25, 26, 27
F_K1, F_K2, F_EPH_NONCE1, F_EPH_NONCE2, F_EPH_BLIND_PK, F_EPH_BLIND_POK = 32, 33, 34, 35, 36, 37


def valid_point(pt):
    """what curv accepts when it deserialises a point: canonical coordinates, on the curve, not the neutral element"""
    return pt is not None and 0 <= pt[0] < P and 0 <= pt[1] < P and (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0


def commit_point(pt, blind):
    """HashCommitment(BigInt::from_bytes(P.to_bytes(true)), blind)"""
    return RG.hash_commitment(pt, blind)


def commit_bigint(m, blind):
    """HashCommitment::create_commitment_with_user_defined_randomness(m, blind): SHA-256 over to_bytes(m) | to_bytes(blind)"""
    return R.hash_bigints([m, blind])


def points_digest(a1, a2):
    """Sha256::new().chain_points([a1, a2]).result_bigint() — not reduced mod q (party_two.rs:347-349)"""
    return int.from_bytes(hashlib.sha256(R.chain_point_bytes(a1) + R.chain_point_bytes(a2)).digest(), "big")


# ---- the long-term exchange ---------------------------------------------------------------------------------------------
def keygen_first_msg(x1, nonce, blind_pk, blind_pok):
    """party one, KeyGenFirstMsg::create_commitments_with_fixed_secret_share (party_one.rs:179-219)"""
    Q1, Rp, z = R.dlog_prove(x1 % Q, nonce % Q)
    return dict(Q1=Q1, R=Rp, z=z, pk_com=commit_point(Q1, blind_pk), pok_com=commit_point(Rp, blind_pok))


def keygen_verify_first_msg(pk_com, pok_com, blind_pk, blind_pok, Q1, Rp, z):
    """party two, KeyGenSecondMsg::verify_commitments_and_dlog_proof (party_two.rs:180-223)"""
    if not (valid_point(Q1) and valid_point(Rp)):
        return False
    if pk_com != commit_point(Q1, blind_pk) or pok_com != commit_point(Rp, blind_pok):
        return False
    return R.dlog_verify(Q1, Rp, z % Q)


# ---- the ephemeral exchange ---------------------------------------------------------------------------------------------
def eph_first_msg(k2, nonce, blind_pk, blind_pok):
    """party two, EphKeyGenFirstMsg::create_commitments (party_two.rs:315-371)"""
    pub, c = R.ec_mul(k2, G), R.ec_mul(k2, H2)
    a1, a2, z = RG.ecddh_prove(k2 % Q, nonce % Q, G, pub, H2, c)
    return dict(pub=pub, c=c, a1=a1, a2=a2, z=z, pk_com=commit_point(pub, blind_pk),
                pok_com=commit_bigint(points_digest(a1, a2), blind_pok))


def eph_verify_first_msg(pk_com, pok_com, blind_pk, blind_pok, pub, c, a1, a2, z):
    """party one, EphKeyGenSecondMsg::verify_commitments_and_dlog_proof (party_one.rs:437-483)"""
    if not all(valid_point(p) for p in (pub, c, a1, a2)):
        return False
    if pk_com != commit_point(pub, blind_pk) or pok_com != commit_bigint(points_digest(a1, a2), blind_pok):
        return False
    return RG.ecddh_verify(G, pub, H2, c, a1, a2, z % Q)


def eph_p1_first_msg(k1, nonce):
    """party one, EphKeyGenFirstMsg::create (party_one.rs:403-434)"""
    pub, c = R.ec_mul(k1, G), R.ec_mul(k1, H2)
    a1, a2, z = RG.ecddh_prove(k1 % Q, nonce % Q, G, pub, H2, c)
    return dict(pub=pub, c=c, a1=a1, a2=a2, z=z)


# ---- party_one::verify (party_one.rs:567-592) -------------------------------------------------------------------------------
def verify(pub, msg, r, s):
    if not valid_point(pub):
        return False
    if not (1 <= s and s < Q - s):                            # s = 0 would panic in invert().unwrap(); s >= q gives q - s <= 0
        return False
    si = pow(s, -1, Q)
    pt = R.ec_add(R.ec_mul(msg % Q * si % Q, G), R.ec_mul(r % Q * si % Q, pub))
    return pt is not None and pt[0] == r                      # x_coord().unwrap() panics at infinity; the bytes compared are the integers'


# ---- generate_h1_h2_n_tilde (party_one.rs:594-607) ---------------------------------------------------------------------------
def _words(vals, k32):
    return np.array([[(v >> (32 * j)) & 0xffffffff for j in range(k32)] for v in vals], dtype=np.uint32)


def _ints(arr):
    return [sum(int(w) << (32 * j) for j, w in enumerate(row)) for row in arr]


def h2_of(h1, xhi, nt):
    return pow(pow(h1, -1, nt), xhi, nt)


def ntilde_generate(seed, counter, count):
    """dict of lists Nt, h1, h2, xhi (+ phi) and `fail`: the primes by tests/pyref_primes.py's restatement of the search (fields 6, 7),
    h1 = sample_below(phi) (14), xhi = sample_below(2^256) (15); a failed item is all zero"""
    import pyref_primes as PP
    seed = bytes(seed)
    sid = lambda f: counter | (f << 56)
    pt, _, _ = PP.sample_primes(seed, sid(F_PT), count)
    qt, _, _ = PP.sample_primes(seed, sid(F_QT), count)
    phi = [(a - 1) * (b - 1) if a and b else 0 for a, b in zip(pt, qt)]
    h1s, _ = orc.sample_below(count, seed, sid(F_H1), _words([f or 1 for f in phi], 64), 64)
    xs, _ = orc.sample_below(count, seed, sid(F_XHI), _words([1 << 256], 9), 9)
    out = dict(Nt=[], h1=[], h2=[], xhi=[], phi=[], fail=0)
    for a, b, f, h1, x in zip(pt, qt, phi, _ints(h1s), _ints(xs)):
        nt = a * b
        if not f or math.gcd(h1, nt) != 1:
            for k in ("Nt", "h1", "h2", "xhi", "phi"):
                out[k].append(0)
            out["fail"] += 1
            continue
        out["Nt"].append(nt); out["h1"].append(h1); out["h2"].append(h2_of(h1, x, nt)); out["xhi"].append(x); out["phi"].append(f)
    return out


# ---- the chains: test_full_key_gen, the ephemeral exchange both ways, rotation ------------------------------------------------
def _scalars(B, seed, sid):
    return _ints(orc.sample_scalar(B, seed, sid)[0])


def _bits(B, seed, sid, bits, words):
    return _ints(orc.sample_bits(B, seed, sid, bits, words))


def _below(B, seed, sid, bounds, words, flags=0):
    return _ints(orc.sample_below(B, seed, sid, _words(bounds, words), words, None, flags)[0])


def paillier_half(seed, counter, x1, q1, material=None):
    """generate_keypair_and_encrypted_share, generate_ni_proof_correct_key, verify_ni_proof_correct_key, pdl_proof, pdl_verify
    (party_one.rs:319-401, party_two.rs:275-311) for the shares x1 — what keygen and rotate share.
    material: dict of int lists p, q, pt, qt, h1, xhi; None = minted from the streams (fields 0, 1 and ntilde_generate)."""
    import pyref_primes as PP
    seed, B = bytes(seed), len(x1)
    sid = lambda f: counter | (f << 56)
    fail = 0
    if material is None:
        p, q, N, fail = PP.paillier_keygen(seed, counter, B)
        nt = ntilde_generate(seed, counter, B)
        fail += nt["fail"]
        Nt, h1, h2, xhi = nt["Nt"], nt["h1"], nt["h2"], nt["xhi"]
    else:
        p, q = list(material["p"]), list(material["q"])
        N = [a * b for a, b in zip(p, q)]
        Nt = [a * b for a, b in zip(material["pt"], material["qt"])]
        h1, xhi = list(material["h1"]), list(material["xhi"])
        h2 = [h2_of(h, x, n) for h, x, n in zip(h1, xhi, Nt)]
    r = _below(B, seed, sid(F_ENC_R), N, 64)                                             # Randomness::sample(&ek)
    c_key = [R.paillier_encrypt(n, x, rr) for n, x, rr in zip(N, x1, r)]
    sigma = [R.correct_key_prove(a, b) for a, b in zip(p, q)]
    ok_ck = [n.bit_length() >= 2047 and R.correct_key_verify(n, s) for n, s in zip(N, sigma)]   # party_two.rs:302-311
    cd_r = _bits(B, seed, sid(F_CDLOG_R), 512, 16)
    cd = [R.composite_dlog_prove(n, g, ni, x, rr) for n, g, ni, x, rr in zip(Nt, h1, h2, xhi, cd_r)]
    al = _below(B, seed, sid(F_PDL_ALPHA), [Q ** 3], 24)
    be = _below(B, seed, sid(F_PDL_BETA), [n - 2 for n in N], 64, orc.SAMPLE_PLUS_ONE)
    rh = _below(B, seed, sid(F_PDL_RHO), [Q * n for n in Nt], 72)
    ga = _below(B, seed, sid(F_PDL_GAMMA), [Q ** 3 * n for n in Nt], 88)
    Qs = [R.ec_mul(x, G) for x in x1]
    pdl = [R.pdl_prove(N[i], Nt[i], h1[i], h2[i], c_key[i], Qs[i], G, x1[i], r[i], al[i], be[i], rh[i], ga[i]) for i in range(B)]
    ok_pdl = [Qs[i] == q1[i] and R.composite_dlog_verify(Nt[i], h1[i], h2[i], *cd[i]) and
              R.pdl_verify(N[i], Nt[i], h1[i], h2[i], c_key[i], Qs[i], G, pdl[i]) for i in range(B)]
    return dict(p=p, q=q, N=N, c_key=c_key, r=r, Nt=Nt, h1=h1, h2=h2, xhi=xhi, sigma=sigma, cdlog=cd, pdl=pdl, Q=Qs,
                ok=[int(a and b) for a, b in zip(ok_ck, ok_pdl)], failures=fail)


def keygen(seed, counter, B, x1=None, x2=None, material=None):
    """test_full_key_gen (lindell_2017/test.rs) for B wallets, every draw from the streams of (seed, counter)"""
    seed = bytes(seed)
    sid = lambda f: counter | (f << 56)
    x1 = _scalars(B, seed, sid(F_X1)) if x1 is None else [x % Q for x in x1]
    x2 = _scalars(B, seed, sid(F_X2)) if x2 is None else [x % Q for x in x2]
    bpk, bpok = _bits(B, seed, sid(F_BLIND_PK), 256, 8), _bits(B, seed, sid(F_BLIND_POK), 256, 8)
    n1, n2 = _scalars(B, seed, sid(F_NONCE1)), _scalars(B, seed, sid(F_NONCE2))
    m1 = [keygen_first_msg(x1[i], n1[i], bpk[i], bpok[i]) for i in range(B)]
    m2 = [R.dlog_prove(x2[i], n2[i]) for i in range(B)]                                  # party two's KeyGenFirstMsg::create
    ok1 = [R.dlog_verify(*m) for m in m2]                                                # party one's verify_and_decommit
    ok2 = [keygen_verify_first_msg(m["pk_com"], m["pok_com"], bpk[i], bpok[i], m["Q1"], m["R"], m["z"]) for i, m in enumerate(m1)]
    Q1, Q2 = [m["Q1"] for m in m1], [m[0] for m in m2]
    half = paillier_half(seed, counter, x1, Q1, material)
    pub1 = [R.ec_mul(x1[i], Q2[i]) for i in range(B)]                                    # compute_pubkey on both sides
    pub2 = [R.ec_mul(x2[i], Q1[i]) for i in range(B)]
    ok = [int(ok1[i] and ok2[i] and half["ok"][i] and pub1[i] == pub2[i]) for i in range(B)]
    return dict(ok=ok, failures=half["failures"], x1=x1, x2=x2, Q1=Q1, Q2=Q2, pubkey=pub1, p=half["p"], q=half["q"], N=half["N"],
                c_key=half["c_key"], r=half["r"], first_msg=m1, half=half)


def eph_exchange(seed, counter, B):
    """both ephemeral first messages and both verdicts; returns ok, k1, k2, R1, R2"""
    seed = bytes(seed)
    sid = lambda f: counter | (f << 56)
    k1, k2 = _scalars(B, seed, sid(F_K1)), _scalars(B, seed, sid(F_K2))
    s1, s2 = _scalars(B, seed, sid(F_EPH_NONCE1)), _scalars(B, seed, sid(F_EPH_NONCE2))
    bpk, bpok = _bits(B, seed, sid(F_EPH_BLIND_PK), 256, 8), _bits(B, seed, sid(F_EPH_BLIND_POK), 256, 8)
    m1 = [eph_p1_first_msg(k1[i], s1[i]) for i in range(B)]
    m2 = [eph_first_msg(k2[i], s2[i], bpk[i], bpok[i]) for i in range(B)]
    okA = [RG.ecddh_verify(G, m["pub"], H2, m["c"], m["a1"], m["a2"], m["z"]) for m in m1]      # party two's verify_and_decommit
    okB = [eph_verify_first_msg(m["pk_com"], m["pok_com"], bpk[i], bpok[i], m["pub"], m["c"], m["a1"], m["a2"], m["z"]) for i, m in enumerate(m2)]
    return dict(ok=[int(a and b) for a, b in zip(okA, okB)], k1=k1, k2=k2, R1=[m["pub"] for m in m1], R2=[m["pub"] for m in m2])


def rotate(wallet, factor, seed, counter, factor2=None, material=None):
    """Party1Private::refresh_private_key (party_one.rs:246-296) over x1 f; Party2Private::update_private_key (party_two.rs:241-246)
    over x2 factor2 when factor2 is given.  What party two checks the new statement against is f Q1."""
    x1 = [x * f % Q for x, f in zip(wallet["x1"], factor)]
    q1 = [R.ec_mul(f, p) for f, p in zip(factor, wallet["Q1"])]
    half = paillier_half(seed, counter, x1, q1, material)
    out = dict(wallet)
    out.update(x1=x1, Q1=q1, p=half["p"], q=half["q"], N=half["N"], c_key=half["c_key"], r=half["r"], ok=half["ok"],
               failures=half["failures"], half=half)
    if factor2 is not None:
        out["x2"] = [x * f % Q for x, f in zip(wallet["x2"], factor2)]
        out["Q2"] = [R.ec_mul(f, p) for f, p in zip(factor2, wallet["Q2"])]
    return out
