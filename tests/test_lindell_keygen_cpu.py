"""CPU tests of tests/pyref_lindell.py, the checker of the device's Lindell'17 key generation: it agrees with the unchanged C oracle
wherever the oracle has the piece (DLogProof, the point commitment, Paillier encryption, PDLwSlackProof), both exchanges accept
honest input and refuse every single tampered field, a wallet it makes signs through the restated signing path and verifies under
OpenSSL, and the record tests/golden/lindell_keygen.json is what the restatement computes."""
import json

import numpy as np
import pytest

import enc_profiles as EP
import fixtures as F
import orc
import ossl
import pyref
import pyref_lindell as L

Q = pyref.Q


def _flip(v, bit=0):
    if isinstance(v, tuple):
        return (v[0] ^ (1 << bit), v[1])
    return v ^ (1 << bit)


@pytest.fixture(scope="module")
def wallet(keys):
    m = dict(p=[keys[0].p, keys[2].p], q=[keys[0].q, keys[2].q], pt=[keys[1].p, keys[3].p], qt=[keys[1].q, keys[3].q])
    r = F.Rng("lindell-cpu-wallet")
    m["h1"] = [r.below((a - 1) * (b - 1)) for a, b in zip(m["pt"], m["qt"])]
    m["xhi"] = [r.bits(256) for _ in range(2)]
    return L.keygen(b"lindell-cpu-wallet".ljust(32, b"."), 1, 2, material=m)


@pytest.mark.parametrize("profile", ["default", "all-alt"])
def test_first_messages_agree_with_the_oracle(profile):
    r = F.Rng("lindell-cpu-oracle")
    x = [1, Q - 1, Q + 5] + [r.below(Q) for _ in range(3)]
    nonce = [r.below(Q - 1) + 1 for _ in x]
    blind = [0, r.bits(248), r.bits(256), r.bits(256), r.bits(100), r.bits(256)]
    blind2 = [r.bits(256), 0, r.bits(240), r.bits(256), r.bits(256), r.bits(8)]
    with EP.applied(EP.PROFILES[profile]):
        msgs = [L.keygen_first_msg(x[i], nonce[i], blind[i], blind2[i]) for i in range(len(x))]
        pk, R, z = orc.dlog_prove(F.words([v % Q for v in x], 8), F.words(nonce, 8))
        assert F.points(pk) == [m["Q1"] for m in msgs] and F.points(R) == [m["R"] for m in msgs] and F.ints(z) == [m["z"] for m in msgs]
        for pts, bl, f in ((pk, blind, "pk_com"), (R, blind2, "pok_com")):
            com = np.zeros((len(x), 8), dtype=np.uint32)
            orc.lib.orc_hash_commit_point(len(x), orc._p(pts), orc._p(F.words(bl, 8)), orc._p(com))
            assert F.ints(com) == [m[f] for m in msgs]
        for i, m in enumerate(msgs):
            assert L.keygen_verify_first_msg(m["pk_com"], m["pok_com"], blind[i], blind2[i], m["Q1"], m["R"], m["z"])


def test_paillier_half_agrees_with_the_oracle(wallet, keys):
    h = wallet["half"]
    Nw = F.words(h["N"], 64)
    c = orc.paillier_encrypt(Nw, F.words(wallet["x1"], 64), F.words(h["r"], 64), [0, 1])
    assert F.ints(c) == h["c_key"]
    seed, sid = b"lindell-cpu-wallet".ljust(32, b"."), lambda f: 1 | (f << 56)
    B = 2
    al = orc.sample_below(B, seed, sid(L.F_PDL_ALPHA), F.words([Q ** 3], 24), 24)[0]
    be = orc.sample_below(B, seed, sid(L.F_PDL_BETA), F.words([n - 2 for n in h["N"]], 64), 64, None, orc.SAMPLE_PLUS_ONE)[0]
    rh = orc.sample_below(B, seed, sid(L.F_PDL_RHO), F.words([Q * n for n in h["Nt"]], 72), 72)[0]
    ga = orc.sample_below(B, seed, sid(L.F_PDL_GAMMA), F.words([Q ** 3 * n for n in h["Nt"]], 88), 88)[0]
    want = orc.pdl_prove(Nw, F.words(h["Nt"], 64), F.words(h["h1"], 64), F.words(h["h2"], 64), [0, 1], [0, 1], c, F.point_words(h["Q"]),
                         F.point_words([pyref.G] * B), F.words(wallet["x1"], 8), F.words(h["r"], 64), al, be, rh, ga)
    for f, w in (("z", 64), ("u2", 128), ("u3", 64), ("s1", 25), ("s2", 64), ("s3", 89)):
        assert F.ints(want[f]) == [p[f] for p in h["pdl"]], f
    assert F.points(want["u1"]) == [p["u1"] for p in h["pdl"]]
    assert wallet["ok"] == [1, 1] and wallet["failures"] == 0
    for i in range(B):                                        # h2 h1^xhi = 1 (mod N~): the statement CompositeDLogProof::prove(.., xhi) proves
        assert h["h2"][i] * pow(h["h1"][i], h["xhi"][i], h["Nt"][i]) % h["Nt"][i] == 1


def test_long_term_exchange_refuses_every_tampered_field():
    r = F.Rng("lindell-cpu-tamper")
    x, nonce, b1, b2 = r.below(Q), r.below(Q), r.bits(256), r.bits(256)
    m = L.keygen_first_msg(x, nonce, b1, b2)
    args = dict(pk_com=m["pk_com"], pok_com=m["pok_com"], blind_pk=b1, blind_pok=b2, Q1=m["Q1"], Rp=m["R"], z=m["z"])
    assert L.keygen_verify_first_msg(**args)
    for f in args:
        assert not L.keygen_verify_first_msg(**dict(args, **{f: _flip(args[f])})), f
    other = pyref.ec_mul(7, pyref.G)                          # a valid point that is not the committed one
    assert not L.keygen_verify_first_msg(**dict(args, Q1=other)) and not L.keygen_verify_first_msg(**dict(args, Rp=other))
    assert not L.keygen_verify_first_msg(**dict(args, Q1=None)) and not L.keygen_verify_first_msg(**dict(args, Rp=None))


@pytest.mark.parametrize("profile", ["default", "compressed"])
def test_ephemeral_exchange_refuses_every_tampered_field(profile):
    r = F.Rng("lindell-cpu-eph")
    with EP.applied(EP.PROFILES[profile]):
        k2, nonce, b1, b2 = r.below(Q), r.below(Q), r.bits(256), r.bits(256)
        m = L.eph_first_msg(k2, nonce, b1, b2)
        a1o, a2o, zo = np.zeros((1, 16), np.uint32), np.zeros((1, 16), np.uint32), np.zeros((1, 8), np.uint32)
        orc.lib.orc_ecddh_prove(1, *[orc._p(a) for a in (F.words([k2], 8), F.words([nonce], 8), F.point_words([pyref.G]), F.point_words([m["pub"]]),
                                                         F.point_words([pyref.H2]), F.point_words([m["c"]]), a1o, a2o, zo)])
        assert (F.points(a1o)[0], F.points(a2o)[0], F.ints(zo)[0]) == (m["a1"], m["a2"], m["z"])
        args = dict(pk_com=m["pk_com"], pok_com=m["pok_com"], blind_pk=b1, blind_pok=b2, pub=m["pub"], c=m["c"], a1=m["a1"], a2=m["a2"], z=m["z"])
        assert L.eph_verify_first_msg(**args)
        for f in args:
            assert not L.eph_verify_first_msg(**dict(args, **{f: _flip(args[f])})), f
        other = pyref.ec_mul(9, pyref.G)
        for f in ("pub", "c", "a1", "a2"):
            assert not L.eph_verify_first_msg(**dict(args, **{f: other})), f
            assert not L.eph_verify_first_msg(**dict(args, **{f: None})), f
        # a digest with a leading zero byte is committed to by its minimal bytes
        d = L.points_digest(m["a1"], m["a2"])
        assert L.commit_bigint(d, b2) == pyref.hash_bigints([d, b2])
        assert L.commit_bigint(1, 0) == int.from_bytes(ossl.sha256(pyref.to_bytes(1) + pyref.to_bytes(0)), "big")


def test_verify_rule():
    r = F.Rng("lindell-cpu-verify")
    d, k, m = r.below(Q - 1) + 1, r.below(Q - 1) + 1, r.bits(256)
    pub, Rp = pyref.ec_mul(d, pyref.G), pyref.ec_mul(k, pyref.G)
    rr = Rp[0] % Q
    s = pow(k, -1, Q) * (m + rr * d) % Q
    s = min(s, Q - s)
    assert L.verify(pub, m, rr, s) and pyref.ecdsa_verify(pub, m % Q, rr, s)
    assert not L.verify(pub, m, rr, Q - s) and pyref.ecdsa_verify(pub, m % Q, rr, Q - s)      # high s: refused here, valid ECDSA
    assert L.verify(pub, m % Q, rr, s) and L.verify(pub, m % Q + Q, rr, s)                    # the message is reduced
    for bad in (dict(r=rr ^ 1), dict(msg=m ^ 1), dict(s=0), dict(s=Q), dict(r=0), dict(pub=None), dict(pub=(pub[0], pub[1] ^ 1))):
        a = dict(pub=pub, msg=m, r=rr, s=s)
        a.update(bad)
        assert not L.verify(**a), bad


def test_wallet_signs_and_openssl_accepts(wallet, keys):
    B = 2
    eph = L.eph_exchange(b"lindell-cpu-eph-exchange".ljust(32, b"."), 2, B)
    assert eph["ok"] == [1] * B
    r = F.Rng("lindell-cpu-sign")
    for i in range(B):
        msg, rho, rnd = r.bits(256), r.below(Q * Q), r.below(wallet["N"][i])
        c3 = pyref.lindell_partial_sig(wallet["N"][i], wallet["c_key"][i], wallet["x2"][i], eph["k2"][i], eph["R1"][i], msg, rho, rnd)
        rr, s, _ = pyref.lindell_sign(wallet["p"][i], wallet["q"][i], c3, eph["k1"][i], eph["R2"][i])
        assert wallet["pubkey"][i] == pyref.ec_mul(wallet["x1"][i] * wallet["x2"][i], pyref.G)
        assert L.verify(wallet["pubkey"][i], msg, rr, s)
        assert ossl.ecdsa_verify(F.point_words([wallet["pubkey"][i]])[0], F.words([msg], 8), F.words([rr], 8), F.words([s], 8)).all()


def test_rotation_keeps_the_public_key(wallet):
    f = F.Rng("lindell-cpu-rotate").below(Q - 1) + 1
    h = wallet["half"]
    keys = F.load_keys()
    m = dict(p=[keys[4].p, keys[5].p], q=[keys[4].q, keys[5].q], pt=[keys[6].p, keys[7].p], qt=[keys[6].q, keys[7].q], h1=h["h1"], xhi=h["xhi"])
    w2 = L.rotate(wallet, [f, f], b"lindell-cpu-rotate".ljust(32, b"."), 4, factor2=[pow(f, -1, Q)] * 2, material=m)
    assert w2["ok"] == [1, 1] and w2["N"] != wallet["N"]
    for i in range(2):
        assert pyref.ec_mul(w2["x1"][i] * w2["x2"][i], pyref.G) == wallet["pubkey"][i]
        assert pyref.paillier_decrypt_textbook(w2["p"][i], w2["q"][i], w2["c_key"][i]) == w2["x1"][i]


def test_golden_record_is_what_the_restatement_computes():
    """tests/golden/lindell_keygen.json (tests/golden/make_lindell_keygen.py): the GPU tests compare the device's arrays with it"""
    import importlib.util
    import os
    path = os.path.join(F.HERE, "golden", "make_lindell_keygen.py")
    spec = importlib.util.spec_from_file_location("make_lindell_keygen", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    want = mk.build()
    if not os.path.exists(mk.PATH):
        mk.main()
    got = json.load(open(mk.PATH))
    assert got == json.loads(json.dumps(want))
    nt = got["ntilde"]
    assert nt["fail"] == 0
    for i in range(nt["count"]):
        Nt, h1, h2, xhi, phi = (int(nt[k][i], 16) for k in ("Nt", "h1", "h2", "xhi", "phi"))
        assert h2 * pow(h1, xhi, Nt) % Nt == 1 and h1 < phi and xhi < 1 << 256 and Nt.bit_length() in (2047, 2048)
    assert got["keygen"]["ok"] == [1] * got["keygen"]["B"] and got["keygen"]["failures"] == 0
