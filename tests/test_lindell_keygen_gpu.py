"""GPU tests of Lindell'17 key generation on the device (mpe_lindell_keygen.h and the three chains of engine.py) against the
pure-Python restatement tests/pyref_lindell.py: first messages byte for byte, verdicts item by item under single-field tampering,
the N~ rule, the ECDSA check against the restatement and OpenSSL, whole key generation over fixed material, seed to signature with
material minted on the device, rotation, and workspace hygiene.  Per-lane kernels run B = 70: one full 64-lane workgroup and a
partial one."""
import json
import os

import numpy as np
import pytest
import torch

import enc_profiles as EP
import fixtures as F
import lindell_fixture as LF
import ossl
import pyref
import pyref_lindell as L

pytestmark = pytest.mark.gpu
Q, G, H2 = pyref.Q, pyref.G, pyref.H2
B70 = 70


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _np(t):
    return t.cpu().numpy().view(np.uint32)


def _seed(tag):
    return tag.encode().ljust(32, b".")


def _zero_digest_nonce(start):
    """the first nonce s >= start whose Sha256(chain_points([s G, s H])) begins with a zero byte (s G and s H stepped by one addition)"""
    a1, a2 = pyref.ec_mul(start, G), pyref.ec_mul(start, H2)
    for j in range(4096):
        if L.points_digest(a1, a2) >> 248 == 0:
            return start + j
        a1, a2 = pyref.ec_add(a1, G), pyref.ec_add(a2, H2)
    raise AssertionError("no nonce with a zero leading digest byte in 4096 tries")


_cases = {}


def first_msg_case(profile):
    """the batch of tests 1 and 2 with the restatement's messages, computed once per profile"""
    if profile in _cases:
        return _cases[profile]
    r = F.Rng("gpu-lindell-keygen-first")
    x = [1, Q - 1, Q + 5] + [r.below(Q - 1) + 1 for _ in range(B70 - 3)]
    nonce = [r.below(Q - 1) + 1 for _ in range(B70)]
    bpk = [r.bits(256) for _ in range(B70)]
    bpok = [r.bits(256) for _ in range(B70)]
    bpk[3], bpk[4], bpok[5], bpok[6] = 0, r.bits(248), 0, r.bits(240)            # minimal bytes: zero, and a zero top byte
    with EP.applied(EP.PROFILES[profile]):
        enonce = list(nonce)
        enonce[7] = _zero_digest_nonce(nonce[7])
        kg = [L.keygen_first_msg(x[i], nonce[i], bpk[i], bpok[i]) for i in range(B70)]
        eph = [L.eph_first_msg(x[i], enonce[i], bpk[i], bpok[i]) for i in range(B70)]
        assert L.points_digest(eph[7]["a1"], eph[7]["a2"]) >> 248 == 0
    assert x[0] == 1 and x[1] == Q - 1 and x[2] > Q and bpk[3] == 0 and bpok[5] == 0 and 0 < bpk[4] < 1 << 248 and 0 < bpok[6] < 1 << 248
    _cases[profile] = dict(x=x, nonce=nonce, enonce=enonce, bpk=bpk, bpok=bpok, kg=kg, eph=eph)
    return _cases[profile]


def _ctx_for(gpu_ctx, profile):
    from multi_party_ecdsa_amd import engine as E
    return gpu_ctx if profile == "default" else E.Context(0, encoding=EP.PROFILES[profile].as_dict())


# ---- 1. first messages, byte for byte ------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["default", "all-alt"])
def test_first_messages_match_the_restatement(gpu_ctx, profile):
    from multi_party_ecdsa_amd import engine as E
    c = first_msg_case(profile)
    ctx = _ctx_for(gpu_ctx, profile)
    d = lambda vals, w=8: _dev(ctx, F.words(vals, w))
    m = E.lindell_keygen_first_msg(ctx, d(c["x"]), d(c["nonce"]), d(c["bpk"]), d(c["bpok"]))
    e = E.lindell_eph_first_msg(ctx, d(c["x"]), d(c["enonce"]), d(c["bpk"]), d(c["bpok"]))
    with EP.applied(EP.PROFILES[profile]):
        dg = [L.points_digest(v["a1"], v["a2"]) for v in c["eph"]]
        want_com = [L.commit_bigint(a, b) for a, b in zip(dg, c["bpok"])]
    com = E.hash_commit_bigint(ctx, d(dg), d(c["bpok"]))
    ctx.sync()
    for f in ("Q1", "R"):
        assert np.array_equal(_np(m[f]), F.point_words([v[f] for v in c["kg"]])), f
    for f in ("z", "pk_com", "pok_com"):
        assert np.array_equal(_np(m[f]), F.words([v[f] for v in c["kg"]], 8)), f
    for f in ("pub", "c", "a1", "a2"):
        assert np.array_equal(_np(e[f]), F.point_words([v[f] for v in c["eph"]])), f
    for f in ("z", "pk_com", "pok_com"):
        assert np.array_equal(_np(e[f]), F.words([v[f] for v in c["eph"]], 8)), f
    assert dg[7] >> 248 == 0
    assert np.array_equal(_np(com), F.words(want_com, 8)) and want_com == [v["pok_com"] for v in c["eph"]]
    # the ECDDH triple is what mpe_ecddh_prove gives for the statement (G, pub, H, c)
    st = dict(g1=_dev(ctx, F.point_words([G] * B70)), h1=e["pub"], g2=_dev(ctx, F.point_words([H2] * B70)), h2=e["c"])
    pr = E.ecddh_prove(ctx, d(c["x"]), d(c["enonce"]), st)
    ctx.sync()
    for f in ("a1", "a2", "z"):
        assert np.array_equal(_np(pr[f]), _np(e[f])), f


# ---- 2. verdicts ------------------------------------------------------------------------------------------------------------
OFF_CURVE = (G[0], G[1] ^ 1)


def _tampered(honest, widths, f, third):
    """copies of the honest columns with bit 0 of field f flipped in the items i % 3 == third; two items get an invalid point"""
    cols = {k: list(v) for k, v in honest.items()}
    for i in range(B70):
        if i % 3 == third:
            v = cols[f][i]
            cols[f][i] = (v[0] ^ 1, v[1]) if isinstance(v, tuple) else v ^ 1
    if widths[f] == 16:
        cols[f][10], cols[f][11] = OFF_CURVE, None
    return cols


def _verdicts(fn, cols, order, memo):
    """the restatement's verdict per item; items a run leaves untouched are computed once"""
    out = []
    for i in range(B70):
        key = tuple(cols[f][i] for f in order)
        if key not in memo:
            memo[key] = int(fn(**dict(zip(order, key))))
        out.append(memo[key])
    return out


def _words_of(cols, widths):
    return {k: (F.point_words(v) if widths[k] == 16 else F.words(v, 8)) for k, v in cols.items()}


def test_long_term_verdicts(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    c = first_msg_case("default")
    order = ("pk_com", "pok_com", "blind_pk", "blind_pok", "Q1", "Rp", "z")
    widths = dict(pk_com=8, pok_com=8, blind_pk=8, blind_pok=8, Q1=16, Rp=16, z=8)
    honest = dict(pk_com=[m["pk_com"] for m in c["kg"]], pok_com=[m["pok_com"] for m in c["kg"]], blind_pk=c["bpk"], blind_pok=c["bpok"],
                  Q1=[m["Q1"] for m in c["kg"]], Rp=[m["R"] for m in c["kg"]], z=[m["z"] for m in c["kg"]])
    runs = [("honest", honest)] + [(f, _tampered(honest, widths, f, k % 3)) for k, f in enumerate(order)]
    memo = {}
    for name, cols in runs:
        w = _words_of(cols, widths)
        ok = E.lindell_keygen_verify_first_msg(gpu_ctx, *[_dev(gpu_ctx, w[f]) for f in order])
        gpu_ctx.sync()
        want = _verdicts(L.keygen_verify_first_msg, cols, order, memo)
        assert list(ok.cpu().numpy()) == want, name
        if name == "honest":
            assert want == [1] * B70
        else:
            assert 0 < sum(want) < B70, name


def test_ephemeral_verdicts(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    c = first_msg_case("default")
    order = ("pk_com", "pok_com", "blind_pk", "blind_pok", "pub", "c", "a1", "a2", "z")
    widths = dict(pk_com=8, pok_com=8, blind_pk=8, blind_pok=8, pub=16, c=16, a1=16, a2=16, z=8)
    honest = {f: [m[f] for m in c["eph"]] for f in ("pk_com", "pok_com", "pub", "c", "a1", "a2", "z")}
    honest.update(blind_pk=c["bpk"], blind_pok=c["bpok"])
    runs = [("honest", honest)] + [(f, _tampered(honest, widths, f, k % 3)) for k, f in enumerate(order)]
    memo = {}
    for name, cols in runs:
        w = _words_of(cols, widths)
        ok = E.lindell_eph_verify_first_msg(gpu_ctx, *[_dev(gpu_ctx, w[f]) for f in order])
        gpu_ctx.sync()
        want = _verdicts(L.eph_verify_first_msg, cols, order, memo)
        assert list(ok.cpu().numpy()) == want, name
        if name == "honest":
            assert want == [1] * B70
        else:
            assert 0 < sum(want) < B70, name


# ---- 3. mpe_lindell_ntilde_generate ------------------------------------------------------------------------------------------
def _golden():
    with open(os.path.join(F.HERE, "golden", "lindell_keygen.json")) as fh:
        return json.load(fh)


def test_ntilde_generate_matches_the_replay(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    g = _golden()["ntilde"]
    n = g["count"]
    assert n == 5
    o = E.lindell_ntilde_generate(gpu_ctx, n, bytes.fromhex(g["seed"]), g["counter"])
    r = E.sample_bits(gpu_ctx, n, _seed("gpu-lindell-cdlog"), 1, 512, 16)
    xw = torch.zeros((n, 64), dtype=torch.int32, device=gpu_ctx.device)
    xw[:, :8] = o["xhi"]
    x, y = E.composite_dlog_prove(gpu_ctx, o["Nt"], o["h1"], o["h2"], xw, r)
    ok = E.composite_dlog_verify(gpu_ctx, o["Nt"], o["h1"], o["h2"], x, y)
    gpu_ctx.sync()
    want = {k: [int(v, 16) for v in g[k]] for k in ("Nt", "h1", "h2", "xhi", "phi")}
    for k, w in (("Nt", 64), ("h1", 64), ("h2", 64), ("xhi", 8)):
        assert F.ints(_np(o[k])) == want[k], k
    for i in range(n):
        assert want["h2"][i] * pow(want["h1"][i], want["xhi"][i], want["Nt"][i]) % want["Nt"][i] == 1 and want["h1"][i] < want["phi"][i]
    assert int(o["fail"].item()) == 0 == g["fail"]
    assert list(ok.cpu().numpy()) == [1] * n


# ---- 4. mpe_ecdsa_verify -----------------------------------------------------------------------------------------------------
def test_ecdsa_verify_against_restatement_and_openssl(gpu_ctx, keys):
    from multi_party_ecdsa_amd import engine as E
    nsig = 7
    fx = LF.make(keys, nsig, seed="gpu-lindell-verify")
    _, wr, ws, _ = LF.oracle_run(fx)
    rs, ss, msgs, pubs = F.ints(wr), F.ints(ws), fx["msg_int"], fx["pub"]
    assert msgs[3] == Q + 5
    other = pyref.ec_mul(12345, G)
    items = []                                                # (tag, pub, msg, r, s)
    for i in range(nsig):
        a = (pubs[i], msgs[i], rs[i], ss[i])
        items += [("valid",) + a, ("high-s", a[0], a[1], a[2], Q - a[3]), ("r^1", a[0], a[1], a[2] ^ 1, a[3]), ("msg^1", a[0], a[1] ^ 1, a[2], a[3]),
                  ("s=0", a[0], a[1], a[2], 0), ("s=q", a[0], a[1], a[2], Q), ("r=0", a[0], a[1], 0, a[3]),
                  ("off-curve", (a[0][0], a[0][1] ^ 1), a[1], a[2], a[3]), ("infinity", None, a[1], a[2], a[3])]
    items.append(("reduced-twin", pubs[3], msgs[3] - Q, rs[3], ss[3]))               # msg >= q and its reduced twin are both valid
    items += [("wrong-key", other, msgs[i], rs[i], ss[i]) for i in range(6)]
    assert len(items) == B70
    pw = F.point_words([it[1] for it in items])
    mw, rw, sw = (F.words([it[k] for it in items], 8) for k in (2, 3, 4))
    ok = E.ecdsa_verify(gpu_ctx, _dev(gpu_ctx, pw), _dev(gpu_ctx, mw), _dev(gpu_ctx, rw), _dev(gpu_ctx, sw))
    gpu_ctx.sync()
    got = list(ok.cpu().numpy())
    want = [int(L.verify(*it[1:])) for it in items]
    assert got == want
    op = list(ossl.ecdsa_verify(pw, mw, rw, sw).astype(int))
    for i, it in enumerate(items):
        if it[0] == "high-s":
            assert got[i] == 0 and op[i] == 1, i             # refused by party_one::verify although it is a valid ECDSA signature
        else:
            assert got[i] == op[i], (i, it[0])
        assert got[i] == (1 if it[0] in ("valid", "reduced-twin") else 0), (i, it[0])


# ---- 5. whole keygen over fixed material -----------------------------------------------------------------------------------------
def test_keygen_fixed_material_matches_the_restatement(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    g = _golden()["keygen"]
    B = g["B"]
    assert B == 4
    ints = lambda k: [int(v, 16) for v in g["material"][k]]
    material = dict(p=F.words(ints("p"), 32), q=F.words(ints("q"), 32), pt=F.words(ints("pt"), 32), qt=F.words(ints("qt"), 32),
                    h1=F.words(ints("h1"), 64), xhi=F.words(ints("xhi"), 8))
    w = E.lindell_keygen(gpu_ctx, B, bytes.fromhex(g["seed"]), g["counter"], material=material)
    assert list(w["ok"].cpu().numpy()) == [1] * B == g["ok"] and w["failures"] == 0 == g["failures"]
    for k, words in (("x1", 8), ("x2", 8), ("p", 32), ("q", 32), ("N", 64), ("c_key", 128), ("r", 64)):
        assert F.ints(_np(w[k])) == [int(v, 16) for v in g[k]], k
    for k in ("Q1", "Q2", "pubkey"):
        assert F.points(_np(w[k])) == [(int(x, 16), int(y, 16)) for x, y in g[k]], k
    x1, x2 = F.ints(_np(w["x1"])), F.ints(_np(w["x2"]))
    assert F.points(_np(w["pubkey"])) == [pyref.ec_mul(a * b, G) for a, b in zip(x1, x2)]
    assert np.array_equal(_np(E.ec_mul(gpu_ctx, w["x2"], w["Q1"])), _np(w["pubkey"]))        # party two's compute_pubkey


# ---- 6..8. seed to signature, rotation, hygiene -----------------------------------------------------------------------------------
MINT_SEED = _seed("gpu-lindell-mint")


def _sign(ctx, wallet, seed, counter):
    """lindell_eph_exchange -> lindell_partial_sig -> lindell_sign with every draw from the device sampler: (ok, msg, r, s)"""
    from multi_party_ecdsa_amd import engine as E
    B = wallet["x1"].shape[0]
    eph = E.lindell_eph_exchange(ctx, B, seed, counter)
    sid = lambda f: counter | (f << 56)
    msg = E.sample_bits(ctx, B, seed, sid(40), 256, 8)
    rho, _ = E.sample_below(ctx, B, seed, sid(41), E.dev(ctx, [Q * Q], 16), 16)
    rnd, _ = E.sample_below(ctx, B, seed, sid(42), wallet["N"], 64)
    ctx.sync()
    pk = E.PaillierKeys(ctx, N=E.host(wallet["N"]))
    sk = E.PaillierKeys(ctx, p=wallet["p"], q=wallet["q"])
    c3 = E.lindell_partial_sig(ctx, pk, wallet["c_key"], wallet["x2"], eph["k2"], eph["R1"], msg, rho, rnd)
    r, s, _ = E.lindell_sign(ctx, sk, c3, eph["k1"], eph["R2"])
    ctx.sync()
    pk.close(); sk.close()
    return eph["ok"], msg, r, s


@pytest.fixture(scope="module")
def minted(gpu_ctx):
    from multi_party_ecdsa_amd import engine as E
    return E.lindell_keygen(gpu_ctx, 3, MINT_SEED, 1)


def _same(a, b, fields=("x1", "x2", "Q1", "Q2", "pubkey", "p", "q", "N", "c_key", "r")):
    return [bool(np.array_equal(_np(a[f]), _np(b[f]))) for f in fields]


def test_seed_to_signature(gpu_ctx, minted):
    from multi_party_ecdsa_amd import engine as E
    B = 3
    w = minted
    assert list(w["ok"].cpu().numpy()) == [1] * B and w["failures"] == 0
    ok, msg, r, s = _sign(gpu_ctx, w, MINT_SEED, 2)
    assert list(ok.cpu().numpy()) == [1] * B
    assert list(E.ecdsa_verify(gpu_ctx, w["pubkey"], msg, r, s).cpu().numpy()) == [1] * B
    assert ossl.ecdsa_verify(_np(w["pubkey"]), _np(msg), _np(r), _np(s)).all()
    assert list(E.is_probable_prime(gpu_ctx, w["p"]).cpu().numpy()) == [1] * B and list(E.is_probable_prime(gpu_ctx, w["q"]).cpu().numpy()) == [1] * B
    assert all(n.bit_length() in (2047, 2048) for n in F.ints(_np(w["N"])))
    assert all(_same(w, E.lindell_keygen(gpu_ctx, B, MINT_SEED, 1)))                       # the chain is a function of (seed, counter)
    assert not any(_same(w, E.lindell_keygen(gpu_ctx, B, MINT_SEED, 3)))


def test_rotation(gpu_ctx, minted):
    from multi_party_ecdsa_amd import engine as E
    B = 3
    fr = F.Rng("gpu-lindell-rotate")
    f = [fr.below(Q - 1) + 1 for _ in range(B)]
    d = lambda vals: _dev(gpu_ctx, F.words(vals, 8))
    w2 = E.lindell_rotate(gpu_ctx, minted, d(f), MINT_SEED, 5, d_factor2=d([pow(v, -1, Q) for v in f]))
    assert list(w2["ok"].cpu().numpy()) == [1] * B and w2["failures"] == 0                 # the new correct-key and pdl_verify verdicts
    assert not any(_same(minted, w2, ("N",))) and all(a != b for a, b in zip(F.ints(_np(minted["N"])), F.ints(_np(w2["N"]))))
    ok, msg, r, s = _sign(gpu_ctx, w2, MINT_SEED, 6)
    assert list(ok.cpu().numpy()) == [1] * B
    assert list(E.ecdsa_verify(gpu_ctx, minted["pubkey"], msg, r, s).cpu().numpy()) == [1] * B        # the OLD public key
    assert ossl.ecdsa_verify(_np(minted["pubkey"]), _np(msg), _np(r), _np(s)).all()
    w3 = E.lindell_rotate(gpu_ctx, minted, d(f), MINT_SEED, 7, d_factor2=d(f))             # f on both sides: the key becomes f^2 pubkey
    assert list(w3["ok"].cpu().numpy()) == [1] * B
    ok, msg, r, s = _sign(gpu_ctx, w3, MINT_SEED, 8)
    f2pub = E.ec_mul(gpu_ctx, d([v * v % Q for v in f]), minted["pubkey"])
    assert list(E.ecdsa_verify(gpu_ctx, f2pub, msg, r, s).cpu().numpy()) == [1] * B
    assert list(E.ecdsa_verify(gpu_ctx, minted["pubkey"], msg, r, s).cpu().numpy()) == [0] * B


def test_workspace_hygiene(gpu_ctx, minted):
    """the new calls keep their secrets (p~, q~, phi, the sampling rows of xhi) in the context workspace: the audit sees them, the wipe clears them"""
    from multi_party_ecdsa_amd import engine as E
    o = E.lindell_ntilde_generate(gpu_ctx, 2, MINT_SEED, 9)
    gpu_ctx.sync()
    assert int(o["fail"].item()) == 0
    assert gpu_ctx.scratch_audit()[0] > 0
    gpu_ctx.wipe()
    assert gpu_ctx.scratch_audit()[0] == 0
