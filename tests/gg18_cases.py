"""GG18 signing cases shared by tests/test_gg18_cpu.py and tests/test_gg18_gpu.py: wallets (gg20_fixture.make_local_keys over
tests/golden/keys16.json), draws derived from SHA-256 of a tag, the tamper / hostile table, the reference runs of the Python
restatement (tests/pyref_gg18.py; computed once per process and shared, sessions spread over worker processes) and the packing of
its messages into the word layout of the batched calls (multi_party_ecdsa_amd.engine.GG18_MSG_FIELDS)."""
import hashlib
import os

import numpy as np

import fixtures as F
import gg20_fixture as G
import pyref as R
import pyref_gg18 as P18

Q = R.Q
SHAPES = {"t1n3": (1, 3, [0, 2]), "t2n5": (2, 5, [0, 2, 3, 4]), "t4n8": (4, 8, [0, 1, 2, 4, 6, 7]), "t1n3s3": (1, 3, [0, 1, 2])}

# field -> (round, kind, words); MessageB fields are [S][S-1][2]
MSG_FIELDS = dict(com=(1, "int", 8), c_a=(1, "int", 128), mb_c=(2, "int", 128), mb_b_pk=(2, "pt", 16), mb_b_R=(2, "pt", 16), mb_b_z=(2, "int", 8),
                  mb_bt_pk=(2, "pt", 16), mb_bt_R=(2, "pt", 16), mb_bt_z=(2, "int", 8), delta=(3, "int", 8), blind=(4, "int", 8), g_gamma=(4, "pt", 16),
                  com5a=(5, "int", 8), V=(6, "pt", 16), A=(6, "pt", 16), B=(6, "pt", 16), blind5a=(6, "int", 8), heg_T=(6, "pt", 16), heg_A3=(6, "pt", 16),
                  heg_z1=(6, "int", 8), heg_z2=(6, "int", 8), dlog_pk=(6, "pt", 16), dlog_R=(6, "pt", 16), dlog_z=(6, "int", 8), com5c=(7, "int", 8),
                  u=(8, "pt", 16), t=(8, "pt", 16), blind5c=(8, "int", 8), s_i=(9, "int", 8))
DRAW_WORDS = dict(k=8, gamma=8, blind=8, r_a=64, mb_beta_tag=64, mb_r=64, mb_nonce_b=8, mb_nonce_bt=8, l=8, rho=8, blind5a=8, heg_s1=8, heg_s2=8,
                  dlog_nonce=8, blind5c=8)

_keys16 = None


def wallet(shape):
    """(lk of gg20_fixture, the restatement's wallet dict of Python ints, signers)"""
    global _keys16
    if _keys16 is None:
        _keys16 = F.load_keys()
    t, n, signers = SHAPES[shape]
    lk = G.make_local_keys(_keys16, t, n, signers, seed="gg18-" + shape)
    a = lk["arrays"]
    w = dict(n=n, x=F.ints(a["x"]), p=F.ints(a["p"]), q=F.ints(a["q"]), X=F.points(a["X"]), y=F.points(a["y"])[0])
    w["N"] = [p_ * q_ for p_, q_ in zip(w["p"], w["q"])]
    return lk, w, list(signers)


def _h(tag, bits):
    out, c = b"", 0
    while len(out) * 8 < bits:
        out += hashlib.sha256(b"gg18|%s|%d" % (tag.encode(), c)).digest()
        c += 1
    return int.from_bytes(out, "big") >> (len(out) * 8 - bits)


def session_draws(w, signers, tag):
    """every value one session draws, per signer ordinal, from SHA-256 of the tag (pyref_gg18.sign_session's layout)"""
    S = len(signers)
    sc = lambda *a: _h("|".join(str(x) for x in (tag,) + a), 320) % (Q - 1) + 1
    below = lambda N, *a: _h("|".join(str(x) for x in (tag,) + a), 2304) % N
    d = {f: [] for f in P18.DRAW_FIELDS}
    for i in range(S):
        for f in ("k", "gamma", "l", "rho", "heg_s1", "heg_s2", "dlog_nonce"):
            d[f].append(sc(f, i))
        for f in ("blind", "blind5a", "blind5c"):
            d[f].append(_h("%s|%s|%d" % (tag, f, i), 256))
        d["r_a"].append(below(w["N"][signers[i]], "r_a", i))
        peerN = [w["N"][signers[P18.ind_of(i, jj)]] for jj in range(S - 1)]
        d["mb_beta_tag"].append([[below(peerN[jj], "bt", i, jj, v) for v in range(2)] for jj in range(S - 1)])
        d["mb_r"].append([[below(peerN[jj], "r", i, jj, v) for v in range(2)] for jj in range(S - 1)])
        d["mb_nonce_b"].append([[sc("nb", i, jj, v) for v in range(2)] for jj in range(S - 1)])
        d["mb_nonce_bt"].append([[sc("nbt", i, jj, v) for v in range(2)] for jj in range(S - 1)])
    return d


def session_msg(tag):
    return int.from_bytes(hashlib.sha256(b"gg18 message|" + tag.encode()).digest(), "big")


# ---- the tamper and hostile table: (name, status the row is about, round, edit(msgs, draws, env)) ------------------------------------
# env: dict(w, signers).  Every row attacks what signer ordinal 1 sends (ordinal 0 for the rows that say so), so every other signer sees it.
def _off_curve(env):
    x, y = R.ec_mul(31337, R.G)
    return (x, (y + 1) % R.P)


def _set(field, j, value):
    def edit(m, d, env):
        m[field][j] = value(m, d, env) if callable(value) else value
    return edit


def _mb(j, slot, v, fn):
    def edit(m, d, env):
        m["mb"][j][slot][v] = fn(dict(m["mb"][j][slot][v]), m, d, env)
    return edit


def _other_scalar(mb, m, d, env):
    """the w side answered with another scalar: a well-formed MessageB, so 201 passes and the pk differs from the sender's g_w"""
    w, sg = env["w"], env["signers"]
    return P18.message_b(0x1234567, w["N"][sg[0]], m["c_a"][0], 0xabcdef, 0x13579b, 0x2468, 0x369c)[0]


def _zero_sum(m, d, env):
    return (-sum(m["delta"][1:])) % Q


def _cancel_gamma(m, d, env):
    """signer 1 decommits to minus the others' sum: its peers see 401, the sender itself (which checks the peers only) a neutral R"""
    acc = None
    for j, p in enumerate(m["g_gamma"]):
        if j != 1:
            acc = R.ec_add(acc, p)
    return R.ec_neg(acc)


def _dbl_l(m, d, env):
    d["l"][1] = 2 * d["l"][1] % Q


def _k_zero(m, d, env):
    d["k"][0] = 0


ROWS = [
    ("bad k_i", 91, 0, _k_zero),
    ("c_b corrupted", 201, 2, _mb(1, 0, 0, lambda mb, m, d, e: dict(mb, c=mb["c"] ^ 2))),
    ("beta_tag_proof.z + 1", 201, 2, _mb(1, 0, 1, lambda mb, m, d, e: dict(mb, beta_tag_proof=mb["beta_tag_proof"][:2] + ((mb["beta_tag_proof"][2] + 1) % Q,)))),
    ("w side with another scalar", 202, 2, _mb(1, 0, 1, _other_scalar)),
    ("deltas sum to zero", 301, 3, _set("delta", 0, _zero_sum)),
    ("wrong blind factor", 401, 4, _set("blind", 1, lambda m, d, e: m["blind"][1] ^ 1)),
    ("g_gamma replaced", 401, 4, _set("g_gamma", 1, R.ec_mul(777, R.G))),
    ("g_gamma sum is neutral", 402, 4, _set("g_gamma", 1, _cancel_gamma)),
    ("V_i replaced", 531, 6, _set("V", 1, R.ec_mul(999, R.G))),
    ("ElGamal z1 + 1", 531, 6, _set("heg", 1, lambda m, d, e: dict(m["heg"][1], z1=(m["heg"][1]["z1"] + 1) % Q))),
    ("DLog z + 1", 531, 6, _set("dlog", 1, lambda m, d, e: m["dlog"][1][:2] + ((m["dlog"][1][2] + 1) % Q,))),
    ("u_i replaced", 541, 8, _set("u", 1, R.ec_mul(555, R.G))),
    ("l_i doubled after 5A", 542, 6, _dbl_l),
    ("s_i doubled", 601, 9, _set("s_i", 1, lambda m, d, e: 2 * m["s_i"][1] % Q)),
]
for _f, _rnd, _code in (("g_gamma", 4, 401), ("V", 6, 531), ("A", 6, 531), ("B", 6, 531), ("u", 8, 541), ("t", 8, 541)):
    ROWS.append(("%s off the curve" % _f, _code, _rnd, _set(_f, 1, lambda m, d, e: _off_curve(e))))
    ROWS.append(("%s all zero" % _f, _code, _rnd, _set(_f, 1, None)))
ROWS.append(("b_proof.pk off the curve", 201, 2, _mb(1, 0, 0, lambda mb, m, d, e: dict(mb, b_proof=(_off_curve(e),) + mb["b_proof"][1:]))))
ROWS.append(("b_proof.pk all zero", 201, 2, _mb(1, 0, 1, lambda mb, m, d, e: dict(mb, b_proof=(None,) + mb["b_proof"][1:]))))
CLEAN_EVERY = 4                                     # a clean session after every fourth row


def matrix_plan():
    """session k -> row index or None (clean)"""
    plan = []
    for r in range(len(ROWS)):
        plan.append(r)
        if r % CLEAN_EVERY == CLEAN_EVERY - 1:
            plan.append(None)
    plan.append(None)
    return plan


def row_tamper(row, env):
    """the restatement's tamper hook of one session carrying ROWS[row] (None: no tamper)"""
    if row is None:
        return None
    _, _, rnd, edit = ROWS[row]

    def tamper(r, msgs, draws):
        if r == rnd:
            edit(msgs, draws, env)
    return tamper


# ---- reference runs, once per process ---------------------------------------------------------------------------------------------
def _run_session(job):
    shape, tag, row, enc = job
    _, w, signers = wallet(shape)
    draws = session_draws(w, signers, tag)
    env = dict(w=w, signers=signers)
    if row is not None and ROWS[row][2] == 0:
        ROWS[row][3](None, draws, env)
    import copy
    given = copy.deepcopy(draws)                   # what the session starts with: a later row edits `draws` while it runs
    with R.use_encoding(R.Encoding(**enc)):
        out = P18.sign_session(w, signers, session_msg(tag), draws, tamper=row_tamper(row, env) if row is not None and ROWS[row][2] else None)
    out["draws"], out["msg"] = given, session_msg(tag)
    return out


_cache = {}


def reference(jobs):
    """jobs: list of (shape, tag, row or None, encoding dict) -> list of sign_session results (+ draws, msg).  Sessions are independent
    and a Python modular exponentiation at Paillier size takes 0.1 s, so the missing ones run in worker processes (fresh interpreters
    that import only the restatement)."""
    keyed = [(s, t, r, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in e.items()))) for s, t, r, e in jobs]
    todo = [(j, k) for j, k in zip(jobs, keyed) if k not in _cache]
    if todo:
        workers = min(16, os.cpu_count() or 1, len(todo))
        res = None
        if workers > 1:
            try:
                import multiprocessing as mp
                from concurrent.futures import ProcessPoolExecutor
                with ProcessPoolExecutor(workers, mp_context=mp.get_context("spawn")) as ex:
                    res = list(ex.map(_run_session, [j for j, _ in todo]))
            except (OSError, RuntimeError, ImportError):
                res = None
        if res is None:
            res = [_run_session(j) for j, _ in todo]
        for (_, k), r in zip(todo, res):
            _cache[k] = r
    return [_cache[k] for k in keyed]


def jobs_for(shape, B, enc=None, prefix="s"):
    e = (enc or R.Encoding()).as_dict()
    return [(shape, "%s-%s-%d" % (prefix, shape, b), None, e) for b in range(B)]


def matrix_jobs(shape="t1n3s3"):
    e = R.Encoding().as_dict()
    return [(shape, "matrix-%d" % k, row, e) for k, row in enumerate(matrix_plan())]


# ---- packing into the word layout of the batched calls ----------------------------------------------------------------------------
def _pt_int(p):
    return 0 if p is None else p[0] | (p[1] << 256)


def _int_pt(v):
    x, y = v & ((1 << 256) - 1), v >> 256
    return None if x == 0 and y == 0 else (x, y)


def flat_session(m):
    """pyref_gg18 msgs (possibly only the first rounds) -> {field: nested lists of ints}, points as x | y << 256"""
    o = {}
    for f, (_, kind, _) in MSG_FIELDS.items():
        conv = _pt_int if kind == "pt" else int
        if f.startswith("mb_"):
            if "mb" not in m:
                continue
            part = f[3:]
            get = (lambda mb: mb["c"]) if part == "c" else (lambda mb, part=part: mb["b_proof" if part.startswith("b_") else "beta_tag_proof"][("pk", "R", "z").index(part.split("_")[1])])
            o[f] = [[[conv(get(mb)) for mb in pair] for pair in row] for row in m["mb"]]
        elif f.startswith("heg_"):
            if "heg" in m:
                o[f] = [conv(h[f[4:]]) for h in m["heg"]]
        elif f.startswith("dlog_"):
            if "dlog" in m:
                o[f] = [conv(d[("pk", "R", "z").index(f[5:])]) for d in m["dlog"]]
        elif f in m:
            o[f] = [conv(v) for v in m[f]]
    return o


def unflat_session(o):
    """the inverse of flat_session over the fields present"""
    m = {}
    S = len(o["com"])
    pt = lambda f, v: _int_pt(v) if MSG_FIELDS[f][1] == "pt" else v
    for f in o:
        if not (f.startswith("mb_") or f.startswith("heg_") or f.startswith("dlog_")):
            m[f] = [pt(f, v) for v in o[f]]
    if "mb_c" in o:
        m["mb"] = [[[dict(c=o["mb_c"][i][jj][v],
                          b_proof=(_int_pt(o["mb_b_pk"][i][jj][v]), _int_pt(o["mb_b_R"][i][jj][v]), o["mb_b_z"][i][jj][v]),
                          beta_tag_proof=(_int_pt(o["mb_bt_pk"][i][jj][v]), _int_pt(o["mb_bt_R"][i][jj][v]), o["mb_bt_z"][i][jj][v]))
                     for v in range(2)] for jj in range(S - 1)] for i in range(S)]
    if "heg_T" in o:
        m["heg"] = [dict(T=_int_pt(o["heg_T"][i]), A3=_int_pt(o["heg_A3"][i]), z1=o["heg_z1"][i], z2=o["heg_z2"][i]) for i in range(S)]
    if "dlog_pk" in o:
        m["dlog"] = [(_int_pt(o["dlog_pk"][i]), _int_pt(o["dlog_R"][i]), o["dlog_z"][i]) for i in range(S)]
    return m


def _words(v, w):
    return np.frombuffer(int(v).to_bytes(4 * w, "little"), dtype="<u4")


def pack_msgs(results):
    """reference results of B sessions -> {field: uint32 [S, B, w]} ([S, S-1, 2, B, w] for the MessageB fields)"""
    B, flats = len(results), [flat_session(r["msgs"]) for r in results]
    S = len(flats[0]["com"])
    out = {}
    for f, (_, _, w) in MSG_FIELDS.items():
        if f.startswith("mb_"):
            a = np.zeros((S, S - 1, 2, B, w), dtype=np.uint32)
            for b, fl in enumerate(flats):
                for i in range(S):
                    for jj in range(S - 1):
                        for v in range(2):
                            a[i, jj, v, b] = _words(fl[f][i][jj][v], w)
        else:
            a = np.zeros((S, B, w), dtype=np.uint32)
            for b, fl in enumerate(flats):
                for i in range(S):
                    a[i, b] = _words(fl[f][i], w)
        out[f] = a
    return out


def pack_draws(results, local=None):
    """the draws of B sessions -> {field: uint32 [L, B, w]} ([2, L, S-1, B, w] for the MessageB fields), the layout gg18_sign takes"""
    B = len(results)
    S = len(results[0]["draws"]["k"])
    local = list(range(S)) if local is None else list(local)
    L = len(local)
    out = {}
    for f, w in DRAW_WORDS.items():
        if f.startswith("mb_"):
            a = np.zeros((2, L, S - 1, B, w), dtype=np.uint32)
            for b, r in enumerate(results):
                for li, i in enumerate(local):
                    for jj in range(S - 1):
                        for v in range(2):
                            a[v, li, jj, b] = _words(r["draws"][f][i][jj][v], w)
        else:
            a = np.zeros((L, B, w), dtype=np.uint32)
            for b, r in enumerate(results):
                for li, i in enumerate(local):
                    a[li, b] = _words(r["draws"][f][i], w)
        out[f] = a
    return out


def pack_list(vals, w, kind="int"):
    """[S or L][B] nested Python values -> uint32 [len, B, w]"""
    a = np.zeros((len(vals), len(vals[0]), w), dtype=np.uint32)
    for i, row in enumerate(vals):
        for b, v in enumerate(row):
            a[i, b] = _words(_pt_int(v) if kind == "pt" else v, w)
    return a


def pack_sigs(results, i=0):
    """(r [B,8], s [B,8], recid [B]) of signer ordinal i; zero where that party has no signature"""
    B = len(results)
    r, s, rec = np.zeros((B, 8), dtype=np.uint32), np.zeros((B, 8), dtype=np.uint32), np.zeros(B, dtype=np.int32)
    for b, res in enumerate(results):
        if res["sig"][i] is not None:
            r[b], s[b], rec[b] = _words(res["sig"][i][0], 8), _words(res["sig"][i][1], 8), res["sig"][i][2]
    return r, s, rec


def device_hook(plan, env, rounds_done=None):
    """the `_fault` hook of engine.gg18_sign for a batch in which session k carries ROWS[plan[k]]: the messages of the rounds so far
    are read back (they are public), the row's edit runs on the restatement's form of session k, what it changed is written back."""
    import torch

    def hook(rnd, dmsgs):
        ks = [k for k, row in enumerate(plan) if row is not None and ROWS[row][2] == rnd]
        if not ks:
            return
        names = [f for f, (r_, _, _) in MSG_FIELDS.items() if r_ <= rnd]
        host = {f: dmsgs[f].cpu().numpy().view(np.uint32) for f in names}
        dl = dmsgs["draws"]["l"].cpu().numpy().view(np.uint32)                   # [L, B, 8]; the one draw a row edits after the start
        for k in ks:
            flat = {}
            for f in names:
                a = host[f]
                flat[f] = ([[[F.ints(a[i, jj, v, k:k + 1])[0] for v in range(2)] for jj in range(a.shape[1])] for i in range(a.shape[0])]
                           if f.startswith("mb_") else [F.ints(a[i, k:k + 1])[0] for i in range(a.shape[0])])
            m = unflat_session(flat)
            d = dict(l=[F.ints(dl[i, k:k + 1])[0] for i in range(dl.shape[0])])
            ROWS[plan[k]][3](m, d, env)
            new = flat_session(m)
            for f in names:
                if new[f] != flat[f]:
                    w = MSG_FIELDS[f][2]
                    if f.startswith("mb_"):
                        for i in range(len(new[f])):
                            for jj in range(len(new[f][i])):
                                for v in range(2):
                                    if new[f][i][jj][v] != flat[f][i][jj][v]:
                                        dmsgs[f][i, jj, v, k] = torch.from_numpy(_words(new[f][i][jj][v], w).astype(np.uint32).view(np.int32).copy()).to(dmsgs[f].device)
                    else:
                        for i in range(len(new[f])):
                            if new[f][i] != flat[f][i]:
                                dmsgs[f][i, k] = torch.from_numpy(_words(new[f][i], w).astype(np.uint32).view(np.int32).copy()).to(dmsgs[f].device)
            for i in range(dl.shape[0]):
                if d["l"][i] != F.ints(dl[i, k:k + 1])[0]:
                    dmsgs["draws"]["l"][i, k] = torch.from_numpy(_words(d["l"][i], 8).astype(np.uint32).view(np.int32).copy()).to(dmsgs["draws"]["l"].device)
    return hook
