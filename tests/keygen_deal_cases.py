"""Pure-Python restatement (over tests/pyref.py) of the dealing side of GG20 keygen and of its round-3 verdict, and the case tables the
CPU and GPU tests share (gg_2020/party_i.rs:260-438):
  vss_share            `VerifiableSS::share(t, n, &u_i)`
  construct_keypair    the OK branch of `phase2_verify_vss_construct_keypair_phase3_pok_dlog` (:355-363)
  xi_commitments       `Keys::get_commitments_to_xi` (:369-388)
  verify_round3        `Keys::verify_dlog_proofs_check_against_vss` (:405-438)
Points are (x, y) tuples, None = the neutral element (the all-zero row).  A tuple may be OFF the curve (a tampered row): the
restatement then follows the documented divergence of mpe_keygen_verify_round3 — such a commitment refuses its whole session.
Every expected value is exact.  Test infrastructure: nothing here is imported by the product."""
import functools

import fixtures as F
import pyref

Q, P, G = pyref.Q, pyref.P, pyref.G


def pt_valid(p):
    """ec::aff_valid: canonical coordinates, on the curve, not neutral (what curv's deserialisation lets through)"""
    return p is not None and p[0] < P and p[1] < P and (p[1] * p[1] - p[0] ** 3 - 7) % P == 0


def vss_share(coef, n):
    """coef[0] = the secret; -> (commitments [t + 1], shares [n]), shares[j] = f(j + 1) mod q"""
    coef = [c % Q for c in coef]
    shares = []
    for j in range(1, n + 1):
        acc = 0
        for c in reversed(coef):
            acc = (acc * j + c) % Q
        shares.append(acc)
    return [pyref.ec_mul(c, G) for c in coef], shares


def dlog_prove(x, nonce):
    """pyref.dlog_prove, and x = 0: pk is neutral and z = nonce - c 0 = nonce whatever the challenge hashes for the neutral row"""
    if x % Q == 0:
        return None, pyref.ec_mul(nonce, G), nonce % Q
    return pyref.dlog_prove(x % Q, nonce % Q)


def construct_keypair(shares, ys, nonce):
    x = sum(s % Q for s in shares) % Q
    ysum = None
    for y in ys:
        ysum = pyref.ec_add(ysum, y)
    return (x, ysum) + tuple(dlog_prove(x, nonce))


def xi_commitments(commits):
    """commits[j][k] of one session -> [sum_k (i + 1)^k sum_j commits[j][k] for i < n], through pyref.vss_point on the global polynomial;
    None for every party when a commitment is no valid point"""
    n, t1 = len(commits), len(commits[0])
    if not all(pt_valid(c) for row in commits for c in row):
        return None
    glob = []
    for k in range(t1):
        acc = None
        for j in range(n):
            acc = pyref.ec_add(acc, commits[j][k])
        glob.append(acc)
    return [pyref.vss_point(glob, i + 1) for i in range(n)]


def dlog_verify(pk, R, z):
    return pt_valid(pk) and pt_valid(R) and pyref.dlog_verify(pk, R, z % Q)


def verify_round3(commits, proofs):
    """one session: commits[j][k], proofs[i] = (pk, R, z) -> (ok [n], bad_actors mask, xi_commit [n] (None rows for a refused session))"""
    n = len(commits)
    xi = xi_commitments(commits)
    ok = [int(xi is not None and dlog_verify(*proofs[i]) and xi[i] == proofs[i][0]) for i in range(n)]
    return ok, sum((1 - o) << i for i, o in enumerate(ok)), (xi if xi is not None else [None] * n)


# ---- case tables ------------------------------------------------------------------------------------------------------------------
DEAL_SHAPES = [(0, 1), (1, 3), (2, 5)]
DEAL_BATCH = 67                      # one full wave and a ragged one
DEAL_ZERO_DEALER = 3                 # the sharing whose top coefficient is 0: the only one mpe_vss_validate_share refuses


@functools.lru_cache(maxsize=None)
def deal_case(t, n):
    """67 dealers: dict(coef [67, (t+1) 8] words, commits [67, (t+1) 16], shares [67, n 8], valid [67 n] = what validate_share must say)"""
    r = F.Rng("deal-%d-%d" % (t, n))
    coefs = [[r.below(Q - 1) + 1 for _ in range(t + 1)] for _ in range(DEAL_BATCH)]
    coefs[0] = [1] * (t + 1)
    coefs[1] = [Q - 1] * (t + 1)
    coefs[2] = [Q + 5] + [(1 << 256) - 1] * t                  # values >= q: reduced as read
    coefs[DEAL_ZERO_DEALER][t] = 0
    dealt = [vss_share(c, n) for c in coefs]
    valid = [0 if b == DEAL_ZERO_DEALER else 1 for b in range(DEAL_BATCH) for _ in range(n)]
    return dict(coef=F.words([c for cs in coefs for c in cs], 8).reshape(DEAL_BATCH, (t + 1) * 8),
                commits=F.point_words([c for d in dealt for c in d[0]]).reshape(DEAL_BATCH, (t + 1) * 16),
                shares=F.words([s for d in dealt for s in d[1]], 8).reshape(DEAL_BATCH, n * 8), valid=valid, coef_ints=coefs)


CONSTRUCT_BATCH = 67
CONSTRUCT_SHAPES = [3, 5]


@functools.lru_cache(maxsize=None)
def construct_case(n):
    """67 (session, party) items: dict(shares [67, n 8], y [67, n 16], nonce [67, 8] and the expected x, ysum, pk, R, z)"""
    r = F.Rng("construct-%d" % n)
    B = CONSTRUCT_BATCH
    shares = [[r.below(Q) for _ in range(n)] for _ in range(B)]
    ys = [[pyref.ec_mul(r.below(1 << 24) + 1, G) for _ in range(n)] for _ in range(B)]       # short scalars: points are points
    nonce = [r.below(Q - 1) + 1 for _ in range(B)]
    shares[0] = [Q - 1] * n                                                  # the sum wraps mod q
    shares[1] = [shares[1][0], Q - shares[1][0]] + [0] * (n - 2)             # x = 0: pk is the neutral row
    shares[5][0] = (1 << 256) - 1                                            # a row >= q
    ys[2][1] = ys[2][0]                                                      # equal summands: a doubling
    ys[3][1] = pyref.ec_neg(ys[3][0])                                        # P + (-P): a neutral intermediate
    ys[4] = [ys[4][0], pyref.ec_neg(ys[4][0])] + [None] * (n - 2)            # neutral operands and a neutral sum
    want = [construct_keypair(s, y, k) for s, y, k in zip(shares, ys, nonce)]
    return dict(shares=F.words([s for row in shares for s in row], 8).reshape(B, n * 8),
                y=F.point_words([p for row in ys for p in row]).reshape(B, n * 16), nonce=F.words(nonce, 8),
                x=F.words([w[0] for w in want], 8), ysum=F.point_words([w[1] for w in want]), pk=F.point_words([w[2] for w in want]),
                R=F.point_words([w[3] for w in want]), z=F.words([w[4] for w in want], 8))


def _session(r, t, n, identical=None, opposite=None):
    """one honest keygen session: (commits[j][k], proofs[i]); identical = (a, b): dealer b repeats dealer a's polynomial;
    opposite = (a, b): dealer b's coefficient 1 is minus dealer a's"""
    coefs = [[r.below(Q - 1) + 1 for _ in range(t + 1)] for _ in range(n)]
    if identical:
        coefs[identical[1]] = list(coefs[identical[0]])
    if opposite:
        coefs[opposite[1]][1] = Q - coefs[opposite[0]][1]
    dealt = [vss_share(c, n) for c in coefs]
    proofs = [dlog_prove(sum(d[1][i] for d in dealt) % Q, r.below(Q - 1) + 1) for i in range(n)]
    return [d[0] for d in dealt], proofs


def _pack(sessions):
    commits = F.point_words([c for cs, _ in sessions for row in cs for c in row])
    n, t1 = len(sessions[0][0]), len(sessions[0][0][0])
    pr = [p for _, ps in sessions for p in ps]
    return dict(commits=commits.reshape(len(sessions) * n, t1 * 16), pk=F.point_words([p[0] for p in pr]), R=F.point_words([p[1] for p in pr]),
                z=F.words([p[2] for p in pr], 8))


def _expect(case, n, t1):
    """the restatement on the (tampered) words of a packed case"""
    S = case["pk"].shape[0] // n
    cp = F.points(case["commits"].reshape(-1, 16))
    pk, R, z = F.points(case["pk"]), F.points(case["R"]), F.ints(case["z"])
    ok, bad, xi = [], [], []
    for s in range(S):
        commits = [[cp[(s * n + j) * t1 + k] for k in range(t1)] for j in range(n)]
        o, b, x = verify_round3(commits, [(pk[s * n + i], R[s * n + i], z[s * n + i]) for i in range(n)])
        ok += o
        bad.append(b)
        xi += x
    return dict(case, ok=ok, bad=bad, xi=F.point_words(xi))


def _other_proof(r):
    return dlog_prove(r.below(Q - 1) + 1, r.below(Q - 1) + 1)        # valid by itself, for a scalar the dealers never shared


def _put(case, row, proof):
    case["pk"][row], case["R"][row] = F.point_words([proof[0]])[0], F.point_words([proof[1]])[0]
    case["z"][row] = F.words([proof[2]], 8)[0]


def _swap(case, a, b):
    for f in ("pk", "R", "z"):
        case[f][[a, b]] = case[f][[b, a]]


# what the tables below must yield: the tests compare the restatement AND the device with these literal lists
ROUND3_WANT = {
    (1, 3): ([1, 1, 1,  1, 0, 1,  1, 1, 0,  0, 1, 0,  1, 1, 1,  1, 1, 1,  0, 0, 0,  0, 1, 1], [0, 0b010, 0b100, 0b101, 0, 0, 0b111, 0b001]),
    (2, 5): ([1, 1, 1, 1, 1,  1, 0, 1, 0, 0,  0, 1, 1, 1, 0,  0, 0, 0, 0, 0], [0, 0b11010, 0b10001, 0b11111]),
}
ROUND3_OFFCURVE_SESSION = {(1, 3): 6, (2, 5): 3}


@functools.lru_cache(maxsize=None)
def round3_case(t, n):
    """(t, n) = (1, 3): 8 sessions, one table row each — clean; one bit of z flipped; a party's proof replaced by a valid proof for another
    scalar; the proofs of two parties swapped; two dealers with identical commitments; two dealers with opposite commitments at k = 1;
    an off-curve commitment; a neutral pk.  (2, 5): the same eight rows in 4 sessions (clean | flipped z, foreign proof, neutral pk |
    identical dealers, opposite dealers, swapped proofs | off-curve)."""
    r = F.Rng("round3-%d-%d" % (t, n))
    if (t, n) == (1, 3):
        c = _pack([_session(r, t, n), _session(r, t, n), _session(r, t, n), _session(r, t, n), _session(r, t, n, identical=(0, 1)),
                   _session(r, t, n, opposite=(0, 1)), _session(r, t, n), _session(r, t, n)])
        c["z"][1 * n + 1, 2] ^= 0x400
        _put(c, 2 * n + 2, _other_proof(r))
        _swap(c, 3 * n + 0, 3 * n + 2)
        c["commits"][6 * n + 1, 8] ^= 1                           # dealer 1, k = 0: y no longer fits x
        c["pk"][7 * n + 0] = 0
    elif (t, n) == (2, 5):
        c = _pack([_session(r, t, n), _session(r, t, n), _session(r, t, n, identical=(0, 1), opposite=(2, 3)), _session(r, t, n)])
        c["z"][1 * n + 1, 7] ^= 1
        _put(c, 1 * n + 3, _other_proof(r))
        c["pk"][1 * n + 4] = 0
        _swap(c, 2 * n + 0, 2 * n + 4)
        c["commits"][3 * n + 4, 2 * 16 + 3] ^= 0x80               # dealer 4, k = 2: x no longer fits y
    else:
        raise ValueError((t, n))
    return _expect(c, n, t + 1)


def round3_profile_case(profile):
    """the clean and the flipped-z row of the (1, 3) table, proved and verified under `profile` (the caller applies it)"""
    t, n = 1, 3
    r = F.Rng("round3-profile-" + profile)
    c = _pack([_session(r, t, n), _session(r, t, n)])
    c["z"][1 * n + 1, 2] ^= 0x400
    return _expect(c, n, t + 1)


ROUND3_PROFILE_WANT = ([1, 1, 1, 1, 0, 1], [0, 0b010])


# ---- Lagrange: what a (t + 1)-subset of the x_i reconstructs ------------------------------------------------------------------
def lagrange_at_zero(xs, idx):
    """sum_i x_i prod_{j != i} (j + 1) / ((j + 1) - (i + 1)) over the party indices idx (0-based), mod q"""
    acc = 0
    for i in idx:
        lam = 1
        for j in idx:
            if j != i:
                lam = lam * (j + 1) * pow(j - i, -1, Q) % Q
        acc = (acc + xs[i] * lam) % Q
    return acc
