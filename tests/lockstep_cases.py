"""Batches of GG20 signing sessions in which clean sessions alternate with degenerate ones, for the lock-step signer
(`mpe_gg20_sign`) and its ahead-of-time schedule (mpe_gg20.h round0 / round1 / round2: the inversion of round 1's ciphertexts, the
PDL proofs' beta^N ladders).  Every degenerate session is made from INPUTS alone — a sampled value or a key value overwritten, no
message tampered with — so the same arrays go through the oracle (`G.oracle_sign_ex`) and through the one-call signer unchanged.
What a session must give is what the oracle gives: no status is written down here as an expectation.

`batches(keys)` -> {name: Batch}; `expected(batch)` -> the oracle's dict (cached per batch object);
tests/test_lockstep_cases_cpu.py checks that the table is not vacuous, tests/test_lockstep_failures_gpu.py runs it on the GPU."""
import numpy as np

import fixtures as F
import gg20_fixture as G
import pyref

Q = pyref.Q
KEY_FIELDS = ("x", "p", "q", "Nt", "h1", "h2", "y", "X")


class Batch:
    def __init__(self, name, lk, nonces, B, keyset=None, kw=None, recipes=None, wallets=None):
        self.name, self.lk, self.nonces, self.B, self.keyset, self.kw = name, lk, nonces, B, keyset, dict(kw or {})
        self.recipes = recipes or {}                 # session -> name of the recipe that made it degenerate
        self.wallets = wallets                       # per key set: the fixture whose public key its clean signatures verify under
        self._want = None

    @property
    def shape(self):
        return self.lk["t"], self.lk["n"], [int(x) for x in self.lk["arrays"]["signers"]]

    def public_key(self, b):
        return (self.wallets[int(self.keyset[b])] if self.wallets else self.lk)["y"]


def host_threads():
    import bench
    return max(1, min(bench.host_cores()[0], 32))


def take(nonces, B, sessions):
    """the rows of the chosen sessions, as a batch of len(sessions)"""
    out = {}
    for f, v in nonces.items():
        per = v.shape[0] // B
        out[f] = np.ascontiguousarray(v.reshape(B, per, v.shape[1])[list(sessions)].reshape(len(sessions) * per, v.shape[1]))
    return out


def oracle(lk, nonces, B, keyset=None, sessions=None, threads=None):
    """`G.oracle_sign_ex` over the chosen sessions (default: all), spread over the host threads (ctypes releases the GIL).  Returns
    dict(r, s, recid, R, status [len(sessions)], party_status [S][len(sessions)]) in the order of `sessions`."""
    from concurrent.futures import ThreadPoolExecutor
    sessions = list(range(B)) if sessions is None else list(sessions)
    threads = threads or host_threads()
    parts = [list(c) for c in np.array_split(np.array(sessions, dtype=np.int64), min(threads, len(sessions))) if len(c)]

    def run(ix):
        return G.oracle_sign_ex(lk, take(nonces, B, ix), len(ix), keyset=None if keyset is None else np.asarray(keyset)[ix])
    with ThreadPoolExecutor(len(parts)) as ex:
        outs = list(ex.map(run, parts))
    got = {f: np.concatenate([o[f] for o in outs]) for f in ("r", "s", "recid", "R", "status")}
    got["party_status"] = np.concatenate([o["party_status"] for o in outs], axis=1)
    return got


def expected(batch):
    """the oracle's word on the batch (cached on the batch object)"""
    if batch._want is None:
        batch._want = oracle(batch.lk, batch.nonces, batch.B, keyset=batch.keyset)
    return batch._want


# ---- recipes: (lk, nonces, b) -> None, one value of session b overwritten in place ------------------------------------------------
def _put(nonces, field, row, value):
    nonces[field][row] = F.words([value], nonces[field].shape[1])[0]


def _get(nonces, field, row):
    return F.ints(nonces[field][row:row + 1])[0]


def _key(lk, ordinal):
    return lk["keys"][int(lk["arrays"]["signers"][ordinal])]


def _mb_row(lk, b, i, ind, v):
    """MessageB number v (0: gamma, 1: w) of sender ordinal i for receiver ordinal ind"""
    S = lk["S"]
    return ((b * S + i) * (S - 1) + (ind if ind < i else ind - 1)) * 2 + v


def non_unit_r_a(i):
    """Paillier randomness a multiple of the party's own p: the ciphertext of k_i is not a unit modulo N^2"""
    def f(lk, z, b):
        _put(z, "r_a", b * lk["S"] + i, 12345 * _key(lk, i).p)
    return f


def zero_r_a(i):
    def f(lk, z, b):
        _put(z, "r_a", b * lk["S"] + i, 0)
    return f


def opposite(field):
    """two signers: party 1's value = q - party 0's (gamma: delta = 0 has no inverse; k: the nonce k = 0)"""
    def f(lk, z, b):
        assert lk["S"] == 2
        _put(z, field, b * 2 + 1, Q - _get(z, field, b * 2))
    return f


def wide_al_alpha(i, ind):
    """the range proof of party i under party ind's statement answers with s1 > q^3"""
    def f(lk, z, b):
        _put(z, "al_alpha", (b * lk["S"] + i) * lk["n"] + int(lk["arrays"]["signers"][ind]), Q ** 3 + 5)
    return f


def scalar(field, i, value):
    def f(lk, z, b):
        _put(z, field, b * lk["S"] + i, value)
    return f


def non_unit_mb_r(i, ind, v=0):
    """the randomness of one MessageB of party i a multiple of the RECEIVER's p"""
    def f(lk, z, b):
        _put(z, "mb_r", _mb_row(lk, b, i, ind, v), 777 * _key(lk, ind).p)
    return f


def wide_pdl_alpha(i, ind):
    """a PDL nonce above its sampling range: the proof has slack for it, the session signs"""
    def f(lk, z, b):
        S = lk["S"]
        _put(z, "pdl_alpha", (b * S + i) * (S - 1) + (ind if ind < i else ind - 1), (1 << 767) + 1)
    return f


TWO_SIGNER_RECIPES = {
    "r_a not a unit": non_unit_r_a(0),
    "gamma sums to 0": opposite("gamma"),
    "k sums to 0": opposite("k"),
    "al_alpha above q^3": wide_al_alpha(1, 0),
    "k = 2^256 - 1": scalar("k", 0, (1 << 256) - 1),
    "r_a = 0": zero_r_a(1),
    "mb_r not a unit": non_unit_mb_r(0, 1),
    "pdl_alpha = 2^767 + 1": wide_pdl_alpha(0, 1),
}
# the recipes that the 1 024-session batch cycles through (statuses 91 / 101 / 201 / 301 by the oracle)
CYCLE = ["k = 2^256 - 1", "r_a not a unit", "mb_r not a unit", "gamma sums to 0"]


def _alternating(name, keys, t, n, signers, recipes, seed, kw=None, tail_clean=1):
    """clean, degenerate, clean, degenerate, ..., clean"""
    lk = G.make_local_keys(keys, t, n, signers)
    B = 2 * len(recipes) + tail_clean
    z = G.make_nonces(lk, B, seed=seed)
    used = {}
    for j, (nm, f) in enumerate(recipes.items()):
        f(lk, z, 2 * j + 1)
        used[2 * j + 1] = nm
    return Batch(name, lk, z, B, kw=kw, recipes=used)


def _placed(name, keys, t, n, signers, B, where, seed, kw=None):
    """where: {session: recipe name of TWO_SIGNER_RECIPES}"""
    lk = G.make_local_keys(keys, t, n, signers)
    z = G.make_nonces(lk, B, seed=seed)
    for b, nm in where.items():
        TWO_SIGNER_RECIPES[nm](lk, z, b)
    return Batch(name, lk, z, B, kw=kw, recipes=dict(where))


def multi_wallet(keys, B=9):
    """Four wallets in one launch: wallet 0 sound, wallet 1 with a signer's X doubled, wallet 2 with one bit of a signer's N~ flipped,
    wallet 3 with a wrong y.  Sessions alternate between wallet 0 and one of the others."""
    t, n, signers, K = 1, 3, [0, 2], 4
    lks = [G.make_local_keys(keys[kk:] + keys[:kk], t, n, signers, seed=f"lockstep-wallet-{kk}") for kk in range(K)]
    arrays = {f: np.concatenate([lk["arrays"][f] for lk in lks]) for f in KEY_FIELDS}
    arrays["signers"] = lks[0]["arrays"]["signers"]
    X1 = F.points(lks[1]["arrays"]["X"])
    arrays["X"][1 * n + 0] = F.point_words([pyref.ec_add(X1[0], X1[0])])[0]      # wallet 1: X of signer 0 doubled
    # wallet 2: one bit of signer 0's N~ (the modulus stays odd; with THIS bit it shares the factor 11 with h2, so the range proofs made
    # under it have no inverse for z — a flip that leaves gcd(h1 h2, N~) = 1 signs, prover and verifier read the same array)
    arrays["Nt"][2 * n + 0, 63] ^= np.uint32(1 << 30)
    arrays["y"][3] = F.point_words([pyref.ec_mul(999, pyref.G)])[0]              # wallet 3: not the wallet's public key
    lkm = dict(lks[0], arrays=arrays, nkeysets=K)
    keyset = np.array([0 if b % 2 == 0 else 1 + (b // 2) % 3 for b in range(B)], dtype=np.int32)
    parts = [G.make_nonces(lks[int(keyset[b])], 1, seed=f"lockstep-mw-{b}") for b in range(B)]
    z = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
    names = {1: "wallet with a doubled X", 2: "wallet with a flipped N~ bit", 3: "wallet with a wrong y"}
    return Batch("multi-wallet", lkm, z, B, keyset=keyset, recipes={b: names[int(keyset[b])] for b in range(B) if keyset[b]}, wallets=lks)


# the batches that are NOT built as "clean neighbours on both sides, at least half clean", on purpose
EXEMPT = ("chunking", "every session fails")
CLEAN_SHAPE = (1, 3, [0, 1])


def batches(keys):
    out = {}
    add = lambda bt: out.__setitem__(bt.name, bt)
    # every recipe of the two-signer table in a session of its own
    add(_alternating("two signers", keys, 1, 3, [0, 2], TWO_SIGNER_RECIPES, "lockstep-two"))
    # three signers: two peers judge the same sender
    add(_alternating("three signers", keys, 2, 5, [0, 2, 4], {"gamma = 0 (a 91 party)": scalar("gamma", 1, 0), "r_a not a unit": non_unit_r_a(1)},
                     "lockstep-three"))
    add(_alternating("dedup_verify", keys, 2, 4, [1, 2, 3], {"r_a not a unit": non_unit_r_a(2), "mb_r not a unit": non_unit_mb_r(0, 2, 1)},
                     "lockstep-dedup", kw={"dedup_verify": True}))
    add(multi_wallet(keys))
    # chunk = 3 over 11 sessions: [0..2] mixed, [3..5] failing only, [6..8] clean only, [9..10] ragged with a failure at the very end
    add(_placed("chunking", keys, 1, 3, [0, 2], 11, {1: "r_a not a unit", 3: "k = 2^256 - 1", 4: "r_a = 0", 5: "mb_r not a unit",
                                                    10: "gamma sums to 0"}, "lockstep-chunks", kw={"chunk": 3}))
    # the wallet and signer set of the clean parity case of tests/test_paths_gpu.py: one key object serves these two and clean_batch
    add(_placed("every session fails", keys, *CLEAN_SHAPE, 4, {0: "r_a not a unit", 1: "k = 2^256 - 1", 2: "mb_r not a unit", 3: "k sums to 0"},
                "lockstep-all-fail"))
    add(_placed("wallet of the clean case", keys, *CLEAN_SHAPE, 7, {1: "r_a not a unit", 3: "mb_r not a unit", 5: "gamma sums to 0"},
                "lockstep-reuse"))
    add(sampled_batch(keys)[0])
    return out


def clean_batch(keys, B=5):
    """sessions that all sign, for the wallet of CLEAN_SHAPE (the (1, 3, [0, 1]) x 5, chunk = 2 case of tests/test_paths_gpu.py)"""
    lk = G.make_local_keys(keys, *CLEAN_SHAPE)
    return Batch("clean", lk, G.make_nonces(lk, B, seed="lockstep-clean-after-failures"), B, kw={"chunk": 2})


SAMPLER_SEED = bytes(range(64, 96))
SAMPLER_COUNTER, SAMPLER_ATTEMPTS = 10, 3      # (a batch counter whose given-up draws sit between sessions that sign)
SAMPLER_COUNTER_2 = 3                          # a second batch for the pipeline's pass


def sampled_batch(keys, B=12):
    """nonces as the device sampler gives them when a draw gives up after three candidates (tests/test_sampler_gpu.py): the oracle's
    expansion of the same seed.  Returns (Batch, msg words, the oracle's count of given-up draws)."""
    import hashlib
    import orc
    lk = G.make_local_keys(keys, 1, 3, [0, 1])
    msg = F.words([int.from_bytes(hashlib.sha256(b"lockstep gives up %d" % b).digest(), "big") for b in range(B)], 8)
    try:
        orc.lib.orc_sampler_set_max_attempts(SAMPLER_ATTEMPTS)
        z, fails = G.oracle_sample_nonces(lk, B, SAMPLER_SEED, SAMPLER_COUNTER, msg=msg)
    finally:
        orc.lib.orc_sampler_set_max_attempts(128)
    return Batch("sampled", lk, z, B), msg, fails


# ---- the shipped thresholds: 1 024 sessions, failing ones at wave and lane-group edges ----------------------------------------------
FULLSIZE_B = 1024
FULLSIZE_FAILING = [0, 15, 16, 63, 64, 511, 512, FULLSIZE_B - 1]


def fullsize_overwrite(lk, nonces):
    """nonces: host arrays of FULLSIZE_B sessions (two signers); returns {session: recipe name}"""
    where = {b: CYCLE[j % len(CYCLE)] for j, b in enumerate(FULLSIZE_FAILING)}
    for b, nm in where.items():
        TWO_SIGNER_RECIPES[nm](lk, nonces, b)
    return where


def fullsize_sample():
    """the sessions compared with the oracle: every failing one, both neighbours of each, and a stride of clean ones"""
    pick = set(FULLSIZE_FAILING)
    for b in FULLSIZE_FAILING:
        pick.update(x for x in (b - 1, b + 1) if 0 <= x < FULLSIZE_B)
    pick.update(range(5, FULLSIZE_B, 41))
    return sorted(pick)
