"""Plain-Python restatement of the presignature pool (include/mpecdsa_hip.h, "the presignature pool"), over the helpers of
pyref_gg20.py: the slot state machine, `phase7_local_sig` (party_i.rs:850-871), `output_signature` with its verify
(party_i.rs:873-936) and the export record.  Written from the header's text, not from csrc/mpe_presig.h.

A presignature of one session is dict(keyset=int, parties=[dict(k=int, sigma=int, R=(x, y)) per local party]) — what
`CompletedOfflineStage` (state_machine/sign/rounds.rs:647-661) carries into `SignManual::new` for those parties."""
import pyref as R
import pyref_gg20 as PG

Q = PG.Q
EMPTY, READY, SIGNED, BUSY = 0, 1, 2, 3
RECORD_VERSION = 1
DEPOSIT_RANGE, DEPOSIT_NOT_EMPTY, SESSION_FAILED = 801, 802, 803
SIGN_RANGE, SIGN_NOT_READY = 811, 812
COMPLETE_RANGE, COMPLETE_NOT_SIGNED, VERIFY_FAILED = 821, 822, 701
RECORD_RANGE, IMPORT_REFUSED, EXPORT_NOT_READY, IMPORT_NOT_EMPTY = 831, 832, 833, 834
REC_HEAD, REC_PARTY = 28, 32


def phase7_local_sig(msg, k, sigma, Rp):
    """(m, r, s_i): m = msg mod q (`Scalar::from(message)`, party_i.rs:857), r = R.x mod q, s_i = m k_i + r sigma_i"""
    m, r = msg % Q, Rp[0] % Q
    return m, r, (m * k + r * sigma) % Q


def output_signature(s_parts, m, r, Rp, y):
    """(status, r, s, recid) from the partial signatures of ALL signers: the sum, the low-s rule with the recid flip, verify;
    outputs are zero unless status == 0"""
    s = sum(s_parts) % Q
    recid = (Rp[1] % Q) & 1
    if s > Q - s:
        s, recid = Q - s, recid ^ 1
    if s == 0 or not R.ecdsa_verify(y, m, r, s):
        return VERIFY_FAILED, 0, 0, 0
    return 0, r, s, recid


def on_curve(pt):
    """what `ec::aff_valid` accepts: canonical coordinates of a point of the curve (never the neutral element)"""
    return pt is not None and 0 <= pt[0] < R.P and 0 <= pt[1] < R.P and (pt[1] * pt[1] - pt[0] ** 3 - 7) % R.P == 0


def signer_mask(signers):
    m = 0
    for s in signers:
        m |= 1 << int(s)
    return m


def _w(v, n):
    return [(int(v) >> (32 * j)) & 0xFFFFFFFF for j in range(n)]


def _i(ws):
    return sum(int(w) << (32 * j) for j, w in enumerate(ws))


def record_pack(mask, local, keyset, y, parties):
    """the record of include/mpecdsa_hip.h as a list of 28 + 32 L 32-bit words"""
    out = [RECORD_VERSION, mask, len(local)] + [int(x) for x in local] + [0] * (8 - len(local)) + [keyset] + _w(y[0], 8) + _w(y[1], 8)
    for p in parties:
        out += _w(p["k"], 8) + _w(p["sigma"], 8) + _w(p["R"][0], 8) + _w(p["R"][1], 8)
    assert len(out) == REC_HEAD + REC_PARTY * len(local)
    return out


def record_unpack(words):
    """-> dict(version, mask, L, local [8], keyset, y, parties); L is taken from the length of the list, not trusted from the words"""
    L = (len(words) - REC_HEAD) // REC_PARTY
    assert len(words) == REC_HEAD + REC_PARTY * L
    parties = []
    for li in range(L):
        p = words[REC_HEAD + REC_PARTY * li:REC_HEAD + REC_PARTY * (li + 1)]
        parties.append(dict(k=_i(p[0:8]), sigma=_i(p[8:16]), R=(_i(p[16:24]), _i(p[24:32]))))
    return dict(version=words[0], mask=words[1], L=words[2], local=list(words[3:11]), keyset=words[11], y=(_i(words[12:20]), _i(words[20:28])),
                parties=parties)


class IllegalTransition(Exception):
    pass


class Pool:
    """The slot state machine.  Every call returns the row status the C-ABI reports and changes a slot only when that status is 0
    (complete: also on 701, which frees the slot).  signers: party indices; local: signer ordinals; ys: the key sets' public keys."""

    def __init__(self, signers, local, ys, capacity):
        self.signers, self.local, self.ys, self.capacity = [int(s) for s in signers], [int(x) for x in local], list(ys), capacity
        self.mask = signer_mask(signers)
        self.state = [EMPTY] * capacity
        self.slot = [None] * capacity

    def _in(self, slot):
        return 0 <= slot < self.capacity

    def deposit(self, slot, presig, healthy=True):
        if not healthy:
            return SESSION_FAILED
        if not self._in(slot):
            return DEPOSIT_RANGE
        if self.state[slot] != EMPTY:
            return DEPOSIT_NOT_EMPTY
        self.state[slot], self.slot[slot] = READY, dict(keyset=presig["keyset"], parties=[dict(p) for p in presig["parties"]])
        return 0

    def sign(self, slot, msg):
        """-> (status, [s_i per local party]); the slot keeps m, r, s_i and loses k_i, sigma_i"""
        L = len(self.local)
        if not self._in(slot):
            return SIGN_RANGE, [0] * L
        if self.state[slot] != READY:
            return SIGN_NOT_READY, [0] * L
        out = []
        for p in self.slot[slot]["parties"]:
            m, r, s_i = phase7_local_sig(msg, p["k"], p["sigma"], p["R"])
            p.update(k=0, sigma=0, m=m, r=r, s_i=s_i)
            out.append(s_i)
        self.state[slot] = SIGNED
        return 0, out

    def complete(self, slot, s_all):
        """s_all: the partial signatures of all S senders, the own included -> [(status, r, s, recid) per local party]"""
        L = len(self.local)
        if not self._in(slot):
            return [(COMPLETE_RANGE, 0, 0, 0)] * L
        if self.state[slot] != SIGNED:
            return [(COMPLETE_NOT_SIGNED, 0, 0, 0)] * L
        sl = self.slot[slot]
        out = []
        for li, p in enumerate(sl["parties"]):
            parts = [p["s_i"] if j == self.local[li] else s_all[j] % Q for j in range(len(self.signers))]
            out.append(output_signature(parts, p["m"], p["r"], p["R"], self.ys[sl["keyset"]]))
        self.state[slot], self.slot[slot] = EMPTY, None
        return out

    def export(self, slot):
        if not self._in(slot):
            return RECORD_RANGE, None
        if self.state[slot] != READY:
            return EXPORT_NOT_READY, None
        sl = self.slot[slot]
        rec = record_pack(self.mask, self.local, sl["keyset"], self.ys[sl["keyset"]], sl["parties"])
        self.state[slot], self.slot[slot] = EMPTY, None
        return 0, rec

    def record_ok(self, words):
        if len(words) != REC_HEAD + REC_PARTY * len(self.local):
            return False
        r = record_unpack(words)
        if r["version"] != RECORD_VERSION or r["mask"] != self.mask or r["L"] != len(self.local):
            return False
        if r["local"] != self.local + [0] * (8 - len(self.local)) or not r["keyset"] < len(self.ys) or r["y"] != self.ys[r["keyset"]]:
            return False
        return all(0 < p["k"] < Q and 0 <= p["sigma"] < Q and on_curve(p["R"]) for p in r["parties"])

    def import_(self, slot, words):
        if not self._in(slot):
            return RECORD_RANGE
        if not self.record_ok(words):
            return IMPORT_REFUSED
        if self.state[slot] != EMPTY:
            return IMPORT_NOT_EMPTY
        r = record_unpack(words)
        self.state[slot], self.slot[slot] = READY, dict(keyset=r["keyset"], parties=r["parties"])
        return 0

    def discard(self, slot):
        if self._in(slot):
            self.state[slot], self.slot[slot] = EMPTY, None

    def audit(self):
        """(slots per state [4], stray): stray = slots outside READY that still hold a non-zero k_i or sigma_i"""
        counts = [self.state.count(s) for s in (EMPTY, READY, SIGNED, BUSY)]
        stray = sum(1 for st, sl in zip(self.state, self.slot) if st != READY and sl is not None
                    for p in sl["parties"] if p["k"] or p["sigma"])
        return counts, stray

    def strict(self, call, slot, *args):
        """the same calls, raising IllegalTransition instead of returning a non-zero status"""
        out = getattr(self, call)(slot, *args)
        code = out if isinstance(out, int) else (out[0][0] if call == "complete" else out[0])
        if code not in (0, VERIFY_FAILED):
            raise IllegalTransition(f"{call}(slot {slot}): {code}")
        return out
