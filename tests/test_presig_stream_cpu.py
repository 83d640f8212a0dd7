"""CPU: the two row rules this library adds on top of the presignature pool, stated in plain Python from the header's text and
checked against tests/pyref_presig.py over all small cases, and the generated binding's view of the new entry points.

  * the status rule of mpe_gg20_presign_sets: the session's smallest non-zero party status if it failed, otherwise the deposit's
    801 / 802, otherwise 0; a row with a non-zero status leaves its slot untouched;
  * the fused online rule of mpe_gg20_sign_online: the claim's 811 / 812, every s_i, the sum, ONE output_signature — against the
    composition Pool.sign + Pool.complete folded the way engine.gg20_sign_online folds it."""
import itertools
import os
import re

import pyref
import pyref_presig as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = PP.Q
CAP = 3


def presign_row_status(party_status, deposit_code):
    failed = [s for s in party_status if s]
    return min(failed) if failed else deposit_code


def sign_online_row(pool, slot, msg):
    """(status, r, s, recid), and the slot is EMPTY afterwards when the claim was won"""
    if not 0 <= slot < pool.capacity:
        return PP.SIGN_RANGE, 0, 0, 0
    if pool.state[slot] != PP.READY:
        return PP.SIGN_NOT_READY, 0, 0, 0
    sl = pool.slot[slot]
    parts, m, r = [], None, None
    for p in sl["parties"]:
        m, r, s_i = PP.phase7_local_sig(msg, p["k"], p["sigma"], sl["parties"][0]["R"])
        parts.append(s_i)
    out = PP.output_signature(parts, m, r, sl["parties"][0]["R"], pool.ys[sl["keyset"]])
    pool.state[slot], pool.slot[slot] = PP.EMPTY, None
    return out


def composed_row(pool, slot, msg):
    """sign + complete as engine.gg20_sign_online folds them: the sign status, else the smallest non-zero party status; party 0's output"""
    st7, s_all = pool.sign(slot, msg)
    if st7:
        return st7, 0, 0, 0
    res = pool.complete(slot, s_all)
    bad = [x[0] for x in res if x[0]]
    return (min(bad), 0, 0, 0) if bad else res[0]


def presig(x, shares_k, shares_sigma_delta=0):
    """an additive presignature of the key x: k = sum k_i, R = k^-1 G, sigma_i additive shares of k x"""
    k = sum(shares_k) % Q
    Rp = pyref.ec_mul(pow(k, -1, Q), pyref.G)
    sigma = [(k * x - 77 * (len(shares_k) - 1) + shares_sigma_delta) % Q] + [77] * (len(shares_k) - 1)
    return dict(keyset=0, parties=[dict(k=ki, sigma=si, R=Rp) for ki, si in zip(shares_k, sigma)])


def test_presign_status_rule_over_all_small_cases():
    party = [(0, 0), (92, 92), (0, 401), (501, 0), (602, 301)]                    # per-party statuses of a session, S = 2
    slot_kinds = [0, 1, -1, CAP, "occupied"]
    x = 0xC0FFEE
    y, held, fresh = pyref.ec_mul(x, pyref.G), presig(x, [5, 6]), [presig(x, [11 + b, 13]) for b in range(2)]
    for rows in itertools.product(itertools.product(party, slot_kinds), repeat=2):     # two rows: duplicates of a slot included
        pool = PP.Pool([0, 1], [0, 1], [y], CAP)
        assert pool.deposit(2, held) == 0
        before = None
        for b, (pst, kind) in enumerate(rows):
            slot = 2 if kind == "occupied" else kind
            before = (list(pool.state), [None if s is None else dict(s) for s in pool.slot])
            code = pool.deposit(slot, fresh[b], healthy=not any(pst))
            status = presign_row_status(pst, code)
            # never the blanket 803; a failed session reads its own smallest status
            assert status != PP.SESSION_FAILED
            if any(pst):
                assert status == min(s for s in pst if s) and code == PP.SESSION_FAILED
            elif slot in (-1, CAP):
                assert status == PP.DEPOSIT_RANGE
            elif before[0][slot] != PP.EMPTY:
                assert status == PP.DEPOSIT_NOT_EMPTY                             # occupied before the call, or won by the row before
            else:
                assert status == 0 and pool.state[slot] == PP.READY
            if status:
                assert (list(pool.state), pool.slot) == before                    # the slot is untouched
        assert pool.slot[2] == held


def test_fused_online_rule_equals_sign_then_complete_over_all_small_cases():
    x = 0x1234567890ABCDEF
    y = pyref.ec_mul(x, pyref.G)
    msg = 0xFEEDFACE << 200
    made = {True: presig(x, [21, 22]), False: presig(x, [21, 22], 1), "other": presig(x, [Q - 5, 9])}      # False: sigma_0 altered by one: 701
    cases = []
    for healthy in (True, False):
        for slots in ([0], [1], [-1], [CAP], [2], [0, 0], [0, 1, 0], [1, 7, 1, 0]):      # slot 2 stays EMPTY; duplicates; out of range
            cases.append((healthy, slots))
    seen = set()
    for healthy, slots in cases:
        pools = []
        for _ in range(2):
            p = PP.Pool([0, 1], [0, 1], [y], CAP)
            assert p.deposit(0, made[healthy]) == 0 and p.deposit(1, made["other"]) == 0
            pools.append(p)
        for slot in slots:
            a, b = sign_online_row(pools[0], slot, msg), composed_row(pools[1], slot, msg)
            assert a == b, (healthy, slots, slot)
            assert a[0] == 0 or a[1:] == (0, 0, 0)
            if a[0] == 0:
                assert pyref.ecdsa_verify(y, msg % Q, a[1], a[2]) and a[2] <= Q - a[2]
            seen.add(a[0])
            assert pools[0].audit() == pools[1].audit() and pools[0].state == pools[1].state
        assert pools[0].audit()[1] == 0
    assert seen == {0, PP.SIGN_RANGE, PP.SIGN_NOT_READY, PP.VERIFY_FAILED}


def test_generated_binding_lists_the_new_symbols_with_the_headers_argument_counts():
    from multi_party_ecdsa_amd import _abi, _native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpecdsa_hip.h")).read(), flags=re.S)
    declared = {name: len([a for a in args.split(",") if a.strip()]) for name, args in re.findall(r"\b(mpe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)}
    want = dict(mpe_gg20_presign_sets=12, mpe_gg20_sign_online=9, mpe_gg20_pipeline_create_presig=8, mpe_gg20_pipeline_submit_presig=8,
                mpe_gg20_pipeline_submit_presig_seeded=9, mpe_gg20_pipeline_submit_sets=11, mpe_gg20_pipeline_submit_seeded_sets=13)
    for name, nargs in want.items():
        assert declared[name] == nargs, name
        assert len(_abi.SIGNATURES[name][1]) == nargs, name
        assert name in _native.EXPORTED and hasattr(_native.lib, name)
        assert len(getattr(_native.lib, name).argtypes) == nargs
    # the forwarding pairs differ by the one set argument
    for old, new in (("mpe_gg20_pipeline_submit", "mpe_gg20_pipeline_submit_sets"), ("mpe_gg20_pipeline_submit_seeded", "mpe_gg20_pipeline_submit_seeded_sets")):
        assert len(_abi.SIGNATURES[new][1]) == len(_abi.SIGNATURES[old][1]) + 1
