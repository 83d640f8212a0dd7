"""Failing sessions on the lock-step signer's ahead-of-time schedule.  `mpe_gg20_sign` is the only call that computes values ahead
(mpe_gg20.h: round 0 inverts the ciphertexts round 1's verifiers need from the parties' LOCAL c_a, the PDL proofs' beta^N ladders
start in rounds 0 and 2 at wave priority 0, MessageB's DLog proofs go first); the tamper matrix goes through the per-round calls and
the small failing batches of the other files through a schedule with nothing ahead.  Here batches in which clean and degenerate
sessions alternate (tests/lockstep_cases.py: made from inputs alone, so the oracle and the one-call signer get the same arrays) go
through `mpe_gg20_sign` on the schedule, on each of its parts alone, on the schedule of the round before, and on the default and
large-batch contexts: status, r, s and recid byte-identical to the oracle for EVERY session, R for every session that signs, no
signature bytes for a session that fails.  As every route equals the oracle, the routes equal each other.

(R of a failed session is not compared: sign_finish_kernel copies party 0's R whatever the status, the oracle zeroes it for most
statuses, and include/mpecdsa_hip.h promises nothing about it.)"""
import numpy as np
import pytest
import torch

import fixtures as F
import lockstep_cases as LC
import ossl
from multi_party_ecdsa_amd import engine as E

pytestmark = pytest.mark.gpu

AHEAD = {"merge_r1_quarters": 0}
ROUTES = {
    "ahead": AHEAD,                                                              # inversion ahead, DLog first, PDL ahead, priorities, p | q
    "pdl-ahead-only": {"merge_r1_quarters": 0, "no_r1_inversion_ahead": 1},
    "inversion-ahead-only": {"merge_r1_quarters": 0, "no_pdl_ahead": 1},
    "round5": {"merge_r1_quarters": 0, "no_r1_inversion_ahead": 1, "no_prio": 1, "no_pdl_ahead": 1, "no_crt_n": 1},
    "default": None,                                                             # conftest.gpu_ctx: small-batch defaults, nothing ahead
    "serial": None,                                                              # conftest.gpu_ctx_serial: the large-batch code paths
    "ahead-9-limb-lanes": {"merge_r1_quarters": 0, "xwide_div": "0"},
}
SCHEDULE_OPTIONS = ("no_r1_inversion_ahead", "no_r1_dlog_first", "no_prio", "no_pdl_ahead", "no_crt_n")


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


@pytest.fixture(scope="module")
def table(keys):
    """the batches and the oracle's word on each, once for the whole file"""
    bs = LC.batches(keys)
    for bt in bs.values():
        LC.expected(bt)
    return bs


def _keys_of(ctx, bt):
    t, n, signers = bt.shape
    return E.Gg20Keys(ctx, t, n, signers, bt.lk["arrays"], nkeysets=bt.lk.get("nkeysets", 1))


def _sign(ctx, bt, gk=None, nonces=None, **kw):
    """mpe_gg20_sign over the batch; returns host arrays dict(r, s, recid, status, R)"""
    own = gk is None
    gk = _keys_of(ctx, bt) if own else gk
    dn = nonces if nonces is not None else {f: _dev(ctx, v) for f, v in bt.nonces.items()}
    keyset = None if bt.keyset is None else torch.from_numpy(bt.keyset).to(ctx.device)
    r, s, recid, status, R = E.gg20_sign(ctx, gk, dn, bt.B, want_R=True, keyset=keyset, **{**bt.kw, **kw})
    ctx.sync()
    got = dict(r=_u32(r), s=_u32(s), recid=recid.cpu().numpy(), status=status.cpu().numpy(), R=_u32(R))
    if own:
        gk.close()
    return got


def _compare(got, want, where, sessions=None):
    """got: the signer's arrays over the whole batch; want: the oracle's over `sessions` (default: all of them, in order)"""
    ix = list(range(len(got["status"]))) if sessions is None else list(sessions)
    gst, wst = [int(x) for x in got["status"][ix]], [int(x) for x in want["status"]]
    assert gst == wst, f"{where}: status {gst} != the oracle's {wst}"
    for f in ("r", "s", "recid"):
        diff = [b for j, b in enumerate(ix) if not np.array_equal(got[f][b], want[f][j])]
        assert not diff, f"{where}: {f} differs from the oracle's in sessions {diff} (statuses {[wst[ix.index(b)] for b in diff]})"
    signed = [j for j in range(len(ix)) if wst[j] == 0]
    diff = [ix[j] for j in signed if not np.array_equal(got["R"][ix[j]], want["R"][j])]
    assert not diff, f"{where}: R differs from the oracle's in the signing sessions {diff}"
    failed = [b for j, b in enumerate(ix) if wst[j]]
    assert not got["r"][failed].any() and not got["s"][failed].any() and not got["recid"][failed].any(), f"{where}: a failed session left signature bytes"
    # (a figure, not a check: in how many failed sessions R differs from the oracle's — see the module docstring)
    return sum(1 for j, b in enumerate(ix) if wst[j] and not np.array_equal(got["R"][b], want["R"][j]))


def _same(a, b, where):
    for f in ("status", "r", "s", "recid", "R"):
        assert np.array_equal(a[f], b[f]), f"{where}: {f}"


def _context(request, route):
    """(context, whether this test owns it)"""
    if route == "default":
        return request.getfixturevalue("gpu_ctx"), False
    if route == "serial":
        return request.getfixturevalue("gpu_ctx_serial"), False
    ctx = E.Context(0, options=ROUTES[route])
    for k, v in ROUTES[route].items():
        assert ctx.get_option(k) == int(v), (route, k)
    for k in SCHEDULE_OPTIONS:                                                   # everything the route does not switch off is on
        assert ctx.get_option(k) == int(ROUTES[route].get(k, 0)), (route, k)
    return ctx, True


@pytest.mark.parametrize("route", list(ROUTES))
def test_clean_and_failing_sessions_side_by_side_equal_the_oracle(request, table, route):
    """every batch of the table (each recipe of tests/lockstep_cases.py in a session of its own between clean ones; three signers with a
    91 party and with a ciphertext that is not a unit; dedup_verify; four wallets of which three are unsound in one launch, 602 coming
    after every ladder started ahead was consumed; one chunk of failing sessions only; a batch in which everybody fails; nonces with
    the sampler's given-up draws) on one route of the lock-step signer"""
    ctx, own = _context(request, route)
    try:
        r_differs = {}
        for nm, bt in table.items():
            r_differs[nm] = _compare(_sign(ctx, bt), LC.expected(bt), f"{route} / {nm}")
        print(f"[{route}] failed sessions whose R differs from the oracle's (not asserted):", r_differs)
    finally:
        if own:
            ctx.close()


def test_no_state_computed_ahead_leaks_from_one_chunk_into_the_next(table):
    """chunk = 3 over 11 sessions: a session object is created and released per chunk, the first chunk mixed, the second with failing
    sessions only (status1_kernel marks everybody while the ladders started ahead still run; session_release waits for them), the third
    clean, the last ragged with a failure at its end: the same bytes as the batch in one piece, and the oracle's"""
    bt = table["chunking"]
    assert bt.kw == {"chunk": 3} and bt.B == 11
    ctx = E.Context(0, options=AHEAD)
    try:
        chunked, whole = _sign(ctx, bt), _sign(ctx, bt, chunk=0)
        _compare(chunked, LC.expected(bt), "chunk = 3")
        _compare(whole, LC.expected(bt), "chunk = 0")
        _same(chunked, whole, "chunk = 3 against chunk = 0")
        # another cut: the failing sessions share their chunks with other neighbours
        again = _sign(ctx, bt, chunk=2)
        _same(again, whole, "chunk = 2 against chunk = 0")
    finally:
        ctx.close()


def test_every_chunk_reads_its_own_rows_of_every_nonce_array(gpu_ctx, keys):
    """three signers of four parties — n, S and S - 1 all distinct, so the rows of a session start at another offset in every row
    domain of mpe_gg20_nonces ([B][L], [B][L][n], [B][L][S-1][2], [B][L][S-1], [B]) — five sessions in chunks of two, the last chunk
    partial: r, s, recid and status of every session are the oracle's on the same arrays and those of the batch in one piece (a wrong
    width or domain for any one field hands sessions 2-4 another row's value)"""
    import gg20_fixture as G
    lk = G.make_local_keys(keys, 2, 4, [0, 1, 3], seed="lockstep-strides")
    bt = LC.Batch("strides", lk, G.make_nonces(lk, 5, seed="lockstep-strides"), 5)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(bt.B) as ex:                     # one session per host thread (ctypes releases the GIL), each writes its own row
        rows = list(ex.map(lambda b: G.oracle_sign(lk, bt.nonces, bt.B, first=b, count=1), range(bt.B)))
    wr, ws, wrecid, wstatus = [np.stack([rows[b][j][b] for b in range(bt.B)]) for j in (0, 1, 2, 4)]
    assert not wstatus.any()
    chunked, whole = _sign(gpu_ctx, bt, chunk=2), _sign(gpu_ctx, bt, chunk=0)
    for got, where in ((chunked, "chunk = 2"), (whole, "chunk = 0")):
        for f, want in (("status", wstatus), ("r", wr), ("s", ws), ("recid", wrecid)):
            assert np.array_equal(got[f], want), f"{where}: {f} differs from the oracle's"
    _same(chunked, whole, "chunk = 2 against chunk = 0")


def test_a_context_and_a_key_object_sign_cleanly_after_batches_with_failures(table, keys):
    """one context on the schedule, one key object: a batch with failures, the clean parity case, a batch in which EVERY session fails
    (nobody consumes what was started ahead for a signature), the clean case again — the clean case gives the oracle's bytes each time"""
    mixed, nobody, clean = table["wallet of the clean case"], table["every session fails"], LC.clean_batch(keys)
    assert mixed.shape == nobody.shape == clean.shape and all(np.array_equal(mixed.lk["arrays"][f], clean.lk["arrays"][f]) for f in LC.KEY_FIELDS)
    ctx = E.Context(0, options=AHEAD)
    gk = _keys_of(ctx, clean)
    try:
        want = LC.expected(clean)
        assert not want["status"].any()
        first = None
        for step, bt in enumerate((mixed, clean, nobody, clean, nobody, mixed, clean)):
            got = _sign(ctx, bt, gk=gk)
            _compare(got, LC.expected(bt), f"step {step} ({bt.name})")
            if bt is clean:
                first = first or got
                _same(got, first, f"the clean case at step {step} against its first run")
    finally:
        gk.close()
        ctx.close()


def test_failing_sessions_at_wave_edges_under_the_shipped_thresholds(gpu_ctx, keys):
    """No option: 1 024 sessions (t = 1, n = 3, two signers: BASELINE's config 4) take the schedule by the shipped thresholds.  Sessions
    0, 15, 16, 63, 64, 511, 512 and 1 023 — both sides of lane-group, wave and half-batch edges, and the two ends — are made degenerate
    (k out of range / a ciphertext that is not a unit / a MessageB that is not a unit / delta = 0, in turn); the nonces are the bench's,
    overwritten on the host.  Compared with the oracle: a SAMPLE of 41 sessions — the 8 failing ones, the 8 neighbours they have, and
    every 41st session from 5 on (the sample bounds the oracle's host time, it is no tolerance).  Over all 1 024: the status is 0
    exactly off the 8 sessions, every signature verifies under OpenSSL, no failed session has signature bytes."""
    import bench
    B, (t, n, signers) = LC.FULLSIZE_B, (1, 3, [0, 1])
    import gg20_fixture as G
    lk = G.make_local_keys(keys, t, n, signers)
    gen = torch.Generator(device=gpu_ctx.device)
    gen.manual_seed(4471)
    host = bench._host(bench.make_device_nonces(gen, gpu_ctx.device, B, 2, 2, n))
    where = LC.fullsize_overwrite(lk, host)
    bt = LC.Batch("1024", lk, host, B, recipes=where)
    got = _sign(gpu_ctx, bt)
    pick = LC.fullsize_sample()
    assert len(pick) == 41
    want = LC.oracle(lk, host, B, sessions=pick)
    failing = sorted(where)
    assert [b for j, b in enumerate(pick) if want["status"][j]] == failing and len({int(x) for x in want["status"]}) == 5, list(want["status"])
    _compare(got, want, "1 024 sessions, default context", sessions=pick)
    assert [b for b in range(B) if got["status"][b]] == failing
    ok = ossl.ecdsa_verify(lk["arrays"]["y"][0], host["msg"], got["r"], got["s"], threads=LC.host_threads())
    clean = np.ones(B, dtype=bool)
    clean[failing] = False
    assert ok[clean].all(), f"{int((~ok[clean]).sum())} signatures rejected by OpenSSL"
    assert not ok[failing].any() and not got["r"][failing].any() and not got["s"][failing].any()


def test_nonces_with_given_up_draws_from_the_device_sampler_on_the_schedule(table, keys):
    """sampler_max_attempts = 3 on a context that computes ahead: the device's arrays equal the oracle's expansion of the seed, the
    sessions whose draw gave up answer 91 between sessions that sign — and through the pipeline's seeded form, whose passes call
    mpe_gg20_sign: two tickets coalesced into one pass"""
    import gg20_fixture as G
    import orc
    bt = table["sampled"]
    _, msg, wfails = LC.sampled_batch(keys)
    want = LC.expected(bt)
    assert wfails > 0 and want["status"].any() and not want["status"].all()
    ctx = E.Context(0, options={"merge_r1_quarters": 0, "sampler_max_attempts": LC.SAMPLER_ATTEMPTS})
    assert ctx.get_option("sampler_max_attempts") == LC.SAMPLER_ATTEMPTS and ctx.get_option("merge_r1_quarters") == 0
    gk = _keys_of(ctx, bt)
    try:
        nonces, fail = E.gg20_sample_nonces(ctx, gk, bt.B, LC.SAMPLER_SEED, LC.SAMPLER_COUNTER, msg=_dev(ctx, msg))
        assert int(fail.item()) >= wfails                          # (the device counts a from_modulo item in both of its passes)
        for f in G.NONCE_FIELDS[:-1]:
            assert np.array_equal(_u32(nonces[f]), bt.nonces[f]), f
        _compare(_sign(ctx, bt, gk=gk, nonces=nonces), want, "device-sampled nonces")
        # the pipeline: the same batch and a second one (another batch counter) in one pass
        other = LC.SAMPLER_COUNTER_2
        try:
            orc.lib.orc_sampler_set_max_attempts(LC.SAMPLER_ATTEMPTS)
            z2, _ = G.oracle_sample_nonces(bt.lk, bt.B, LC.SAMPLER_SEED, other, msg=msg)
        finally:
            orc.lib.orc_sampler_set_max_attempts(128)
        want2 = LC.oracle(bt.lk, z2, bt.B)
        assert want2["status"].any() and not want2["status"].all()
        pipe = E.Gg20Pipeline(ctx, gk, bt.B, group=2, lanes=1)
        try:
            tickets = [pipe.submit_seeded(LC.SAMPLER_SEED, c, _dev(ctx, msg), want_R=True) for c in (LC.SAMPLER_COUNTER, other)]
            pipe.flush()
            for tk, w, nm in zip(tickets, (want, want2), ("first", "second")):
                r, s, recid, status, R = pipe.wait(tk, want_R=True)
                _compare(dict(r=_u32(r), s=_u32(s), recid=recid.cpu().numpy(), status=status.cpu().numpy(), R=_u32(R)), w, f"pipeline, {nm} ticket")
            assert pipe.sampler_failures() > 0
        finally:
            pipe.close()
    finally:
        gk.close()
        ctx.close()
