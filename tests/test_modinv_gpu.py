"""The batched route of `mpe_modinv` (multi_party_ecdsa_amd/csrc/mpe_modinv.h: counting sort by modulus, up-sweep, one
wave-cooperative gcd per chunk, down-sweep, masked lane-kernel fallback) against the GMP oracle on the case table of
tests/modinv_cases.py: `ok` byte-equal and `out` word-equal on every row, failed rows all-zero.  Exact equality, no tolerance.
(tests/test_modinv_cases_cpu.py proves the table reaches what it is named for; the lane-serial route is
tests/test_proofs_gpu.py::test_modinv_vs_oracle.)"""
import numpy as np
import pytest
import torch

import modinv_cases as MC

pytestmark = pytest.mark.gpu
CASES = [(bits, nm) for bits in MC.BITS for nm in MC.NAMES]
IDS = [f"{bits}-{nm}" for bits, nm in CASES]


def E():
    from multi_party_ecdsa_amd import engine
    return engine


def npw(t):
    return np.ascontiguousarray(t.cpu().numpy().view(np.uint32))


def to_dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


@pytest.fixture(scope="module")
def two_trip_ctx():
    """a context of its own: the option caps the sweep kernels' grid at one wave per compute unit"""
    return E().Context(0, options=MC.TWO_TRIP_OPTIONS)


def run(ctx, case):
    """one launch: (out words, ok bytes) on the host, plus the device tensors for further checks"""
    e = E()
    mw, aw = case.words()
    ms = e.ModSet(ctx, case.bits, to_dev(ctx, mw))
    d_a = to_dev(ctx, aw)
    d_idx = None if case.mod_idx is None else torch.tensor(case.mod_idx, dtype=torch.int32, device=ctx.device)
    out, ok = e.modinv_device(ctx, ms, d_a, d_idx)
    ctx.sync()
    return npw(out), ok.cpu().numpy(), (ms, d_a, d_idx, out, ok)


def compare(case, out, ok, what=""):
    w_out, w_ok = case.expected()
    bad = np.flatnonzero((ok != w_ok) | (out != w_out).any(axis=1))
    if bad.size:
        geo = case.geometry
        lines = []
        for i in bad[:8].tolist():
            m, ch, pos = geo.where[i]
            words = np.flatnonzero(out[i] != w_out[i])
            lines.append(f"  row {i}: modulus {m}, chunk {ch} (of {len(geo.chunks[ch][1])} items), position {pos}; ok {int(ok[i])} want "
                         f"{int(w_ok[i])}; {words.size} wrong words" + (f", first at word {int(words[0])}" if words.size else ""))
        pytest.fail(f"{case.bits}-bit case '{case.name}'{what}: {bad.size} of {case.B} rows differ from the oracle "
                    f"(chunks of {case.chunk}, launch-order geometry)\n" + "\n".join(lines))
    assert not out[ok == 0].any(), f"{case.name}{what}: a failed row is not all-zero"


@pytest.mark.parametrize("bits,name", CASES, ids=IDS)
def test_batched_modinv_vs_oracle(gpu_ctx, two_trip_ctx, bits, name):
    case = MC.case(bits, name)
    ctx = two_trip_ctx if case.options else gpu_ctx
    if case.options:
        # the case needs two trips on THIS device: more chunks than the capped grid has lane groups
        cap = MC.trip_capacity(bits, ctx.get_option("waves_per_cu"), torch.cuda.get_device_properties(0).multi_processor_count)
        assert ctx is not gpu_ctx and cap < len(case.geometry.chunks) <= MC.max_chunks(case.B, case.count) <= 2 * cap
    out, ok, _ = run(ctx, case)
    compare(case, out, ok)


@pytest.mark.parametrize("bits", MC.BITS)
def test_stale_workspace_changes_nothing(gpu_ctx, bits):
    """the geometry case, a smaller launch, the geometry case again on ONE context: the second run finds the first one's chunk
    table, prefix products and fallback mask in the workspace and must give the first run's answers"""
    big, small = MC.case(bits, "geometry"), MC.case(bits, "non-units, one modulus")
    first = run(gpu_ctx, big)
    compare(big, *first[:2], what=" (first run)")
    mid = run(gpu_ctx, small)
    compare(small, *mid[:2], what=" (after the geometry case)")
    again = run(gpu_ctx, big)
    compare(big, *again[:2], what=" (on stale workspace)")
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


@pytest.mark.parametrize("bits", MC.BITS)
def test_bulk_inverses_multiply_to_one_on_the_device(gpu_ctx, bits):
    """independent of the oracle: a * out mod n == 1 on every ok row of the 64-item-chunk case (`mpe_modmul`), 0 on the others"""
    case = MC.case(bits, "64-item chunks")
    out, ok, (ms, d_a, d_idx, d_out, d_ok) = run(gpu_ctx, case)
    prod = E().modmul_device(gpu_ctx, ms, d_a, d_out, d_mod_idx=d_idx)
    gpu_ctx.sync()
    one = torch.zeros_like(prod)
    one[:, 0] = 1
    one[d_ok == 0] = 0
    wrong = torch.nonzero((prod != one).any(dim=1)).flatten().cpu().tolist()
    assert not wrong, f"a * a^-1 != 1 on rows {wrong[:8]} ({len(wrong)} in all): " + str([case.geometry.where[i] for i in wrong[:8]])
    assert set(np.flatnonzero(ok == 0).tolist()) == set(case.planted)
