"""-m gpu: bench.py as every change runs it — a plain run (set-up, warm-up, the timed steps, one line with nothing measured after
the timed region) and --dump-outputs: the last timed step's signatures, identical from run to run with the same arguments and
valid under OpenSSL for the messages the run signed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_SESSIONS, STEPS = 64, 2


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--sessions", str(B_SESSIONS), "--steps", str(STEPS),
           "--warmup", "1", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_its_dumped_outputs(tmp_path):
    import bench
    import fixtures as F
    import gg20_fixture as G
    import ossl
    runs = [(_plain_run(tmp_path / d), tmp_path / d) for d in ("a", "b")]
    for rec, _ in runs:
        assert rec["full"] is False and rec["steps"] == STEPS and rec["all_sessions_signed"] is True
        assert abs(rec["value"] - B_SESSIONS / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
        assert rec["unit"] == "signatures/s" and rec["higher_is_better"] is True
        assert not {"configs", "cpu_baseline", "openssl", "host_handover", "paillier", "parity_vs_oracle_on_sample"} & set(rec)
    (_, a), (_, b) = runs
    names = ["r.npy", "recid.npy", "s.npy", "status.npy"]
    assert sorted(os.listdir(a)) == names == sorted(os.listdir(b))
    for n in names:
        x = np.load(a / n)
        assert x.dtype == np.float64 and x.shape[0] == B_SESSIONS and np.array_equal(x, np.load(b / n))
    assert not np.load(a / "status.npy").any()
    # the messages of the run: the first draw of bench.py's device generator (seed 4242 on rank 0)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(4242)
    msg = bench.rand_words(gen, torch.device("cuda:0"), B_SESSIONS, 8, 8).cpu().numpy().view(np.uint32)
    lk = G.make_local_keys(F.load_keys(), 1, 3, [0, 1])
    u32 = lambda n: np.load(a / n).astype(np.uint32)
    assert ossl.ecdsa_verify(lk["arrays"]["y"][0], msg, u32("r.npy"), u32("s.npy")).all()
