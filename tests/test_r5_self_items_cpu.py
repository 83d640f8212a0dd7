"""Which of round 5's PDL verification items are a verifier's own proofs is decided by index arithmetic alone
(multi_party_ecdsa_amd/csrc/mpe_gg20_pv.h: g -> (b, vl, i, jj), self <=> the verifier's ordinal equals i, B L (S-1) of them).
tests/cpp/test_r5_self_items.cpp, compiled with `hipcc --cuda-host-only` against the library's own header, checks it against a
brute-force loop for S in {2, 3, 4}, L in {1, S}, local parties by slot and by party index under per-session signer sets.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("r5_self") / "test_r5_self_items")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_r5_self_items.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr
    return [line.split() for line in out.stdout.splitlines()]


def test_self_items_are_found_and_counted_like_the_brute_force_loop(lines):
    cases = [dict(zip(v[2::2], (int(x) for x in v[3::2])), what=v[1]) for v in lines if v[0] == "case"]
    # per S: all local, S times one by slot, one by party index
    assert [c["what"] for c in cases] == sum((["all_local"] + ["one_by_slot"] * S + ["one_by_party_index"] for S in (2, 3, 4)), [])
    for c in cases:
        assert c["bad"] == 0, c
        assert c["items"] == c["B"] * c["L"] * c["S"] * (c["S"] - 1) and c["self"] == c["B"] * c["L"] * (c["S"] - 1), c
