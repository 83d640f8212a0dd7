"""The bookkeeping of the context workspace (csrc/mpe_ws.h: chained blocks that settle into one, WsKeep, WsHold, the sticky failure flag)
checked on the host over a malloc device: tests/cpp/test_ws_arena.cpp is compiled with `hipcc --cuda-host-only` against the library's own
header and run here, once plain and once as a stand-alone executable under the address and undefined-behaviour sanitizers; no GPU
involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ws_arena.cpp")
HIPCC = ["hipcc", "--cuda-host-only", "-std=c++17", "-O1"]

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_workspace_arena_chains_settles_keeps_holds_and_reports_failure(tmp_path):
    exe = str(tmp_path / "test_ws_arena")
    subprocess.check_call(HIPCC + ["-o", exe, SRC])
    run(exe)


def test_workspace_arena_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "test_ws_arena_san")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"]
    subprocess.check_call(HIPCC + san + ["-c", "-o", exe + ".o", SRC])          # a compile error is a failure, never a skip
    linked = subprocess.run(HIPCC + san + ["-o", exe, exe + ".o"], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the sanitizer runtime failed to link on this machine: " + (linked.stderr.strip().splitlines() or ["?"])[-1])
    run(exe)
