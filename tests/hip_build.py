"""Builds the test-only device library tests/hip/libec_dev.so from tests/hip/ec_dev.hip (the one-item-per-lane layer behind a batched C
interface, for tests/test_fe_gpu.py): one hipcc recipe -- the product's own flags, imported from __graft_entry__ -- and the rule of
tests/cpp_build.py for handing back the library `__graft_entry__.build()` left beside the source (the compile is ~35 s; the prebuilt
library travels to the GPU box with the tree)."""
import os
import subprocess
import sys

from cpp_build import prebuilt_is_fresh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

NAME = "libec_dev.so"
HEADERS = ["mpe_fe.h", "mpe_sc.h", "mpe_jac.h", "mpe_ec.h", "mpe_small.h"]


def recipe(out):
    """(what the library is made of: its source, the five headers of the layer, the C-ABI header mpe_ec.h takes mpe_encoding from;
    the hipcc arguments that build it into `out`)"""
    j = lambda *parts: os.path.join(ROOT, *parts)
    src = j("tests", "hip", "ec_dev.hip")
    deps = [src] + [j("multi_party_ecdsa_amd", "csrc", h) for h in HEADERS] + [j("include", "mpecdsa_hip.h")]
    return deps, ["hipcc"] + entry.HIPCC_FLAGS + ["-shared", src, "-o", out]


def start(out_dir):
    """(the path the library will have, the running compile or None): tests/hip/libec_dev.so and None when that is fresh, else a hipcc
    process that writes into `out_dir`, for the caller to wait for"""
    pre, out = os.path.join(ROOT, "tests", "hip", NAME), os.path.join(out_dir, NAME)
    deps, cmd = recipe(out)
    if prebuilt_is_fresh(pre, deps, out_dir):
        return pre, None
    os.makedirs(out_dir, exist_ok=True)
    return out, subprocess.Popen(cmd, cwd=ROOT)


def build(out_dir):
    """the path of the library: tests/hip/libec_dev.so when that is fresh, else compiled into `out_dir`"""
    path, proc = start(out_dir)
    if proc is not None and proc.wait() != 0:
        raise RuntimeError("hipcc failed on tests/hip/ec_dev.hip")
    return path
