"""GPU: tests/cpp/test_keymint.cpp — key pairs minted through include/mpecdsa.hpp (`Paillier::keypair`, `generate_h1_h2_N_tilde`) and
an encrypt / decrypt round trip under them.  Built with the flags of tests/cpp_shim.py (whose helper builds tests/cpp/test_shim.cpp
only), or taken prebuilt from `__graft_entry__.build()` when that binary is newer than what it is made of."""
import os
import subprocess

import pytest

import cpp_shim

pytestmark = pytest.mark.gpu


def build_keymint(out_dir):
    root = cpp_shim.ROOT
    lib = os.path.join(root, "multi_party_ecdsa_amd", "libmpecdsa_hip.so")
    src = os.path.join(root, "tests", "cpp", "test_keymint.cpp")
    deps = [src, os.path.join(root, "include", "mpecdsa.hpp"), os.path.join(root, "include", "mpecdsa_hip.h"), lib]
    pre = os.path.join(root, "tests", "cpp", "test_keymint")
    if out_dir != os.path.dirname(pre) and os.path.exists(pre) and all(os.path.getmtime(pre) >= os.path.getmtime(d) for d in deps):
        return pre
    exe = os.path.join(out_dir, "test_keymint")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(rocm, "include"), src, "-o", exe, lib, os.path.join(rocm, "lib", "libamdhip64.so"),
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    return exe


def test_cpp_host_layer_mints_keys_and_round_trips(tmp_path):
    exe = build_keymint(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "keymint ok: 3 key pairs" in out.stdout
