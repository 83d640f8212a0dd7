"""GPU: tests/cpp/test_keygen_deal.cpp — one (t = 1, n = 3) wallet dealt, constructed and confirmed through include/mpecdsa.hpp
(`VerifiableSS::share`, both halves of `phase2_verify_vss_construct_keypair_phase3_pok_dlog`, `Keys::verify_dlog_proofs_check_against_vss`)
with one tampered share and one tampered proof.  Built with the flags of tests/test_keymint_gpu.py, or taken prebuilt from
`__graft_entry__.build()` when that binary is newer than what it is made of."""
import os
import subprocess

import pytest

import cpp_shim

pytestmark = pytest.mark.gpu


def build_keygen_deal(out_dir):
    root = cpp_shim.ROOT
    lib = os.path.join(root, "multi_party_ecdsa_amd", "libmpecdsa_hip.so")
    src = os.path.join(root, "tests", "cpp", "test_keygen_deal.cpp")
    deps = [src, os.path.join(root, "include", "mpecdsa.hpp"), os.path.join(root, "include", "mpecdsa_hip.h"), lib]
    pre = os.path.join(root, "tests", "cpp", "test_keygen_deal")
    if out_dir != os.path.dirname(pre) and os.path.exists(pre) and all(os.path.getmtime(pre) >= os.path.getmtime(d) for d in deps):
        return pre
    exe = os.path.join(out_dir, "test_keygen_deal")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(rocm, "include"), src, "-o", exe, lib, os.path.join(rocm, "lib", "libamdhip64.so"),
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    return exe


def test_cpp_host_layer_deals_constructs_and_confirms_a_wallet(tmp_path):
    exe = build_keygen_deal(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "keygen deal ok: 1 wallet" in out.stdout
