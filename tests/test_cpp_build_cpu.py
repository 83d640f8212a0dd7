"""Without a GPU, without a compiler: tests/cpp_build.py — when a prebuilt C++ test program is handed back (temporary files), and the
g++ arguments and dependencies of the three programs (written out: those of the three builders the helper replaced); and the same for
tests/hip_build.py, the recipe of the test-only device library tests/hip/libec_dev.so."""
import os
from collections import Counter

import pytest

import cpp_build
import hip_build


@pytest.mark.parametrize("case, want", [("prebuilt newest", True), ("same age", True), ("dependency newer", False), ("dependency missing", False),
                                        ("prebuilt missing", False), ("out_dir is the prebuilt's directory", False)])
def test_prebuilt_is_handed_back_only_when_fresh(tmp_path, case, want):
    pre, deps = str(tmp_path / "cpp" / "prog"), [str(tmp_path / n) for n in ("prog.cpp", "layer.hpp", "lib.so")]
    os.mkdir(os.path.dirname(pre))
    for p in [pre] + deps:
        open(p, "w").close()
        os.utime(p, (100, 100) if p != pre and case != "same age" else (200, 200))
    if case == "dependency newer":
        os.utime(deps[1], (201, 201))
    if case.endswith("missing"):
        os.remove(pre if case == "prebuilt missing" else deps[2])
    out_dir = os.path.dirname(pre) if case.startswith("out_dir") else str(tmp_path / "out")
    assert cpp_build.prebuilt_is_fresh(pre, deps, out_dir) is want           # and no exception: the copied builders raised on a missing file


@pytest.mark.parametrize("name", ["test_shim", "test_keymint", "test_keygen_deal"])
def test_gxx_arguments_and_dependencies_are_those_of_the_replaced_builders(name, tmp_path):
    j = lambda *parts: os.path.join(cpp_build.ROOT, *parts)
    rocm, exe = os.environ.get("ROCM_PATH", "/opt/rocm"), str(tmp_path / name)
    src, lib, hip = j("tests", "cpp", name + ".cpp"), j("multi_party_ecdsa_amd", "libmpecdsa_hip.so"), rocm + "/lib/libamdhip64.so"
    std = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__"]
    if name == "test_shim":
        orc, ossl = j("oracle", "libmpe_oracle.so"), j("oracle", "libmpe_ossl.so")
        gmp = next(p for p in ("/opt/conda/lib/libgmp.so", "/usr/lib/x86_64-linux-gnu/libgmp.so.10") if os.path.exists(p))
        want = std + ["-I", j("include"), "-I", j("oracle"), "-I", "/opt/conda/include", "-I", rocm + "/include", src, "-o", exe, lib, orc, ossl, gmp, hip,
                      "-Wl,-rpath," + j("multi_party_ecdsa_amd"), "-Wl,-rpath," + j("oracle"), "-Wl,-rpath," + rocm + "/lib"]
        want_deps = [src, j("include", "mpecdsa.hpp"), j("include", "mpecdsa_hip.h"), lib, orc, ossl]
    else:
        want = std + ["-I", j("include"), "-I", rocm + "/include", src, "-o", exe, lib, hip,
                      "-Wl,-rpath," + j("multi_party_ecdsa_amd"), "-Wl,-rpath," + rocm + "/lib"]
        want_deps = [src, j("include", "mpecdsa.hpp"), j("include", "mpecdsa_hip.h"), lib]
    deps, cmd = cpp_build.recipe(name, exe)
    assert Counter(cmd) == Counter(want) and cmd[0] == "g++" and deps == want_deps


def test_device_test_library_is_compiled_with_the_flags_of_the_product(tmp_path, monkeypatch):
    import __graft_entry__ as entry
    j = lambda *parts: os.path.join(hip_build.ROOT, *parts)
    out, src = str(tmp_path / "libec_dev.so"), j("tests", "hip", "ec_dev.hip")
    deps, cmd = hip_build.recipe(out)
    assert cmd == ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out]
    assert deps == [src] + [j("multi_party_ecdsa_amd", "csrc", h) for h in ("mpe_fe.h", "mpe_sc.h", "mpe_jac.h", "mpe_ec.h", "mpe_small.h")] + [j("include", "mpecdsa_hip.h")]
    assert all(os.path.exists(d) for d in deps)
    monkeypatch.setattr(entry, "HIPCC_FLAGS", ["--offload-arch=gfx950", "-O1"])        # taken from __graft_entry__, not restated
    assert hip_build.recipe(out)[1] == ["hipcc", "--offload-arch=gfx950", "-O1", "-shared", src, "-o", out]
    # the library stays out of build/, which does not travel with the tree, and out of git
    assert os.path.dirname(src) == j("tests", "hip") and hip_build.NAME.endswith(".so")
