"""Builds the C++ test programs tests/cpp/<name>.cpp, compiled hosts of include/mpecdsa.hpp (the C++ layer above the C-ABI): one g++
recipe, and one rule for handing back the binary `__graft_entry__.build()` left in tests/cpp/ (the compiles are ~40 s of the GPU
suite's budget; the prebuilt binaries travel to the GPU box with the tree)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# program -> does it link the checkers and see their headers: the C/GMP oracle, libgmp and the glue over OpenSSL's ECDSA_do_verify
# (test infrastructure; the product library links none of them)
PROGRAMS = {"test_shim": True, "test_keymint": False, "test_keygen_deal": False}


def recipe(name, exe):
    """(what the program is made of: its source, the two headers, the libraries of this tree it links; the g++ arguments that build it into `exe`)"""
    j = lambda *parts: os.path.join(ROOT, *parts)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src, lib = j("tests", "cpp", name + ".cpp"), j("multi_party_ecdsa_amd", "libmpecdsa_hip.so")
    inc, libs, gmp, rpaths = [j("include")], [lib], [], [os.path.dirname(lib)]
    if PROGRAMS[name]:
        inc += [j("oracle"), "/opt/conda/include"]
        libs += [j("oracle", "libmpe_oracle.so"), j("oracle", "libmpe_ossl.so")]
        gmp = [next(p for p in ("/opt/conda/lib/libgmp.so", "/usr/lib/x86_64-linux-gnu/libgmp.so.10") if os.path.exists(p))]
        rpaths += [j("oracle")]
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__"]
    cmd += [a for i in inc + [os.path.join(rocm, "include")] for a in ("-I", i)] + [src, "-o", exe]
    cmd += libs + gmp + [os.path.join(rocm, "lib", "libamdhip64.so")] + ["-Wl,-rpath," + r for r in rpaths + [os.path.join(rocm, "lib")]]
    return [src, j("include", "mpecdsa.hpp"), j("include", "mpecdsa_hip.h")] + libs, cmd


def prebuilt_is_fresh(pre, deps, out_dir):
    """the prebuilt `pre` stands in for a build into `out_dir`: another directory, everything exists, no dependency is newer than `pre`"""
    return (out_dir != os.path.dirname(pre) and os.path.exists(pre)
            and all(os.path.exists(d) and os.path.getmtime(pre) >= os.path.getmtime(d) for d in deps))


def build(name, out_dir):
    """the path of the program: tests/cpp/<name> when that is fresh, else compiled into `out_dir`"""
    pre, exe = os.path.join(ROOT, "tests", "cpp", name), os.path.join(out_dir, name)
    deps, cmd = recipe(name, exe)
    if prebuilt_is_fresh(pre, deps, out_dir):
        return pre
    subprocess.check_call(cmd)
    return exe
