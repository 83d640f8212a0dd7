"""CPU tests of the sealed records' C boundary: the header's typed constants as a C compiler sees them equal the names _native.py
and tests/pyref_seal.py use, and every new entry point refuses NULL handles before any HIP call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sealed_record_constants_are_what_a_c_compiler_sees(tmp_path):
    import pyref_seal as PS
    from multi_party_ecdsa_amd import _native as N
    names = ["MPE_SEAL_MAGIC", "MPE_SEAL_REFUSED", "MPE_SEAL_MAX_WORDS", "MPE_SEAL_KIND_PRESIG", "MPE_SEAL_KIND_KEYSHARE", "MPE_SEAL_KIND_USER",
             "MPE_GG20_KEYSHARE_WORDS"]
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "mpecdsa_hip.h"\nint main(void) {\n'
                   + "\n".join(f'  printf("{n} %lld\\n", (long long){n});' for n in names)
                   + '\n  unsigned m = MPE_SEAL_MAGIC; char b[5] = {0}; memcpy(b, &m, 4); printf("bytes %s\\n", b);\n  return 0;\n}\n')
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert seen.pop("bytes") == "MPS1"
    assert {k: int(v) for k, v in seen.items()} == {n: getattr(N, n[len("MPE_"):]) for n in names}
    assert (PS.MAGIC, PS.REFUSED, PS.MAX_WORDS, PS.KIND_PRESIG, PS.KIND_KEYSHARE, PS.KIND_USER) == \
        (N.SEAL_MAGIC, N.SEAL_REFUSED, N.SEAL_MAX_WORDS, N.SEAL_KIND_PRESIG, N.SEAL_KIND_KEYSHARE, N.SEAL_KIND_USER)
    assert PS.EXTRA == 10 and N.GG20_KEYSHARE_WORDS == 8 + 32 + 32


def test_argument_errors_without_gpu():
    from multi_party_ecdsa_amd import _native as N
    L = N.lib
    assert L.mpe_wrap_key_create(None, b"\x00" * 32, None) == N.MPE_E_ARG and L.mpe_wrap_key_destroy(None) == N.MPE_E_ARG
    assert L.mpe_seal(None, None, 16, 1, 1, None, 0, None, None) == N.MPE_E_ARG
    assert L.mpe_unseal(None, None, 16, 1, 1, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_poly1305(None, 1, None, None, 16, None, None) == N.MPE_E_ARG
    assert L.mpe_gg20_sealed_presig_words(None) == N.MPE_E_ARG
    assert L.mpe_gg20_sealed_presig_export(None, None, 1, None, 0, None, None, None) == N.MPE_E_ARG
    assert L.mpe_gg20_sealed_presig_import(None, None, 1, None, None, None, None) == N.MPE_E_ARG
    assert L.mpe_gg20_keyshare_seal(None, None, 1, None, None, None, 0, None, None) == N.MPE_E_ARG
    assert L.mpe_gg20_keys_create_sealed(None, 1, 3, 2, 1, None, 1, 3, None, None, None, None, None, None, None, None, None, None, None) == N.MPE_E_ARG
