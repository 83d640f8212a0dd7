"""GPU: tests/cpp/test_keymint.cpp — key pairs minted through include/mpecdsa.hpp (`Paillier::keypair`, `generate_h1_h2_N_tilde`) and
an encrypt / decrypt round trip under them.  Built by tests/cpp_build.py, or taken prebuilt from `__graft_entry__.build()`
when that binary is newer than what it is made of."""
import subprocess

import pytest

import cpp_build

pytestmark = pytest.mark.gpu


def test_cpp_host_layer_mints_keys_and_round_trips(tmp_path):
    exe = cpp_build.build("test_keymint", str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "keymint ok: 3 key pairs" in out.stdout
