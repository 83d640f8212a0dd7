"""GPU: tests/cpp/test_keygen_deal.cpp — one (t = 1, n = 3) wallet dealt, constructed and confirmed through include/mpecdsa.hpp
(`VerifiableSS::share`, both halves of `phase2_verify_vss_construct_keypair_phase3_pok_dlog`, `Keys::verify_dlog_proofs_check_against_vss`)
with one tampered share and one tampered proof.  Built by tests/cpp_build.py, or taken prebuilt from `__graft_entry__.build()` when
that binary is newer than what it is made of."""
import subprocess

import pytest

import cpp_build

pytestmark = pytest.mark.gpu


def test_cpp_host_layer_deals_constructs_and_confirms_a_wallet(tmp_path):
    exe = cpp_build.build("test_keygen_deal", str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "keygen deal ok: 1 wallet" in out.stdout
