"""The GG20 message layout is stated once for the round engine (csrc/mpe_gg20_msg.h) and once for the host glue (wire.py RECORDS):
tests/cpp/test_gg20_layout.cpp, compiled with `hipcc --cuda-host-only` against the library's own header, dumps the first; it must equal
the second, the table include/mpecdsa_hip.h documents (written out below: the pin from outside), and the widths the library reports.
The same program sizes every round's scratch from what the round takes: never more than the hand-written bound it replaced.  No GPU."""
import os
import shutil
import subprocess

import pytest

import gg20_fixture as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/mpecdsa_hip.h, "GG20 round messages": (field, offset, words); points 16 words, scalars 8, Paillier ciphertexts 128
EXPECTED = {
    "M0A": [("z", 0, 64), ("e", 64, 8), ("s", 72, 64), ("s1", 136, 25), ("s2", 161, 89)],
    "M0L": [("c", 0, 128), ("com", 128, 8)],
    "M1": [("c", 0, 128), ("b_pk", 128, 16), ("b_R", 144, 16), ("b_z", 160, 8), ("bt_pk", 168, 16), ("bt_R", 184, 16), ("bt_z", 200, 8)],
    "M2": [("delta", 0, 8), ("T", 8, 16), ("e", 24, 8), ("a1", 32, 16), ("a2", 48, 16), ("com", 64, 16), ("z1", 80, 8), ("z2", 88, 8)],
    "M3": [("blind", 0, 8), ("g_gamma", 8, 16)],
    "M4P": [("z", 0, 64), ("u1", 64, 16), ("u2", 80, 128), ("u3", 208, 64), ("s1", 272, 25), ("s2", 297, 64), ("s3", 361, 89)],
    "M4R": [("R_dash", 0, 16)],
    "M5": [("S", 0, 16), ("T", 16, 16), ("A3", 32, 16), ("z1", 48, 8), ("z2", 56, 8)],
    "M7": [("s_i", 0, 8)],
}
EXPECTED_WIDTHS = dict(SUB0=256, SUB1=208, W2=96, W3=24, SUB4=450, W5=64, W6=8)
SHAPES = [(1, 2, 3, 1, 2, 1), (1, 2, 3, 2, 2, 2), (4, 3, 5, 3, 2, 3), (24, 2, 3, 2, 1, 1), (1024, 2, 3, 2, 2, 2), (3, 6, 8, 6, 2, 6), (0, 2, 3, 2, 2, 2)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("layout") / "test_gg20_layout")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_gg20_layout.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr
    records, widths, tmp = {}, {}, []
    for line in out.stdout.splitlines():
        kind, *v = line.split()
        if kind == "field":
            records.setdefault(v[0], []).append((v[1], int(v[2]), int(v[3])))
        elif kind == "width":
            widths[v[0]] = int(v[1])
        elif kind == "tmp":
            tmp.append(tuple(int(x) for x in v))
    return records, widths, tmp


def test_the_header_and_wire_py_state_the_same_records(dump):
    records, widths, _ = dump
    assert records == {r: list(f) for r, f in G.wire.RECORDS.items()}
    assert widths == G.wire.WIDTHS


def test_the_header_states_the_documented_layout(dump):
    records, widths, _ = dump
    assert records == EXPECTED
    assert widths == EXPECTED_WIDTHS


def test_the_widths_of_the_table_are_what_the_library_reports():
    from multi_party_ecdsa_amd import _native as N          # loads without a GPU
    for S, n in ((2, 3), (3, 5), (6, 8)):
        for rnd in range(8):
            want = G.wire.msg_words(S, n, rnd) if rnd in G.ROUNDS else 0
            assert N.lib.mpe_gg20_msg_words(S, n, rnd) == want, (S, n, rnd)


def test_round_scratch_is_sized_from_what_the_rounds_take_and_never_grows(dump):
    tmp = dump[2]
    assert [t[:6] for t in tmp] == SHAPES
    for *shape, total, r0, r1, r2, r4, r5, earlier in tmp:
        print(shape, "tmp_bytes_of", total, "takes", (r0, r1, r2, r4, r5), "earlier bound", earlier)
        assert max(r0, r1, r2, r4, r5) <= total <= earlier, shape
