"""The GG20 message layout is stated once for the round engine (csrc/mpe_gg20_msg.h) and once for the host glue (wire.py RECORDS):
tests/cpp/test_gg20_layout.cpp, compiled with `hipcc --cuda-host-only` against the library's own header, dumps the first; it must equal
the second, the table include/mpecdsa_hip.h documents (written out below: the pin from outside), and the widths the library reports.
The same program sizes every round's scratch from what the round takes: never more than the hand-written bound it replaced.
The arrays of mpe_gg20_nonces are held the same way: csrc/mpe_gg20_nonces.h (dumped by the same program), wire.NONCE_FIELDS and the pin
written out below from the comment above the struct in include/mpecdsa_hip.h.  No GPU."""
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

# include/mpecdsa_hip.h, the comment above mpe_gg20_nonces: (field, row domain, words) in declaration order.
# Rows: PI [B][L], AP [B][L][n], MB [B][L][S-1][2], PP [B][L][S-1], B [B]
EXPECTED_NONCES = [
    ("k", "PI", 8), ("gamma", "PI", 8), ("blind", "PI", 8), ("r_a", "PI", 64),
    ("al_alpha", "AP", 24), ("al_beta", "AP", 64), ("al_gamma", "AP", 88), ("al_rho", "AP", 72),
    ("mb_beta_tag", "MB", 64), ("mb_r", "MB", 64), ("mb_nonce_b", "MB", 8), ("mb_nonce_bt", "MB", 8),
    ("l", "PI", 8), ("ped_s1", "PI", 8), ("ped_s2", "PI", 8),
    ("pdl_alpha", "PP", 24), ("pdl_beta", "PP", 64), ("pdl_rho", "PP", 72), ("pdl_gamma", "PP", 88),
    ("heg_s1", "PI", 8), ("heg_s2", "PI", 8), ("msg", "B", 8),
]
NONCE_SHAPES = [(2, 3, 1, 1), (2, 3, 2, 1), (3, 5, 3, 4), (3, 4, 2, 5), (6, 8, 6, 3), (2, 3, 2, 0)]          # (S, n, L, B)


@pytest.fixture(scope="module")
def dump_lines(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("layout") / "test_gg20_layout")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_gg20_layout.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr
    return [line.split() for line in out.stdout.splitlines()]


@pytest.fixture(scope="module")
def dump(dump_lines):
    records, widths, tmp = {}, {}, []
    for kind, *v in dump_lines:
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


@pytest.fixture(scope="module")
def nonce_dump(dump_lines):
    """(the table [(name, domain, words)] by index, {shape: [(name, rows, blob word offset)]})"""
    table = [(int(v[0]), v[1], v[2], int(v[3])) for kind, *v in dump_lines if kind == "nonce"]
    assert [i for i, *_ in table] == list(range(len(table)))
    rows = {}
    for kind, *v in dump_lines:
        if kind == "nonce_rows":
            rows.setdefault(tuple(int(x) for x in v[:4]), []).append((v[4], int(v[5]), int(v[6])))
    return [t[1:] for t in table], rows


def test_the_header_and_wire_py_state_the_same_nonce_arrays(nonce_dump):
    assert nonce_dump[0] == list(G.wire.NONCE_FIELDS)


def test_the_header_states_the_documented_nonce_arrays(nonce_dump):
    assert len(EXPECTED_NONCES) == 22 and nonce_dump[0] == EXPECTED_NONCES


def test_nonce_rows_and_blob_offsets_are_those_of_the_engine_and_of_the_allocation(nonce_dump):
    """rows: engine.gg20_nonce_shapes and the pinned domains; offsets: the running sum mpe_gg20_nonces_alloc has always made, every
    field's rows x words rounded up to 64 words"""
    from multi_party_ecdsa_amd import engine as E
    assert list(nonce_dump[1]) == NONCE_SHAPES
    for (S, n, L, B), got in nonce_dump[1].items():
        shapes = E.gg20_nonce_shapes(S, n, L, B)
        assert list(shapes) == [f for f, _, _ in EXPECTED_NONCES]
        per = dict(PI=B * L, AP=B * L * n, MB=B * L * (S - 1) * 2, PP=B * L * (S - 1), B=B)
        off = 0
        for (f, dom, words), (name, rows, blob_off) in zip(EXPECTED_NONCES, got):
            assert (name, rows, blob_off) == (f, per[dom], off) and shapes[f] == (rows, words), (S, n, L, B, f)
            off += (rows * words + 63) & ~63
