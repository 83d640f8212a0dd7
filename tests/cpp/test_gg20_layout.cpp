// Host-only dump of the GG20 message layout and the per-round scratch sizing (multi_party_ecdsa_amd/csrc/mpe_gg20_msg.h), for
// tests/test_gg20_layout_cpu.py: every record as `field <record> <name> <offset> <words>` lines, the widths as `width <name> <words>`,
// and for a few batch shapes `tmp <B S n L V PV> <tmp_bytes_of> <take of rounds 0 1 2 4 5> <the earlier hand-written bound>`.
// The arrays of mpe_gg20_nonces (mpe_gg20_nonces.h) follow: `nonce <index> <name> <domain> <words>` per field, and for a few shapes
// `nonce_rows <S n L B> <name> <rows> <word offset in the blob of mpe_gg20_nonces_alloc>`.
// Built with `hipcc --cuda-host-only` (no GPU needed).
#include <cstdio>

#include "../../multi_party_ecdsa_amd/csrc/mpe_gg20_msg.h"
#include "../../multi_party_ecdsa_amd/csrc/mpe_gg20_nonces.h"

using namespace mpe::gg;

template <int N>
static void dump(const char* record, const NamedField (&fields)[N]) {
  for (const NamedField& f : fields) std::printf("field %s %s %d %d\n", record, f.name, f.f.off, f.f.words);
}

// tmp_bytes_of as commit ac15f6c ("One build recipe for the library and its C++ test programs") wrote it out by hand: the bound the
// session footprint must not exceed
static size_t earlier_tmp_bytes_of(const Counts& c) {
  const size_t r0 = c.nAP * 250 * 4 + 4096;
  const size_t r1 = c.nVI * 5 + c.nMB * (8 + 8 + 128 + 16 + 16 + 8 + 16 + 16 + 8) * 4 + 8192;
  const size_t r2 = c.nMB * (1 + 64 + 8) * 4 + c.nMB + c.nPI * 72 * 4 + 8192;
  const size_t r4 = c.nPP * 450 * 4 + 4096;
  const size_t r5 = c.nPV * 9 + c.nPI * 64 * 4 + 8192;
  size_t m = r0;
  if (r1 > m) m = r1;
  if (r2 > m) m = r2;
  if (r4 > m) m = r4;
  if (r5 > m) m = r5;
  return m + 64 * 256;
}

int main() {
  dump("M0A", M0A_FIELDS); dump("M0L", M0L_FIELDS); dump("M1", M1_FIELDS); dump("M2", M2_FIELDS); dump("M3", M3_FIELDS);
  dump("M4P", M4P_FIELDS); dump("M4R", M4R_FIELDS); dump("M5", M5_FIELDS); dump("M7", M7_FIELDS);
  std::printf("width SUB0 %d\nwidth SUB1 %d\nwidth W2 %d\nwidth W3 %d\nwidth SUB4 %d\nwidth W5 %d\nwidth W6 %d\n", SUB0, SUB1, W2, W3, SUB4, W5, W6);
  const int shapes[][6] = {{1, 2, 3, 1, 2, 1}, {1, 2, 3, 2, 2, 2}, {4, 3, 5, 3, 2, 3}, {24, 2, 3, 2, 1, 1}, {1024, 2, 3, 2, 2, 2}, {3, 6, 8, 6, 2, 6},
                           {0, 2, 3, 2, 2, 2}};
  int bad = 0;
  for (const auto& s : shapes) {
    const Counts c = counts_of(s[0], s[1], s[2], s[3], s[4], s[5]);
    const size_t total = tmp_bytes_of(c), earlier = earlier_tmp_bytes_of(c);
    const size_t take[5] = {tmp_take<Round0Tmp>(c), tmp_take<Round1Tmp>(c), tmp_take<Round2Tmp>(c), tmp_take<Round4Tmp>(c), tmp_take<Round5Tmp>(c)};
    std::printf("tmp %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu\n", s[0], s[1], s[2], s[3], s[4], s[5], total, take[0], take[1], take[2], take[3],
                take[4], earlier);
    for (const size_t t : take) bad += t > total;
    bad += total > earlier;
  }
  for (int f = 0; f < NF; ++f) std::printf("nonce %d %s %s %d\n", f, NONCE_FIELDS[f].name, DOM_NAMES[(int)NONCE_FIELDS[f].dom], NONCE_FIELDS[f].words);
  const int nonce_shapes[][4] = {{2, 3, 1, 1}, {2, 3, 2, 1}, {3, 5, 3, 4}, {3, 4, 2, 5}, {6, 8, 6, 3}, {2, 3, 2, 0}};      // S n L B
  for (const auto& s : nonce_shapes) {
    const NonceBlob blob = nonce_blob(s[0], s[1], s[2], s[3]);
    for (int f = 0; f < NF; ++f)
      std::printf("nonce_rows %d %d %d %d %s %zu %zu\n", s[0], s[1], s[2], s[3], NONCE_FIELDS[f].name, nonce_rows(NONCE_FIELDS[f].dom, s[0], s[1], s[2], s[3]),
                  blob.off[f]);
  }
  if (bad) { std::printf("FAILED %d scratch bounds\n", bad); return 1; }
  std::printf("OK\n");
  return 0;
}
