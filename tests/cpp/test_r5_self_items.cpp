// Host-only check of the index arithmetic that picks a verifier's OWN proofs among round 5's PDL verification items
// (multi_party_ecdsa_amd/csrc/mpe_gg20_pv.h), for tests/test_r5_self_items_cpu.py.  Against a brute-force loop over every
// (session, local verifier, prover, proof): pv_item inverts pv_index, an item is a self item iff the prover's ordinal is the
// verifier's, pv_self_item / pv_rest_item list exactly those two classes, each item once, B L (S-1) and B L (S-1)^2 of them — for
// S in {2, 3, 4}, L in {1, S}, with the local parties named by slot and (L = 1) by party index under per-session signer sets, where
// the verifier's ordinal is its rank in the session's own set (rank_in).
// Built with `hipcc --cuda-host-only` (no GPU needed); prints one `case ...` line per shape and OK.
#include <cstdio>
#include <vector>

#include "../../multi_party_ecdsa_amd/csrc/mpe_gg20_pv.h"

using namespace mpe::gg;

// a signer set as the key object keeps it: party indices ascending, four bits per ordinal
static uint32_t pack(const int* p, int S) {
  uint32_t v = 0;
  for (int i = 0; i < S; ++i) v |= (uint32_t)p[i] << (4 * i);
  return v;
}

// iv(b, vl): the verifier's signer ordinal.  by_party < 0: local slot vl is ordinal loc[vl]; else the rank of party by_party in
// session b's set
struct Shape {
  int B, S, L;
  const int* loc;
  int by_party;
  const uint32_t* set_of;      // [B] when by_party >= 0
  int iv(int b, int vl) const {
    if (by_party < 0) return loc[vl];
    const int r = rank_in(set_of[b], S, by_party);
    return r < 0 ? 0 : r;
  }
};

static int check(const Shape& sh, const char* what) {
  const int B = sh.B, S = sh.S, L = sh.L, P1 = S - 1, PV = L, total = B * PV * S * P1;
  int bad = 0;
  // brute force: every item's class
  std::vector<int> is_self(total, -1);
  int nself = 0;
  for (int b = 0; b < B; ++b)
    for (int vl = 0; vl < PV; ++vl)
      for (int i = 0; i < S; ++i)
        for (int jj = 0; jj < P1; ++jj) {
          const int g = ((b * PV + vl) * S + i) * P1 + jj;
          const PvItem it = pv_item(g, S, PV);
          bad += !(it.b == b && it.vl == vl && it.i == i && it.jj == jj);
          bad += pv_index(b * PV + vl, i, jj, S) != g;
          const bool self = i == sh.iv(b, vl);
          bad += pv_is_self(it, sh.iv(b, vl)) != self;
          is_self[g] = self ? 1 : 0;
          nself += self;
        }
  bad += (size_t)nself != pv_self_count(B, L, S);
  bad += (size_t)(total - nself) != pv_rest_count(B, L, S);
  // the two lists: in range, of the right class, every item exactly once
  std::vector<int> seen(total, 0);
  for (int k = 0; k < (int)pv_self_count(B, L, S); ++k) {
    const int bv = pv_self_bv(k, S), g = pv_self_item(k, S, sh.iv(bv / L, bv % L));
    if (g < 0 || g >= total) { ++bad; continue; }
    bad += is_self[g] != 1;
    ++seen[g];
  }
  for (int k = 0; k < (int)pv_rest_count(B, L, S); ++k) {
    const int bv = pv_rest_bv(k, S), g = pv_rest_item(k, S, sh.iv(bv / L, bv % L));
    if (g < 0 || g >= total) { ++bad; continue; }
    bad += is_self[g] != 0;
    ++seen[g];
  }
  for (int g = 0; g < total; ++g) bad += seen[g] != 1;
  std::printf("case %s B %d S %d L %d items %d self %d bad %d\n", what, B, S, L, total, nself, bad);
  return bad;
}

int main() {
  int bad = 0;
  const int B = 7;
  for (int S = 2; S <= 4; ++S) {
    // every signer local, by slot
    const int all[4] = {0, 1, 2, 3};
    bad += check(Shape{B, S, S, all, -1, nullptr}, "all_local");
    // one local party by slot: every ordinal in turn
    for (int i = 0; i < S; ++i) {
      const int one[1] = {i};
      bad += check(Shape{B, S, 1, one, -1, nullptr}, "one_by_slot");
    }
    // one local party by index under per-session signer sets: party 3 of an 8-party wallet has another rank in every set
    static const int sets[3][4][4] = {{{3, 5}, {0, 3}, {3, 4}, {1, 3}},
                                      {{3, 4, 5}, {0, 3, 5}, {0, 1, 3}, {2, 3, 4}},
                                      {{3, 4, 5, 6}, {0, 3, 5, 7}, {0, 1, 3, 4}, {0, 1, 2, 3}}};
    uint32_t packed[4];
    for (int k = 0; k < 4; ++k) packed[k] = pack(sets[S - 2][k], S);
    uint32_t set_of[B];
    int ranks = 0;
    for (int b = 0; b < B; ++b) { set_of[b] = packed[(b * 3 + 1) % 4]; ranks |= 1 << rank_in(set_of[b], S, 3); }
    bad += check(Shape{B, S, 1, nullptr, 3, set_of}, "one_by_party_index");
    if ((ranks & (ranks - 1)) == 0) { std::printf("FAILED: the sets give party 3 one rank only\n"); ++bad; }
  }
  if (bad) { std::printf("FAILED %d\n", bad); return 1; }
  std::printf("OK\n");
  return 0;
}
