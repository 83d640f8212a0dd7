// Round 5's PDL verification items, stated once: item g of a batch is (session b, local verifier vl, prover ordinal i, proof jj)
//   g = ((b PV + vl) S + i) (S-1) + jj
// and the verifier of local slot vl has a signer ordinal iv of its own (mpe_gg20.h loc_of).  The items with i == iv are the
// verifier's OWN proofs: their ciphertext lies under the verifier's Paillier key, whose p and q it holds (mpe_paillier.h
// modexp_nn2_holder).  With PV == L they are (S-1) of every S (S-1) items of a (session, verifier): B L (S-1) in all, listed by
// pv_self_item; pv_rest_item lists the other B L (S-1)^2.
// Host-compilable: no HIP types (tests/cpp/test_r5_self_items.cpp includes it alone).  Included by mpe_gg20.h.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define MPE_PV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MPE_PV_HD inline
#endif

namespace mpe {
namespace gg {

// peer slot jj of ordinal i -> the peer's ordinal; an ordinal's rank in a set given as four bits per ordinal
MPE_PV_HD int ind_of(int i, int jj) { return jj < i ? jj : jj + 1; }
MPE_PV_HD int rank_in(uint32_t set4, int S, int party) {
  int r = -1;
  for (int i = 0; i < S; ++i) if ((int)((set4 >> (4 * i)) & 15u) == party) r = i;
  return r;
}

struct PvItem { int b, vl, i, jj; };
MPE_PV_HD PvItem pv_item(int g, int S, int PV) {
  const int P1 = S - 1, r1 = g / P1, r2 = r1 / S;
  return PvItem{r2 / PV, r2 % PV, r1 % S, g % P1};
}
// bv = b PV + vl
MPE_PV_HD int pv_index(int bv, int i, int jj, int S) { return (bv * S + i) * (S - 1) + jj; }
MPE_PV_HD bool pv_is_self(const PvItem& it, int iv) { return it.i == iv; }
inline size_t pv_self_count(int B, int L, int S) { return (size_t)B * L * (S - 1); }
inline size_t pv_rest_count(int B, int L, int S) { return (size_t)B * L * (S - 1) * (S - 1); }
// which (session, verifier) the k-th self / rest item belongs to: the caller looks its ordinal iv up and asks for the item
MPE_PV_HD int pv_self_bv(int k, int S) { return k / (S - 1); }
MPE_PV_HD int pv_rest_bv(int k, int S) { return k / ((S - 1) * (S - 1)); }
MPE_PV_HD int pv_self_item(int k, int S, int iv) { return pv_index(k / (S - 1), iv, k % (S - 1), S); }
MPE_PV_HD int pv_rest_item(int k, int S, int iv) {
  const int P1 = S - 1, r = k / P1;
  return pv_index(r / P1, ind_of(iv, r % P1), k % P1, S);
}

}  // namespace gg
}  // namespace mpe
