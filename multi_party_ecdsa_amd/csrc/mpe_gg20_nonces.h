// The arrays of mpe_gg20_nonces — everything a signing path is handed in place of OsRng — stated once: every field's row domain and
// width in words, in declaration order.  include/mpecdsa_hip.h (the comment above the struct) is the public statement of the same
// layout; multi_party_ecdsa_amd/wire.py keeps the table as NONCE_FIELDS and tests/test_gg20_layout_cpu.py holds the three together.
// Host-compilable: no HIP types (tests/cpp/test_gg20_layout.cpp includes it).  Included by mpe_gg20.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mpecdsa_hip.h"
#include "mpe_gg20_msg.h"

namespace mpe {
namespace gg {

// the row domains (index conventions at the top of mpe_gg20.h): PI [B][L], AP [B][L][n], MB [B][L][S-1][2], PP [B][L][S-1], B [B]
enum class Dom { PI, AP, MB, PP, B };
constexpr const char* DOM_NAMES[] = {"PI", "AP", "MB", "PP", "B"};

// X(member, domain, words), msg last.  A field's position is also its stream id in the sampler (mpe_sample.h).
#define MPE_GG20_NONCE_FIELDS(X)                                                      \
  X(k, PI, 8) X(gamma, PI, 8) X(blind, PI, 8) X(r_a, PI, 64)                          \
  X(al_alpha, AP, 24) X(al_beta, AP, 64) X(al_gamma, AP, 88) X(al_rho, AP, 72)        \
  X(mb_beta_tag, MB, 64) X(mb_r, MB, 64) X(mb_nonce_b, MB, 8) X(mb_nonce_bt, MB, 8)   \
  X(l, PI, 8) X(ped_s1, PI, 8) X(ped_s2, PI, 8)                                       \
  X(pdl_alpha, PP, 24) X(pdl_beta, PP, 64) X(pdl_rho, PP, 72) X(pdl_gamma, PP, 88)    \
  X(heg_s1, PI, 8) X(heg_s2, PI, 8)                                                   \
  X(msg, B, 8)
struct NonceField { const char* name; const uint32_t* mpe_gg20_nonces::*ptr; Dom dom; int words; };
constexpr int NF = 22;
#define MPE_X(m, d, w) {#m, &mpe_gg20_nonces::m, Dom::d, w},
constexpr NonceField NONCE_FIELDS[NF] = {MPE_GG20_NONCE_FIELDS(MPE_X)};
#undef MPE_X

// the table is the struct: as many members as entries, entry i at member i (a member added, removed or moved does not compile)
#define MPE_X(m, d, w) offsetof(mpe_gg20_nonces, m),
constexpr size_t NONCE_OFFSETS[] = {MPE_GG20_NONCE_FIELDS(MPE_X)};
#undef MPE_X
constexpr bool nonce_fields_in_declaration_order() {
  for (int i = 0; i < NF; ++i) if (NONCE_OFFSETS[i] != i * sizeof(void*)) return false;
  return true;
}
static_assert(sizeof(mpe_gg20_nonces) == NF * sizeof(void*) && sizeof(NONCE_OFFSETS) == NF * sizeof(size_t) && nonce_fields_in_declaration_order(),
              "NONCE_FIELDS lists every member of mpe_gg20_nonces, in declaration order");

// rows of a domain, and words of a field, for B sessions x L local parties (B = 1: per session)
inline size_t nonce_rows(Dom dom, int S, int n, int L, int B) {
  const Counts c = counts_of(B, S, n, L, 0, 0);
  return dom == Dom::PI ? c.nPI : dom == Dom::AP ? c.nAP : dom == Dom::MB ? c.nMB : dom == Dom::PP ? c.nPP : (size_t)B;
}
inline size_t nonce_words(const NonceField& f, int S, int n, int L, int B) { return nonce_rows(f.dom, S, n, L, B) * (size_t)f.words; }

// the one allocation of mpe_gg20_nonces_alloc: every field at a multiple of 64 words, in table order
struct NonceBlob { size_t off[NF], words; };
inline NonceBlob nonce_blob(int S, int n, int L, int B) {
  NonceBlob l{};
  for (int f = 0; f < NF; ++f) { l.off[f] = l.words; l.words += (nonce_words(NONCE_FIELDS[f], S, n, L, B) + 63) & ~(size_t)63; }
  return l;
}
// the arrays of sessions [b0, ...) of a batch: every non-null pointer moved past the rows of the first b0 sessions
inline mpe_gg20_nonces nonces_from_session(mpe_gg20_nonces z, int S, int n, int L, int b0) {
  for (const NonceField& f : NONCE_FIELDS) if (z.*f.ptr) z.*f.ptr += nonce_words(f, S, n, L, b0);
  return z;
}
// one of the first `fields` arrays is NULL
inline bool nonces_missing(const mpe_gg20_nonces& z, int fields) {
  for (int f = 0; f < fields; ++f) if (!(z.*NONCE_FIELDS[f].ptr)) return true;
  return false;
}

}  // namespace gg
}  // namespace mpe
