// One (t = 1, n = 3) wallet dealt, constructed and confirmed through the C++ host layer (include/mpecdsa.hpp): `VerifiableSS::share`,
// the verdict and the OK branch of `phase2_verify_vss_construct_keypair_phase3_pok_dlog`, `Keys::verify_dlog_proofs_check_against_vss`,
// and one tampered proof.  Built and run by tests/test_keygen_deal_cpp_gpu.py.
#include <cstdio>
#include "mpecdsa.hpp"

using namespace mpecdsa;
using namespace mpecdsa::gg_2020;

int main() {
  Context ctx(0);
  const uint16_t t = 1, n = 3;
  // coefficients small enough that no sum below wraps mod q: the host can add them word by word
  Batch coef(n, (t + 1) * W_SCALAR), nonce(n, W_SCALAR);
  for (int j = 0; j < n; ++j) {
    coef.row(j)[0] = 0x1000u + 17u * j;  coef.row(j)[1] = 0x9E37u + j;          // u_j
    coef.row(j)[W_SCALAR] = 0x77u + 5u * j;  coef.row(j)[W_SCALAR + 2] = 0x1234u * (j + 1);   // a_j
    for (int w = 0; w < W_SCALAR; ++w) nonce.row(j)[w] = 0x85EBCA6Bu * (uint32_t)(j * 8 + w + 1);
  }
  auto [vss, shares] = VerifiableSS::share(ctx, t, n, coef);
  if (vss.commitments.size() != (size_t)n || vss.commitments.words != (t + 1) * W_POINT || shares.words != n * W_SCALAR) { std::printf("FAIL share shapes\n"); return 1; }
  // commitments[j][0] = u_j G = y_j
  Batch u(n, W_SCALAR), y(n, W_POINT);
  for (int j = 0; j < n; ++j) for (int w = 0; w < W_SCALAR; ++w) u.row(j)[w] = coef.row(j)[w];
  const Batch ug = ec_mul_base(ctx, u);
  for (int j = 0; j < n; ++j) for (int w = 0; w < W_POINT; ++w) {
    y.row(j)[w] = vss.commitments.row(j)[w];
    if (y.row(j)[w] != ug.row(j)[w]) { std::printf("FAIL commitments[0] != u G\n"); return 2; }
  }
  // round 2 as party r sees it: items (r, dealer j)
  VerifiableSS seen{t, n, Batch((size_t)n * n, (t + 1) * W_POINT)};
  Batch got((size_t)n * n, W_SCALAR), y_it((size_t)n * n, W_POINT), recv(n, n * W_SCALAR), y_vec(n, n * W_POINT);
  Index index((size_t)n * n);
  for (int r = 0; r < n; ++r) for (int j = 0; j < n; ++j) {
    const size_t it = (size_t)r * n + j;
    index[it] = r + 1;
    for (int w = 0; w < (t + 1) * W_POINT; ++w) seen.commitments.row(it)[w] = vss.commitments.row(j)[w];
    for (int w = 0; w < W_SCALAR; ++w) got.row(it)[w] = recv.row(r)[j * W_SCALAR + w] = shares.row(j)[r * W_SCALAR + w];
    for (int w = 0; w < W_POINT; ++w) y_it.row(it)[w] = y_vec.row(r)[j * W_POINT + w] = y.row(j)[w];
  }
  std::vector<uint32_t> bad;
  Flags ok2 = Keys::phase2_verify_vss(ctx, n, seen, got, index, y_it, &bad);
  for (uint8_t f : ok2) if (!f) { std::printf("FAIL round 2 refuses an honest share\n"); return 3; }
  for (uint32_t m : bad) if (m) { std::printf("FAIL round 2 mask\n"); return 3; }
  got.row(1 * n + 2)[0] ^= 1u;                                                    // dealer 3's share to party 2
  ok2 = Keys::phase2_verify_vss(ctx, n, seen, got, index, y_it, &bad);
  if (ok2[1 * n + 2] || bad[0] != 0 || bad[1] != 0b100 || bad[2] != 0) { std::printf("FAIL round 2 misses the flipped share\n"); return 4; }
  // the key pair of every party and its proof
  auto [sk, proofs] = Keys::phase2_construct_keypair_phase3_pok_dlog(ctx, n, recv, y_vec, nonce);
  for (int r = 1; r < n; ++r) for (int w = 0; w < W_POINT; ++w) if (sk.y.row(r)[w] != sk.y.row(0)[w]) { std::printf("FAIL parties disagree on y\n"); return 5; }
  Batch usum(1, W_SCALAR);
  uint64_t carry = 0;
  for (int w = 0; w < W_SCALAR; ++w) {
    for (int j = 0; j < n; ++j) carry += u.row(j)[w];
    usum.row(0)[w] = (uint32_t)carry;
    carry >>= 32;
  }
  const Batch yg = ec_mul_base(ctx, usum);
  for (int w = 0; w < W_POINT; ++w) if (yg.row(0)[w] != sk.y.row(0)[w]) { std::printf("FAIL y != (sum u_j) G\n"); return 6; }
  if (ec_mul_base(ctx, sk.x_i) != proofs.pk) { std::printf("FAIL pk != x_i G\n"); return 7; }
  curv::DLogProof again = curv::DLogProof::prove(ctx, sk.x_i, nonce);
  if (again.pk != proofs.pk || again.pk_t_rand_commitment != proofs.pk_t_rand_commitment || again.challenge_response != proofs.challenge_response) {
    std::printf("FAIL proof != DLogProof::prove(x_i)\n"); return 8;
  }
  // round 3
  Flags ok3 = Keys::verify_dlog_proofs_check_against_vss(ctx, n, proofs, vss, &bad);
  if (ok3 != Flags{1, 1, 1} || bad != std::vector<uint32_t>{0}) { std::printf("FAIL round 3 refuses an honest wallet\n"); return 9; }
  curv::DLogProof tampered = proofs;
  tampered.challenge_response.row(1)[3] ^= 0x10u;
  ok3 = Keys::verify_dlog_proofs_check_against_vss(ctx, n, tampered, vss, &bad);
  if (ok3 != Flags{1, 0, 1} || bad != std::vector<uint32_t>{0b010}) { std::printf("FAIL round 3 misses the tampered proof\n"); return 10; }
  std::printf("keygen deal ok: 1 wallet (t = %d, n = %d), 1 tampered share and 1 tampered proof refused\n", (int)t, (int)n);
  return 0;
}
