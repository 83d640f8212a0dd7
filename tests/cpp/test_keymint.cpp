// Key material through the C++ host layer (include/mpecdsa.hpp): `Paillier::keypair()` and `generate_h1_h2_N_tilde()` on the device,
// then an encrypt / decrypt round trip under the minted keys.  Built and run by tests/test_keymint_gpu.py.
#include <cstdio>
#include "mpecdsa.hpp"

using namespace mpecdsa;

static bool nonzero(const Batch& b, size_t i) {
  for (int j = 0; j < b.words; ++j) if (b.row(i)[j]) return true;
  return false;
}

int main() {
  Context ctx(0);
  uint8_t seed[32];
  for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(0xA0 + i);
  const int K = 3;
  paillier::Keypairs kp = paillier::Paillier::keypair(ctx, seed, 1, K);
  if (kp.failed != 0 || kp.p.size() != (size_t)K || kp.n.words != W_N) { std::printf("FAIL keypair\n"); return 1; }
  for (int k = 0; k < K; ++k) {
    if (!(kp.p.row(k)[0] & 1u) || !(kp.q.row(k)[0] & 1u) || !(kp.p.row(k)[31] >> 31) || !(kp.q.row(k)[31] >> 31)) { std::printf("FAIL prime shape\n"); return 2; }
    uint64_t lo = (uint64_t)kp.p.row(k)[0] * kp.q.row(k)[0];
    if ((uint32_t)lo != kp.n.row(k)[0]) { std::printf("FAIL n = p q\n"); return 3; }
  }
  paillier::Keypairs again = paillier::Paillier::keypair(ctx, seed, 1, 2);          // same (seed, counter): the same keys, whatever the count
  for (int j = 0; j < W_PRIME; ++j) if (again.p.row(1)[j] != kp.p.row(1)[j] || again.q.row(0)[j] != kp.q.row(0)[j]) { std::printf("FAIL determinism\n"); return 4; }
  paillier::DecryptionKeys dk(ctx, kp.p, kp.q);
  const int B = 12;
  Batch m(B, W_N), r(B, W_N);
  Index idx(B);
  for (int i = 0; i < B; ++i) {
    idx[i] = i % K;
    for (int j = 0; j < 40; ++j) m.row(i)[j] = 0x9E3779B9u * (uint32_t)(i * 64 + j + 1);
    for (int j = 0; j < 20; ++j) r.row(i)[j] = 0x85EBCA6Bu * (uint32_t)(i * 32 + j + 1) | 1u;
  }
  Batch c = paillier::Paillier::encrypt_with_chosen_randomness(ctx, dk, idx, m, r);
  Batch back = paillier::Paillier::decrypt(ctx, dk, idx, c);
  if (back != m) { std::printf("FAIL round trip\n"); return 5; }
  paillier::EncryptionKeys ek(ctx, kp.n);                                             // a peer encrypts to the same keys
  if (paillier::Paillier::encrypt_with_chosen_randomness(ctx, ek, idx, m, r) != c) { std::printf("FAIL public encrypt\n"); return 6; }
  H1H2NTilde nt = generate_h1_h2_N_tilde(ctx, seed, 2, 2);
  if (nt.failed != 0) { std::printf("FAIL ntilde\n"); return 7; }
  for (size_t i = 0; i < 2; ++i) if (!nonzero(nt.n_tilde, i) || !nonzero(nt.h1, i) || !nonzero(nt.h2, i) || !nonzero(nt.xhi, i) || !nonzero(nt.xhi_inv, i)) { std::printf("FAIL ntilde rows\n"); return 8; }
  zk_paillier::DLogStatements stm(ctx, nt.n_tilde, nt.h1, nt.h2);
  if (stm.count() != 2) { std::printf("FAIL statements\n"); return 9; }
  std::printf("keymint ok: %d key pairs, %d round trips\n", K, B);
  return 0;
}
