// Lindell'17 two-party ECDSA, the KEY GENERATION half and the ephemeral exchange, batched over independent wallets
// (src/protocols/two_party_ecdsa/lindell_2017/):
//   party one  KeyGenFirstMsg::create_commitments_with_fixed_secret_share        party_one.rs:179-219
//   party two  KeyGenSecondMsg::verify_commitments_and_dlog_proof                party_two.rs:180-223
//   party two  EphKeyGenFirstMsg::create_commitments                             party_two.rs:315-371
//   party one  EphKeyGenSecondMsg::verify_commitments_and_dlog_proof             party_one.rs:437-483
//   party one  verify (the ECDSA check of the finished signature)                party_one.rs:567-592
//   party one  generate_h1_h2_n_tilde                                            party_one.rs:594-607
// The messages whose reference form is one existing call stay that call: party two's KeyGenFirstMsg::create = mpe_dlog_prove, party
// one's verify_and_decommit = mpe_dlog_verify, party one's EphKeyGenFirstMsg::create = two base multiplications + mpe_ecddh_prove,
// party two's verify_and_decommit = mpe_ecddh_verify.
// One item per lane in the EC kernels (64 lanes per workgroup, MPE_EC_OCC, as their neighbours in mpe_sigma.h / mpe_blame.h).
// Included by mpe_lib.hip after mpe_lindell.h.
#pragma once
#include "mpe_lindell.h"
#include "mpe_primes.h"
#include "mpe_sigma_dev.h"

namespace mpe {
namespace lk {

__global__ void __launch_bounds__(64) MPE_EC_OCC hash_commit_bigint_kernel(int B, ec::Enc enc, const uint32_t* __restrict__ m, const uint32_t* __restrict__ blind,
                                                                uint32_t* __restrict__ com) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  ec::u256_store(com + (size_t)i * 8, sig::commit_bigint(m + (size_t)i * 8, blind + (size_t)i * 8, enc));
}

// party two's verdict on party one's long-term first and second message (party_two.rs:180-223): both commitments recomputed and
// compared, then DLogProof::verify (the check of dlog_verify_kernel).  A Q1 or R that is no valid point refuses the item.
__global__ void __launch_bounds__(64) MPE_EC_OCC kg_verdict_kernel(int B, ec::Enc enc, const uint32_t* __restrict__ pk_com, const uint32_t* __restrict__ pok_com,
                                                        const uint32_t* __restrict__ blind_pk, const uint32_t* __restrict__ blind_pok,
                                                        const uint32_t* __restrict__ Q1, const uint32_t* __restrict__ R, const uint32_t* __restrict__ z,
                                                        uint8_t* __restrict__ ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const ec::Aff P = ec::aff_load(Q1 + (size_t)i * 16), Rp = ec::aff_load(R + (size_t)i * 16);
  if (!ec::aff_valid(P) || !ec::aff_valid(Rp)) { ok[i] = 0; return; }         // curv rejects such points when it deserialises them
  const bool c1 = ec::u256_eq(sig::commit_point(P, blind_pk + (size_t)i * 8, enc), ec::u256_load(pk_com + (size_t)i * 8));       // :195-202
  const bool c2 = ec::u256_eq(sig::commit_point(Rp, blind_pok + (size_t)i * 8, enc), ec::u256_load(pok_com + (size_t)i * 8));    // :203-215
  const bool pr = sig::dlog_verify_body(P, Rp, ec::sc_reduce(z + (size_t)i * 8, 8), enc);                                        // :221
  ok[i] = (c1 && c2 && pr) ? 1 : 0;
}

// party two's ephemeral first message with its witness (party_two.rs:315-371): public_share = k2 G, c = k2 H (H = base_point2), the
// ECDDHProof over (G, public_share, H, c) — the words mpe_ecddh_prove gives for that statement —, pk_commitment = Com(public_share)
// and zk_pok_commitment = Com(H(a1, a2) as a BigInt).  Four comb multiplications, no ladder.
__global__ void __launch_bounds__(64) MPE_EC_OCC eph_first_kernel(int B, ec::Enc enc, const uint32_t* __restrict__ k2, const uint32_t* __restrict__ nonce,
                                                       const uint32_t* __restrict__ blind_pk, const uint32_t* __restrict__ blind_pok,
                                                       uint32_t* __restrict__ pub, uint32_t* __restrict__ c, uint32_t* __restrict__ a1, uint32_t* __restrict__ a2,
                                                       uint32_t* __restrict__ z, uint32_t* __restrict__ pk_com, uint32_t* __restrict__ pok_com) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const ec::U256 x = ec::sc_reduce(k2 + (size_t)i * 8, 8), s = ec::sc_reduce(nonce + (size_t)i * 8, 8);
  const ec::Aff G = ec::aff_gen(), H = ec::aff_h2();
  const ec::Aff P = ec::jac_to_aff(ec::jac_mul_gen(x)), Cc = ec::jac_to_aff(ec::jac_mul_h2(x));                                // :320-324
  ec::Aff A1, A2;
  ec::U256 zz;
  sig::ecddh_prove_body<sig::GEN, sig::H2>(x, s, G, P, H, Cc, enc, A1, A2, zz);                                                // ECDDHProof::prove :334
  ec::aff_store(pub + (size_t)i * 16, P);
  ec::aff_store(c + (size_t)i * 16, Cc);
  ec::aff_store(a1 + (size_t)i * 16, A1);
  ec::aff_store(a2 + (size_t)i * 16, A2);
  ec::u256_store(z + (size_t)i * 8, zz);
  ec::u256_store(pk_com + (size_t)i * 8, sig::commit_point(P, blind_pk + (size_t)i * 8, enc));                                  // :338-342
  const ec::U256 dg = sig::points_digest(enc, A1, A2);
  ec::u256_store(pok_com + (size_t)i * 8, sig::commit_bigint(dg.w, blind_pok + (size_t)i * 8, enc));                                // :345-351
}

// party one's verdict on it (party_one.rs:437-483): both commitments, then ECDDHProof::verify over (G, public_share, H, c); the two
// multiplications by z run on the comb tables of G and H
__global__ void __launch_bounds__(64) MPE_EC_OCC eph_verdict_kernel(int B, ec::Enc enc, const uint32_t* __restrict__ pk_com, const uint32_t* __restrict__ pok_com,
                                                         const uint32_t* __restrict__ blind_pk, const uint32_t* __restrict__ blind_pok,
                                                         const uint32_t* __restrict__ pub, const uint32_t* __restrict__ c, const uint32_t* __restrict__ a1,
                                                         const uint32_t* __restrict__ a2, const uint32_t* __restrict__ z, uint8_t* __restrict__ ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const ec::Aff P = ec::aff_load(pub + (size_t)i * 16), Cc = ec::aff_load(c + (size_t)i * 16), A1 = ec::aff_load(a1 + (size_t)i * 16),
                A2 = ec::aff_load(a2 + (size_t)i * 16);
  if (!(ec::aff_valid(P) && ec::aff_valid(Cc) && ec::aff_valid(A1) && ec::aff_valid(A2))) { ok[i] = 0; return; }
  const bool c1 = ec::u256_eq(sig::commit_point(P, blind_pk + (size_t)i * 8, enc), ec::u256_load(pk_com + (size_t)i * 8));       // :451-458
  const ec::U256 dg = sig::points_digest(enc, A1, A2);
  const bool c2 = ec::u256_eq(sig::commit_bigint(dg.w, blind_pok + (size_t)i * 8, enc), ec::u256_load(pok_com + (size_t)i * 8));     // :459-468
  const ec::Aff G = ec::aff_gen(), H = ec::aff_h2();
  const bool pr = sig::ecddh_verify_body<sig::GEN, sig::H2>(G, P, H, Cc, A1, A2, ec::sc_reduce(z + (size_t)i * 8, 8), enc);      // :480
  ok[i] = (c1 && c2 && pr) ? 1 : 0;
}

// party_one::verify (party_one.rs:567-592): accept iff pub is a valid point, 1 <= s and s < q - s (so s >= q and high s are refused),
// P = (m mod q) s^-1 G + (r mod q) s^-1 pub is finite and r == P.x AS INTEGERS (P.x is not reduced mod q; r is reduced only where it
// enters u2).  Where the reference would panic (s = 0 mod q: invert().unwrap(); P at infinity: x_coord().unwrap()) the item is refused.
// (The GG20 check inside complete_kernel is another rule: it compares P.x mod q and accepts s up to q - 1.)
__global__ void __launch_bounds__(64) MPE_EC_OCC ecdsa_verify_kernel(int B, const uint32_t* __restrict__ pub, const uint32_t* __restrict__ msg,
                                                          const uint32_t* __restrict__ r, const uint32_t* __restrict__ s, uint8_t* __restrict__ ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const ec::Aff Y = ec::aff_load(pub + (size_t)i * 16);
  const ec::U256 sv = ec::u256_load(s + (size_t)i * 8), rv = ec::u256_load(r + (size_t)i * 8);
  bool v = ec::aff_valid(Y) && !ec::u256_is_zero(sv) && !ec::u256_ge(sv, ec::FQ);
  if (v) {                                                              // s < q - s                                  :586
    const ec::U256 neg = ec::sc_neg(sv);
    bool lt = false;
    for (int j = 7; j >= 0; --j) { if (sv.w[j] != neg.w[j]) { lt = sv.w[j] < neg.w[j]; break; } }
    v = lt;
  }
  if (!v) { ok[i] = 0; return; }
  const ec::U256 si = ec::sc_inv(sv);                                                                                         // :575
  const ec::U256 u1 = ec::sc_mul(ec::sc_reduce(msg + (size_t)i * 8, 8), si), u2 = ec::sc_mul(ec::sc_reduce(rv.w, 8), si);       // :576-579
  const ec::Aff V = ec::jac_to_aff(ec::jac_add(ec::jac_mul_gen(u1), ec::jac_mul(u2, Y)));
  ok[i] = (!V.inf && ec::u256_eq(V.x, rv)) ? 1 : 0;                                                                           // :582-585
}

// out = a b mod q (both reduced as read): Party1Private::refresh_private_key / Party2Private::update_private_key multiply a share by the factor
__global__ void sc_mul_kernel(int B, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  ec::u256_store(out + (size_t)i * 8, ec::sc_mul(ec::sc_reduce(a + (size_t)i * 8, 8), ec::sc_reduce(b + (size_t)i * 8, 8)));
}

// after the two draws: xhi (the 256-bit exponent) out of its 9-word sampling row; a failed item inverts the harmless h1 = 1 modulo 3
__global__ void nt_xhi_kernel(int n, const int32_t* __restrict__ bad, const uint32_t* __restrict__ xhi9, uint32_t* __restrict__ xhi, uint32_t* __restrict__ h1) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  for (int j = 0; j < 8; ++j) xhi[(size_t)k * 8 + j] = bad[k] ? 0u : xhi9[(size_t)k * 9 + j];
  if (bad[k]) { sm::zero(h1 + (size_t)k * 64, 64); h1[(size_t)k * 64] = 1u; }
}
// N~ out; an item whose prime search or draw gave up, or whose h1 is no unit modulo N~ (the reference would unwrap() a None there),
// gets zero rows and counts once in *fail
__global__ void nt_out_kernel(int n, const uint32_t* __restrict__ nt_ms, const int32_t* __restrict__ bad, const uint8_t* __restrict__ inv_ok,
                              uint32_t* __restrict__ Nt, uint32_t* __restrict__ h1, uint32_t* __restrict__ h2, uint32_t* __restrict__ xhi, int32_t* __restrict__ fail) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const size_t o = (size_t)k * 64;
  if (bad[k] || !inv_ok[k]) {
    sm::zero(Nt + o, 64); sm::zero(h1 + o, 64); sm::zero(h2 + o, 64); sm::zero(xhi + (size_t)k * 8, 8);
    if (fail) atomicAdd(fail, 1);
    return;
  }
  for (int j = 0; j < 64; ++j) Nt[o + j] = nt_ms[o + j];
}

}  // namespace lk
}  // namespace mpe

extern "C" {

int mpe_hash_commit_bigint(mpe_ctx* ctx, int batch, const uint32_t* d_m, const uint32_t* d_blind, uint32_t* d_com, void* stream) {
  if (!ctx || !d_m || !d_blind || !d_com || batch < 0) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::lk::hash_commit_bigint_kernel, batch, st, batch, ctx->enc, d_m, d_blind, d_com);
  return MPE_OK;
}

// DLogProof::prove(x1) is dlog_prove_kernel and both commitments are hash_commit_kernel's: three launches, no kernel of its own
int mpe_lindell_keygen_first_msg(mpe_ctx* ctx, int batch, const uint32_t* d_x1, const uint32_t* d_nonce, const uint32_t* d_blind_pk,
                                 const uint32_t* d_blind_pok, uint32_t* d_Q1, uint32_t* d_R, uint32_t* d_z, uint32_t* d_pk_com, uint32_t* d_pok_com,
                                 void* stream) {
  if (!ctx || !d_x1 || !d_nonce || !d_blind_pk || !d_blind_pok || !d_Q1 || !d_R || !d_z || !d_pk_com || !d_pok_com || batch < 0) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::dlog_prove_kernel, batch, st, batch, ctx->enc, d_x1, d_nonce, d_Q1, d_R, d_z);                            // party_one.rs:183-185
  MPE_LAUNCH_1D(mpe::hash_commit_kernel, batch, st, batch, ctx->enc, (const uint32_t*)d_Q1, d_blind_pk, d_pk_com);             // :187-192
  MPE_LAUNCH_1D(mpe::hash_commit_kernel, batch, st, batch, ctx->enc, (const uint32_t*)d_R, d_blind_pok, d_pok_com);            // :194-199
  return MPE_OK;
}

int mpe_lindell_keygen_verify_first_msg(mpe_ctx* ctx, int batch, const uint32_t* d_pk_com, const uint32_t* d_pok_com, const uint32_t* d_blind_pk,
                                        const uint32_t* d_blind_pok, const uint32_t* d_Q1, const uint32_t* d_R, const uint32_t* d_z, uint8_t* d_ok,
                                        void* stream) {
  if (!ctx || !d_pk_com || !d_pok_com || !d_blind_pk || !d_blind_pok || !d_Q1 || !d_R || !d_z || !d_ok || batch < 0) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::lk::kg_verdict_kernel, batch, st, batch, ctx->enc, d_pk_com, d_pok_com, d_blind_pk, d_blind_pok, d_Q1, d_R, d_z, d_ok);
  return MPE_OK;
}

int mpe_lindell_eph_first_msg(mpe_ctx* ctx, int batch, const uint32_t* d_k2, const uint32_t* d_nonce, const uint32_t* d_blind_pk,
                              const uint32_t* d_blind_pok, uint32_t* d_pub, uint32_t* d_c, uint32_t* d_a1, uint32_t* d_a2, uint32_t* d_z,
                              uint32_t* d_pk_com, uint32_t* d_pok_com, void* stream) {
  if (!ctx || !d_k2 || !d_nonce || !d_blind_pk || !d_blind_pok || !d_pub || !d_c || !d_a1 || !d_a2 || !d_z || !d_pk_com || !d_pok_com || batch < 0)
    return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::lk::eph_first_kernel, batch, st, batch, ctx->enc, d_k2, d_nonce, d_blind_pk, d_blind_pok, d_pub, d_c, d_a1, d_a2, d_z, d_pk_com, d_pok_com);
  return MPE_OK;
}

int mpe_lindell_eph_verify_first_msg(mpe_ctx* ctx, int batch, const uint32_t* d_pk_com, const uint32_t* d_pok_com, const uint32_t* d_blind_pk,
                                     const uint32_t* d_blind_pok, const uint32_t* d_pub, const uint32_t* d_c, const uint32_t* d_a1, const uint32_t* d_a2,
                                     const uint32_t* d_z, uint8_t* d_ok, void* stream) {
  if (!ctx || !d_pk_com || !d_pok_com || !d_blind_pk || !d_blind_pok || !d_pub || !d_c || !d_a1 || !d_a2 || !d_z || !d_ok || batch < 0) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::lk::eph_verdict_kernel, batch, st, batch, ctx->enc, d_pk_com, d_pok_com, d_blind_pk, d_blind_pok, d_pub, d_c, d_a1, d_a2, d_z, d_ok);
  return MPE_OK;
}

int mpe_ecdsa_verify(mpe_ctx* ctx, int batch, const uint32_t* d_pub, const uint32_t* d_msg, const uint32_t* d_r, const uint32_t* d_s, uint8_t* d_ok,
                     void* stream) {
  if (!ctx || !d_pub || !d_msg || !d_r || !d_s || !d_ok || batch < 0) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::lk::ecdsa_verify_kernel, batch, st, batch, d_pub, d_msg, d_r, d_s, d_ok);
  return MPE_OK;
}

int mpe_scalar_mul(mpe_ctx* ctx, int batch, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, void* stream) {
  if (!ctx || !d_a || !d_b || !d_out || batch < 0) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::lk::sc_mul_kernel, batch, st, batch, d_a, d_b, d_out);
  return MPE_OK;
}

// Field f draws stream counter | f << 56: 6 p~, 7 q~, 14 h1, 15 xhi (0..5 are mpe_paillier_keygen / mpe_ntilde_generate, 8..13 the GG20 keygen chain)
int mpe_lindell_ntilde_generate(mpe_ctx* ctx, int count, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_Nt, uint32_t* d_h1,
                                uint32_t* d_h2, uint32_t* d_xhi, int32_t* d_fail, void* stream) {
  if (!ctx || !h_seed32 || !d_Nt || !d_h1 || !d_h2 || !d_xhi || count < 0 || count > (1 << 22) || (counter >> 56) != 0 || max_attempts < 0 ||
      max_attempts > (1 << 24))
    return MPE_E_ARG;
  if (count == 0) return MPE_OK;
  using namespace mpe;
  hipStream_t st = (hipStream_t)stream;
  const smp::Seed key = smp::seed_of(h_seed32);
  const int cap = max_attempts ? max_attempts : pr::DEFAULT_MAX_ATTEMPTS;
  auto sid = [&](int f) { return counter | ((uint64_t)f << 56); };
  // p~, q~, phi, the 9-word sampling rows of xhi and h1^-1 live in the context workspace (mpe_ctx_wipe covers them); the two prime
  // searches and the inversion allocate behind these arrays, one after the other
  MPE_TRY(ws_begin(ctx, st));
  uint32_t* pt = ws_array<uint32_t>(ctx, (size_t)count * 32);
  uint32_t* qt = ws_array<uint32_t>(ctx, (size_t)count * 32);
  uint32_t* nt_ms = ws_array<uint32_t>(ctx, (size_t)count * 64);
  uint32_t* phi = ws_array<uint32_t>(ctx, (size_t)count * 64);
  uint32_t* h1inv = ws_array<uint32_t>(ctx, (size_t)count * 64);
  uint32_t* xhi9 = ws_array<uint32_t>(ctx, (size_t)count * 9);
  uint32_t* two256 = ws_array<uint32_t>(ctx, 9);
  int32_t* bad = ws_array<int32_t>(ctx, count);
  uint8_t* inv_ok = ws_array<uint8_t>(ctx, count);
  MPE_TRY(ws_ok(ctx));
  MPE_TRY(pr::search_primes(ctx, count, key, sid(6), cap, pt, nullptr, nullptr, st));                          // Paillier::keypair()  :597
  MPE_TRY(pr::search_primes(ctx, count, key, sid(7), cap, qt, nullptr, nullptr, st));
  MPE_LAUNCH_1D(pr::nt_setup_kernel, count, st, count, pt, qt, nt_ms, phi, bad);                               // N~, phi  :599
  hipLaunchKernelGGL(kg::fill_words_kernel, dim3(1), dim3(64), 0, st, 1, 9, 256, two256);
  (void)hipMemsetAsync(h1inv, 0, (size_t)count * 64 * 4, st);
  (void)hipMemsetAsync(inv_ok, 0, (size_t)count, st);
  MPE_TRY(smp::launch_sample(count, h_seed32, sid(14), 0, phi, 64, nullptr, count, 0, 64, d_h1, nullptr, st, nullptr, ctx->sampler_max_attempts, bad));     // h1 = sample_below(phi)  :600
  MPE_TRY(smp::launch_sample(count, h_seed32, sid(15), 0, two256, 9, nullptr, 1, 0, 9, xhi9, nullptr, st, nullptr, ctx->sampler_max_attempts, bad));        // xhi = sample_below(2^256)  :601-602
  MPE_LAUNCH_1D(lk::nt_xhi_kernel, count, st, count, (const int32_t*)bad, (const uint32_t*)xhi9, d_xhi, d_h1);
  mpe_modset* ms = nullptr;
  MPE_TRY(modset_create_dev(ctx, 2048, count, nt_ms, &ms, st));
  const Rows sel = rows(nullptr, 1);                                                                           // modulus i for item i
  int rc = launch_modinv(ctx, ms, count, sel, rows(d_h1, 64), h1inv, inv_ok, st);                              // h1^-1 mod N~  :603
  if (rc == MPE_OK) rc = launch_modexp(ctx, ms, count, sel, rows(h1inv, 64), no_rows(), rows(d_xhi, 8), 8, d_h2, st);      // ^xhi: a 256-bit ladder  :604
  if (rc == MPE_OK) {
    hipLaunchKernelGGL(lk::nt_out_kernel, dim3(blocks_for(count, 64)), dim3(64), 0, st, count, (const uint32_t*)nt_ms, (const int32_t*)bad, (const uint8_t*)inv_ok,
                       d_Nt, d_h1, d_h2, d_xhi, d_fail);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);          // the moduli set is released below
    if (e != hipSuccess) { mpe_set_error("mpe_lindell_ntilde_generate", e); rc = MPE_E_HIP; }
  } else {
    (void)hipStreamSynchronize(st);
  }
  mpe_modset_destroy(ms);
  return rc;
}

}  // extern "C"
