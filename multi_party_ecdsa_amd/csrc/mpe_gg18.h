// GG18 threshold signing (src/protocols/multi_party_ecdsa/gg_2018/party_i.rs:384-737), the calls examples/gg18_sign_client.rs makes,
// batched over independent sessions:
//   SignKeys::create                                      :385-406    -> mpe_gg18_sign_keys
//   MessageB::b_with_predefined_randomness(.., &[])       mta/mod.rs:111-158 -> mpe_gg18_message_b (the tail mpe_mta_message_b shares)
//   phase2_delta_i / phase2_sigma_i                       :426-444    -> mpe_gg18_phase2
//   phase3_reconstruct_delta / phase4                     :446-483    -> mpe_gg18_phase4
//   phase5_local_sig / phase5a_broadcast_5b_zkproof       :487-559    -> mpe_gg18_phase5a
//   phase5c                                               :561-636    -> mpe_gg18_phase5c
//   phase5d                                               :638-673    -> mpe_gg18_phase5d
//   output_signature / verify                             :674-737    -> mpe_gg18_output_signature
// What is one existing call stays that call: phase1_broadcast = mpe_hash_commit_point, MessageA::a(.., &[]) = mpe_paillier_encrypt of
// the zero-extended k_i, verify_proofs_get_alpha = mpe_mta_verify_get_alpha.
// Item pi = li * B + b: local party li (signer ordinal i = loc[li]) of session b.  Broadcast values are sender-major [S][B][w] (own
// value included), values of the local parties [L][B][w], per-peer values [L][S-1][B][w] (peer slot jj = signer ordinal jj, or jj + 1
// from the own ordinal on).  One item per lane (64 lanes per workgroup, MPE_EC_OCC, as mpe_sigma.h / mpe_lindell_keygen.h).
// A party whose status is not 0 when a phase starts, or becomes so inside it, emits all-zero words for that phase: a zero point is no
// valid point, so its peers refuse it with the code of the phase in which they read it.
// Included by mpe_lib.hip after mpe_lindell_keygen.h.
#pragma once
#include "mpe_gg20.h"
#include "mpe_mta.h"

namespace mpe {
namespace g18 {

struct Dim {
  int B, S, L;
  int sg[8];          // party index of signer ordinal j (ascending)
  int loc[8];         // signer ordinal of local party li
  ec::Enc enc;
};

__device__ __forceinline__ void zero_words(uint32_t* p, int n) { for (int j = 0; j < n; ++j) p[j] = 0u; }
// the first failure sticks
__device__ __forceinline__ void fail(int32_t* status, int pi, int code) { if (status[pi] == 0) status[pi] = code; }

// SignKeys::create (:385-406) with k_i, gamma_i handed in: w_i = lambda_i x_i, g_w_i, g_gamma_i; status 0 or 91
__global__ void __launch_bounds__(64) MPE_EC_OCC sign_keys_kernel(Dim d, const uint32_t* __restrict__ x_i, const uint32_t* __restrict__ k_in,
                                                                  const uint32_t* __restrict__ gamma_in, uint32_t* __restrict__ w, uint32_t* __restrict__ g_w_i,
                                                                  uint32_t* __restrict__ g_gamma, int32_t* __restrict__ status) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= d.B * d.L) return;
  const int i = d.loc[pi / d.B];
  // k_i, gamma_i are `Scalar::random()` (:396,402): non-zero and below q; anything else is what a sampler that gave up leaves
  if (!ec::sc_is_canonical_nonzero(k_in + (size_t)pi * 8) || !ec::sc_is_canonical_nonzero(gamma_in + (size_t)pi * 8)) {
    status[pi] = MPE_GG20_STATUS_BAD_NONCE;
    zero_words(w + (size_t)pi * 8, 8); zero_words(g_w_i + (size_t)pi * 16, 16); zero_words(g_gamma + (size_t)pi * 16, 16);
    return;
  }
  status[pi] = 0;
  const ec::U256 wi = ec::sc_mul(gg::lagrange0(d.sg, d.S, i), ec::sc_reduce(x_i + (size_t)pi * 8, 8));                      // :391-393
  ec::u256_store(w + (size_t)pi * 8, wi);
  ec::aff_store(g_w_i + (size_t)pi * 16, ec::jac_to_aff(ec::jac_mul_gen(wi)));                                               // :395
  ec::aff_store(g_gamma + (size_t)pi * 16, ec::jac_to_aff(ec::jac_mul_gen(ec::sc_reduce(gamma_in + (size_t)pi * 8, 8))));    // :397
}
// g_w of every signer from pk_vec [B][n][16]: lambda_j X_j (what Keys::update_commitments_to_xi gives, gg18_sign_client.rs:235-240);
// item j * B + b.  An X_j that is no valid point leaves a zero row (which equals no b_proof.pk that passed its check).
__global__ void __launch_bounds__(64) MPE_EC_OCC g_w_kernel(Dim d, int n, const uint32_t* __restrict__ pk_vec, uint32_t* __restrict__ g_w) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= d.S * d.B) return;
  const int j = g / d.B, b = g % d.B;
  const ec::Aff X = ec::aff_load(pk_vec + ((size_t)b * n + d.sg[j]) * 16);
  if (!ec::aff_valid(X)) { zero_words(g_w + (size_t)g * 16, 16); return; }
  ec::aff_store(g_w + (size_t)g * 16, ec::mul_aff(gg::lagrange0(d.sg, d.S, j), X));
}

// the verdicts of the 2 (S-1) verify_proofs_get_alpha calls in the order of gg18_sign_client.rs:221-244, then phase2_delta_i and
// phase2_sigma_i (:426-444)
__global__ void __launch_bounds__(64) MPE_EC_OCC phase2_kernel(Dim d, const uint32_t* __restrict__ k, const uint32_t* __restrict__ gamma, const uint32_t* __restrict__ w,
                                                               const uint32_t* __restrict__ alpha, const uint32_t* __restrict__ beta, const uint32_t* __restrict__ miu,
                                                               const uint32_t* __restrict__ ni, const uint8_t* __restrict__ ok_gamma, const uint8_t* __restrict__ ok_w,
                                                               const uint32_t* __restrict__ w_pk, const uint32_t* __restrict__ g_w, uint32_t* __restrict__ delta_i,
                                                               uint32_t* __restrict__ sigma_i, int32_t* __restrict__ status) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= d.B * d.L) return;
  const int li = pi / d.B, b = pi % d.B, i = d.loc[li], P1 = d.S - 1;
  if (status[pi] == 0) {
    for (int jj = 0; jj < P1; ++jj) {
      const int ind = jj < i ? jj : jj + 1;
      const size_t it = ((size_t)li * P1 + jj) * d.B + b;
      if (!ok_gamma[it] || !ok_w[it]) { fail(status, pi, 201); break; }                                 // test.rs:265,272
      // the w side's b_proof.pk is that PEER's g_w (the comment at test.rs:274-277)
      if (!ec::aff_eq(ec::aff_load(w_pk + it * 16), ec::aff_load(g_w + ((size_t)ind * d.B + b) * 16))) { fail(status, pi, 202); break; }
    }
  }
  if (status[pi] != 0) { zero_words(delta_i + (size_t)pi * 8, 8); zero_words(sigma_i + (size_t)pi * 8, 8); return; }
  const ec::U256 kk = ec::sc_reduce(k + (size_t)pi * 8, 8);
  ec::U256 dl = ec::sc_mul(kk, ec::sc_reduce(gamma + (size_t)pi * 8, 8)), sg = ec::sc_mul(kk, ec::sc_reduce(w + (size_t)pi * 8, 8));
  for (int jj = 0; jj < P1; ++jj) {
    const size_t it = ((size_t)li * P1 + jj) * d.B + b;
    dl = ec::sc_add(dl, ec::sc_add(ec::sc_reduce(alpha + it * 8, 8), ec::sc_reduce(beta + it * 8, 8)));
    sg = ec::sc_add(sg, ec::sc_add(ec::sc_reduce(miu + it * 8, 8), ec::sc_reduce(ni + it * 8, 8)));
  }
  ec::u256_store(delta_i + (size_t)pi * 8, dl);
  ec::u256_store(sigma_i + (size_t)pi * 8, sg);
}

// phase3_reconstruct_delta and phase4 as gg18_sign_client.rs:272-309 uses them: the peers' b_proof.pk == g_gamma_i and commitments,
// then R = delta^-1 (sum of every g_gamma_i, the own one included)
__global__ void __launch_bounds__(64) MPE_EC_OCC phase4_kernel(Dim d, const uint32_t* __restrict__ delta, const uint32_t* __restrict__ b_pk,
                                                               const uint32_t* __restrict__ g_gamma, const uint32_t* __restrict__ blind, const uint32_t* __restrict__ com,
                                                               uint32_t* __restrict__ R, int32_t* __restrict__ status) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= d.B * d.L) return;
  const int li = pi / d.B, b = pi % d.B, i = d.loc[li], P1 = d.S - 1;
  uint32_t* Ro = R + (size_t)pi * 16;
  if (status[pi] != 0) { zero_words(Ro, 16); return; }
  ec::U256 tot = ec::u256_zero();
  for (int j = 0; j < d.S; ++j) tot = ec::sc_add(tot, ec::sc_reduce(delta + ((size_t)j * d.B + b) * 8, 8));
  if (ec::u256_is_zero(tot)) { fail(status, pi, 301); zero_words(Ro, 16); return; }                     // :451 expect("sum of deltas is zero")
  bool good = true;
  ec::Jac acc = ec::jac_inf();
  for (int j = 0; j < d.S; ++j) {
    const size_t row = (size_t)j * d.B + b;
    const ec::Aff Gj = ec::aff_load(g_gamma + row * 16);
    if (!ec::aff_valid(Gj)) { good = false; break; }                                                    // no point the reference can hold
    if (j != i) {
      const int jj = j < i ? j : j - 1;
      const ec::Aff Bp = ec::aff_load(b_pk + (((size_t)li * P1 + jj) * d.B + b) * 16);
      good = good && ec::aff_eq(Bp, Gj) && ec::u256_eq(sig::commit_point(Gj, blind + row * 8, d.enc), ec::u256_load(com + row * 8));   // :463-469
    }
    acc = ec::jac_add_aff(acc, Gj);
  }
  if (!good) { fail(status, pi, 401); zero_words(Ro, 16); return; }
  const ec::Aff Rp = ec::jac_to_aff(acc);
  const ec::Aff Rr = Rp.inf ? Rp : ec::mul_aff(ec::sc_inv(tot), Rp);                                    // :478, client :309
  if (Rr.inf) { fail(status, pi, 402); zero_words(Ro, 16); return; }                                    // R.x_coord().unwrap() would panic (:496-497)
  ec::aff_store(Ro, Rr);
}

// phase5_local_sig and phase5a_broadcast_5b_zkproof (:487-559); the DLogProof of rho_i is dlog_prove_kernel's, launched in front of
// this kernel, which wipes it for a party that has failed
__global__ void __launch_bounds__(64) MPE_EC_OCC phase5a_kernel(Dim d, const uint32_t* __restrict__ k, const uint32_t* __restrict__ sigma, const uint32_t* __restrict__ msg,
                                                                const uint32_t* __restrict__ R, const uint32_t* __restrict__ l_in, const uint32_t* __restrict__ rho_in,
                                                                const uint32_t* __restrict__ blind, const uint32_t* __restrict__ s1_in, const uint32_t* __restrict__ s2_in,
                                                                uint32_t* __restrict__ s_i, uint32_t* __restrict__ V, uint32_t* __restrict__ A, uint32_t* __restrict__ Bo,
                                                                uint32_t* __restrict__ com, mpe_heg_proof h, mpe_dlog_proof dl, const int32_t* __restrict__ status) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= d.B * d.L) return;
  const int b = pi % d.B;
  const ec::Aff Rp = ec::aff_load(R + (size_t)pi * 16);
  if (status[pi] != 0 || !ec::aff_valid(Rp)) {
    zero_words(s_i + (size_t)pi * 8, 8); zero_words(V + (size_t)pi * 16, 16); zero_words(A + (size_t)pi * 16, 16); zero_words(Bo + (size_t)pi * 16, 16);
    zero_words(com + (size_t)pi * 8, 8); zero_words(h.T + (size_t)pi * 16, 16); zero_words(h.A3 + (size_t)pi * 16, 16); zero_words(h.z1 + (size_t)pi * 8, 8);
    zero_words(h.z2 + (size_t)pi * 8, 8); zero_words(dl.pk + (size_t)pi * 16, 16); zero_words(dl.R + (size_t)pi * 16, 16); zero_words(dl.z + (size_t)pi * 8, 8);
    return;
  }
  const ec::U256 m = ec::sc_reduce(msg + (size_t)b * 8, 8), r = ec::sc_reduce(Rp.x.w, 8);                                      // :494-499
  const ec::U256 si = ec::sc_add(ec::sc_mul(m, ec::sc_reduce(k + (size_t)pi * 8, 8)), ec::sc_mul(r, ec::sc_reduce(sigma + (size_t)pi * 8, 8)));   // :500
  const ec::U256 l = ec::sc_reduce(l_in + (size_t)pi * 8, 8), rho = ec::sc_reduce(rho_in + (size_t)pi * 8, 8);
  const ec::Aff G = ec::aff_gen();
  const ec::Aff Ai = ec::jac_to_aff(ec::jac_mul_gen(rho)), Bi = ec::jac_to_aff(ec::jac_mul_gen(ec::sc_mul(l, rho)));           // :523-525
  const ec::Aff Vi = ec::jac_to_aff(ec::jac_add(ec::jac_mul(si, Rp), ec::jac_mul_gen(l)));                                     // :526
  const ec::U256 dg = sig::points_digest(d.enc, Vi, Ai, Bi);                                                                       // :527-529
  ec::u256_store(s_i + (size_t)pi * 8, si);
  ec::aff_store(V + (size_t)pi * 16, Vi);
  ec::aff_store(A + (size_t)pi * 16, Ai);
  ec::aff_store(Bo + (size_t)pi * 16, Bi);
  ec::u256_store(com + (size_t)pi * 8, sig::commit_bigint(dg.w, blind + (size_t)pi * 8, d.enc));                                // :530-533
  ec::Aff T, A3;
  ec::U256 z1, z2;                                                                                       // witness {r: l_i, x: s_i}, statement (A_i, R, g, V_i, B_i)  :534-546
  sig::heg_prove_body(si, l, ec::sc_reduce(s1_in + (size_t)pi * 8, 8), ec::sc_reduce(s2_in + (size_t)pi * 8, 8), Ai, Rp, G, Vi, Bi, d.enc, T, A3, z1, z2);
  ec::aff_store(h.T + (size_t)pi * 16, T);
  ec::aff_store(h.A3 + (size_t)pi * 16, A3);
  ec::u256_store(h.z1 + (size_t)pi * 8, z1);
  ec::u256_store(h.z2 + (size_t)pi * 8, z2);
}

struct Bc5 {                                                        // what every signer broadcast in 5A and 5B, [S][B][..]
  const uint32_t *V, *A, *B, *blind, *com, *T, *A3, *z1, *z2, *dpk, *dR, *dz;
};
// phase5c (:561-636) over the peers' decommitments, commitments and proofs, aligned as gg18_sign_client.rs:381-401
__global__ void __launch_bounds__(64) MPE_EC_OCC phase5c_kernel(Dim d, const uint32_t* __restrict__ msg, const uint32_t* __restrict__ y, const uint32_t* __restrict__ R,
                                                                const uint32_t* __restrict__ l_in, const uint32_t* __restrict__ rho_in, const uint32_t* __restrict__ blind2,
                                                                Bc5 in, uint32_t* __restrict__ u, uint32_t* __restrict__ t, uint32_t* __restrict__ com2,
                                                                int32_t* __restrict__ status) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= d.B * d.L) return;
  const int li = pi / d.B, b = pi % d.B, i = d.loc[li];
  uint32_t *uo = u + (size_t)pi * 16, *to = t + (size_t)pi * 16, *co = com2 + (size_t)pi * 8;
  const ec::Aff Rp = ec::aff_load(R + (size_t)pi * 16), Y = ec::aff_load(y + (size_t)b * 16);
  if (status[pi] == 0 && !(ec::aff_valid(Rp) && ec::aff_valid(Y))) fail(status, pi, 531);
  if (status[pi] != 0) { zero_words(uo, 16); zero_words(to, 16); zero_words(co, 8); return; }
  const ec::Aff G = ec::aff_gen();
  bool good = true;
  ec::Jac v = ec::jac_inf(), a = ec::jac_inf();
  for (int j = 0; j < d.S && good; ++j) {
    const size_t row = (size_t)j * d.B + b;
    const ec::Aff Vj = ec::aff_load(in.V + row * 16);
    if (!ec::aff_valid(Vj)) { good = false; break; }                                                    // before any secret meets it
    v = ec::jac_add_aff(v, Vj);                                                                         // :597  v_i + the peers'
    if (j == i) continue;                                                                               // of the own entry phase5c reads V_i only
    const ec::Aff Aj = ec::aff_load(in.A + row * 16), Bj = ec::aff_load(in.B + row * 16);
    if (!(ec::aff_valid(Aj) && ec::aff_valid(Bj))) { good = false; break; }
    a = ec::jac_add_aff(a, Aj);                                                                         // :599  the peers' only
    const ec::Aff T = ec::aff_load(in.T + row * 16), A3 = ec::aff_load(in.A3 + row * 16), P = ec::aff_load(in.dpk + row * 16), Rd = ec::aff_load(in.dR + row * 16);
    if (!(ec::aff_valid(T) && ec::aff_valid(A3) && ec::aff_valid(P) && ec::aff_valid(Rd))) { good = false; break; }
    const ec::U256 dg = sig::points_digest(d.enc, Vj, Aj, Bj);
    good = ec::u256_eq(sig::commit_bigint(dg.w, in.blind + row * 8, d.enc), ec::u256_load(in.com + row * 8));                   // :582-589
    good = good && sig::heg_verify_body(Aj, Rp, G, Vj, Bj, T, A3, ec::sc_reduce(in.z1 + row * 8, 8), ec::sc_reduce(in.z2 + row * 8, 8), d.enc);   // :590
    good = good && sig::dlog_verify_body(P, Rd, ec::sc_reduce(in.dz + row * 8, 8), d.enc);              // DLogProof::verify  :591
  }
  if (!good) { fail(status, pi, 531); zero_words(uo, 16); zero_words(to, 16); zero_words(co, 8); return; }
  const ec::U256 m = ec::sc_reduce(msg + (size_t)b * 8, 8), r = ec::sc_reduce(Rp.x.w, 8);                                      // :601-610
  v = ec::jac_add(v, ec::jac_neg(ec::jac_mul_gen(m)));                                                  // :612
  v = ec::jac_add(v, ec::jac_neg(ec::jac_mul(r, Y)));
  const ec::Aff va = ec::jac_to_aff(v), aa = ec::jac_to_aff(a);
  const ec::Aff ui = va.inf ? va : ec::mul_aff(ec::sc_reduce(rho_in + (size_t)pi * 8, 8), va);         // :613
  const ec::Aff ti = aa.inf ? aa : ec::mul_aff(ec::sc_reduce(l_in + (size_t)pi * 8, 8), aa);           // :614
  ec::aff_store(uo, ui);
  ec::aff_store(to, ti);
  const ec::U256 dg = sig::points_digest(d.enc, ui, ti);                                                 // :615
  ec::u256_store(co, sig::commit_bigint(dg.w, blind2 + (size_t)pi * 8, d.enc));                          // :617-620
}

// phase5d (:638-673) over all S decommitments of 5D and of 5A
__global__ void __launch_bounds__(64) MPE_EC_OCC phase5d_kernel(Dim d, const uint32_t* __restrict__ u, const uint32_t* __restrict__ t, const uint32_t* __restrict__ blind2,
                                                                const uint32_t* __restrict__ com2, const uint32_t* __restrict__ Bv, int32_t* __restrict__ status) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= d.B * d.L) return;
  if (status[pi] != 0) return;
  const int b = pi % d.B;
  bool test_com = true;
  ec::Jac tb = ec::jac_from_aff(ec::aff_gen()), us = ec::jac_inf();
  for (int j = 0; j < d.S; ++j) {
    const size_t row = (size_t)j * d.B + b;
    const ec::Aff uj = ec::aff_load(u + row * 16), tj = ec::aff_load(t + row * 16), Bj = ec::aff_load(Bv + row * 16);
    if (!(ec::aff_valid(uj) && ec::aff_valid(tj) && ec::aff_valid(Bj))) { test_com = false; break; }
    const ec::U256 dg = sig::points_digest(d.enc, uj, tj);
    test_com = test_com && ec::u256_eq(sig::commit_bigint(dg.w, blind2 + row * 8, d.enc), ec::u256_load(com2 + row * 8));       // :647-655
    tb = ec::jac_add_aff(ec::jac_add_aff(tb, tj), Bj);                                                  // :662
    us = ec::jac_add_aff(us, uj);
  }
  if (!test_com) { fail(status, pi, 541); return; }                                                     // :671
  if (!ec::jac_eq_aff(ec::jac_add(tb, ec::jac_neg(us)), ec::aff_gen())) fail(status, pi, 542);          // :663-668
}

// output_signature with its verify (:674-737): s = s_i + the peers', normalised to the low half with the recid flip; verify has no low-s rule
__global__ void __launch_bounds__(64) MPE_EC_OCC output_kernel(Dim d, const uint32_t* __restrict__ s_own, const uint32_t* __restrict__ s_all, const uint32_t* __restrict__ R,
                                                               const uint32_t* __restrict__ msg, const uint32_t* __restrict__ y, uint32_t* __restrict__ r_out,
                                                               uint32_t* __restrict__ s_out, int32_t* __restrict__ recid_out, int32_t* __restrict__ status) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= d.B * d.L) return;
  const int li = pi / d.B, b = pi % d.B, i = d.loc[li];
  zero_words(r_out + (size_t)pi * 8, 8); zero_words(s_out + (size_t)pi * 8, 8); recid_out[pi] = 0;
  if (status[pi] != 0) return;
  const ec::Aff Rp = ec::aff_load(R + (size_t)pi * 16), Y = ec::aff_load(y + (size_t)b * 16);
  if (!ec::aff_valid(Rp) || !ec::aff_valid(Y)) { fail(status, pi, 601); return; }                       // x_coord().ok_or(InvalidSig)  :682
  ec::U256 s = ec::sc_reduce(s_own + (size_t)pi * 8, 8);
  for (int j = 0; j < d.S; ++j) if (j != i) s = ec::sc_add(s, ec::sc_reduce(s_all + ((size_t)j * d.B + b) * 8, 8));            // :675
  const ec::U256 r = ec::sc_reduce(Rp.x.w, 8), ry = ec::sc_reduce(Rp.y.w, 8);
  // the recid of :697-698, the low-s flip of :699-703, invert().ok_or(InvalidSig) :715 and the check of :725-731: GG20's, one definition
  int recid;
  if (!gg::output_signature_check(s, recid, ec::sc_reduce(msg + (size_t)b * 8, 8), r, ry, y + (size_t)b * 16)) { fail(status, pi, 601); return; }
  ec::u256_store(r_out + (size_t)pi * 8, r);
  ec::u256_store(s_out + (size_t)pi * 8, s);
  recid_out[pi] = recid;
}

static bool dim_of(int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const ec::Enc& enc, Dim* d) {
  if (!h_signers || !h_local || S < 2 || S > 8 || n_local < 1 || n_local > S || batch < 0 || (long long)batch * S > (1ll << 30)) return false;
  d->B = batch; d->S = S; d->L = n_local; d->enc = enc;
  for (int j = 0; j < 8; ++j) { d->sg[j] = 0; d->loc[j] = 0; }
  for (int j = 0; j < S; ++j) {
    if (h_signers[j] < 0 || (j && h_signers[j] <= h_signers[j - 1])) return false;
    d->sg[j] = h_signers[j];
  }
  for (int j = 0; j < n_local; ++j) {
    if (h_local[j] < 0 || h_local[j] >= S || (j && h_local[j] <= h_local[j - 1])) return false;
    d->loc[j] = h_local[j];
  }
  return true;
}

}  // namespace g18
}  // namespace mpe

extern "C" {

int mpe_gg18_sign_keys(mpe_ctx* ctx, int t, int n, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_x_i,
                       const uint32_t* d_pk_vec, const uint32_t* d_k_i, const uint32_t* d_gamma_i, uint32_t* d_w_i, uint32_t* d_g_w_i, uint32_t* d_g_gamma_i,
                       uint32_t* d_g_w, int32_t* d_status, void* stream) {
  mpe::g18::Dim d;
  if (!ctx || !d_x_i || !d_pk_vec || !d_k_i || !d_gamma_i || !d_w_i || !d_g_w_i || !d_g_gamma_i || !d_g_w || !d_status || t < 1 || S <= t || S > n ||
      !mpe::g18::dim_of(S, h_signers, n_local, h_local, batch, ctx->enc, &d) || h_signers[S - 1] >= n)
    return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::g18::sign_keys_kernel, batch * n_local, st, d, d_x_i, d_k_i, d_gamma_i, d_w_i, d_g_w_i, d_g_gamma_i, d_status);
  MPE_LAUNCH_1D(mpe::g18::g_w_kernel, batch * S, st, d, n, d_pk_vec, d_g_w);
  return MPE_OK;
}

int mpe_gg18_message_b(mpe_ctx* ctx, const mpe_paillier* pk, int batch, const int32_t* d_key_idx, const uint32_t* d_b, const uint32_t* d_ca, const uint32_t* d_r,
                       const uint32_t* d_beta_tag, const uint32_t* d_nonce_b, const uint32_t* d_nonce_bt, uint32_t* d_cb, uint32_t* d_beta,
                       const mpe_dlog_proof* b_proof, const mpe_dlog_proof* beta_tag_proof, void* stream) {
  if (!ctx || !pk || !d_b || !d_ca || !d_r || !d_beta_tag || !d_nonce_b || !d_nonce_bt || !d_cb || !d_beta || !b_proof || !beta_tag_proof || batch < 0)
    return MPE_E_ARG;
  if (!d_key_idx && pk->nkeys != 1 && pk->nkeys < batch) return MPE_E_ARG;
  if (batch == 0) return MPE_OK;
  hipStream_t st = (hipStream_t)stream;
  // beta_tag mod q in the workspace (wiped with it), kept under the ciphertext's composites
  MPE_TRY(mpe::ws_begin(ctx, st));
  uint32_t* btq = mpe::ws_array<uint32_t>(ctx, (size_t)batch * 8);
  MPE_TRY(mpe::ws_ok(ctx));
  mpe::WsKeep keep(ctx->ws);
  return mpe::mta_message_b_tail(ctx, pk, batch, d_key_idx, d_b, d_ca, d_r, d_beta_tag, d_nonce_b, d_nonce_bt, btq, d_cb, d_beta, b_proof, beta_tag_proof, st);
}

int mpe_gg18_phase2(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_k_i, const uint32_t* d_gamma_i,
                    const uint32_t* d_w_i, const uint32_t* d_alpha, const uint32_t* d_beta, const uint32_t* d_miu, const uint32_t* d_ni, const uint8_t* d_ok_gamma,
                    const uint8_t* d_ok_w, const uint32_t* d_w_pk, const uint32_t* d_g_w, uint32_t* d_delta_i, uint32_t* d_sigma_i, int32_t* d_status,
                    void* stream) {
  mpe::g18::Dim d;
  if (!ctx || !d_k_i || !d_gamma_i || !d_w_i || !d_alpha || !d_beta || !d_miu || !d_ni || !d_ok_gamma || !d_ok_w || !d_w_pk || !d_g_w || !d_delta_i ||
      !d_sigma_i || !d_status || !mpe::g18::dim_of(S, h_signers, n_local, h_local, batch, ctx->enc, &d))
    return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::g18::phase2_kernel, batch * n_local, st, d, d_k_i, d_gamma_i, d_w_i, d_alpha, d_beta, d_miu, d_ni, d_ok_gamma, d_ok_w, d_w_pk, d_g_w,
                d_delta_i, d_sigma_i, d_status);
  return MPE_OK;
}

int mpe_gg18_phase4(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_delta, const uint32_t* d_b_pk,
                    const uint32_t* d_g_gamma, const uint32_t* d_blind, const uint32_t* d_com, uint32_t* d_R, int32_t* d_status, void* stream) {
  mpe::g18::Dim d;
  if (!ctx || !d_delta || !d_b_pk || !d_g_gamma || !d_blind || !d_com || !d_R || !d_status || !mpe::g18::dim_of(S, h_signers, n_local, h_local, batch, ctx->enc, &d))
    return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::g18::phase4_kernel, batch * n_local, st, d, d_delta, d_b_pk, d_g_gamma, d_blind, d_com, d_R, d_status);
  return MPE_OK;
}

int mpe_gg18_phase5a(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_k_i, const uint32_t* d_sigma_i,
                     const uint32_t* d_msg, const uint32_t* d_R, const uint32_t* d_l_i, const uint32_t* d_rho_i, const uint32_t* d_blind, const uint32_t* d_s1,
                     const uint32_t* d_s2, const uint32_t* d_nonce, uint32_t* d_s_i, uint32_t* d_V, uint32_t* d_A, uint32_t* d_B, uint32_t* d_com,
                     const mpe_heg_proof* heg, const mpe_dlog_proof* dlog, const int32_t* d_status, void* stream) {
  mpe::g18::Dim d;
  if (!ctx || !d_k_i || !d_sigma_i || !d_msg || !d_R || !d_l_i || !d_rho_i || !d_blind || !d_s1 || !d_s2 || !d_nonce || !d_s_i || !d_V || !d_A || !d_B || !d_com ||
      !heg || !dlog || !d_status || !mpe::g18::dim_of(S, h_signers, n_local, h_local, batch, ctx->enc, &d))
    return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int items = batch * n_local;
  MPE_LAUNCH_1D(mpe::dlog_prove_kernel, items, st, items, ctx->enc, d_rho_i, d_nonce, dlog->pk, dlog->R, dlog->z);                 // DLogProof::prove(&rho_i)  :545
  MPE_LAUNCH_1D(mpe::g18::phase5a_kernel, items, st, d, d_k_i, d_sigma_i, d_msg, d_R, d_l_i, d_rho_i, d_blind, d_s1, d_s2, d_s_i, d_V, d_A, d_B, d_com, *heg, *dlog,
                d_status);
  return MPE_OK;
}

int mpe_gg18_phase5c(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_msg, const uint32_t* d_y,
                     const uint32_t* d_R, const uint32_t* d_l_i, const uint32_t* d_rho_i, const uint32_t* d_blind2, const mpe_gg18_phase5b_msgs* in, uint32_t* d_u,
                     uint32_t* d_t, uint32_t* d_com2, int32_t* d_status, void* stream) {
  mpe::g18::Dim d;
  if (!ctx || !d_msg || !d_y || !d_R || !d_l_i || !d_rho_i || !d_blind2 || !in || !d_u || !d_t || !d_com2 || !d_status ||
      !mpe::g18::dim_of(S, h_signers, n_local, h_local, batch, ctx->enc, &d))
    return MPE_E_ARG;
  if (!in->V || !in->A || !in->B || !in->blind || !in->com || !in->T || !in->A3 || !in->z1 || !in->z2 || !in->dlog_pk || !in->dlog_R || !in->dlog_z) return MPE_E_ARG;
  const mpe::g18::Bc5 bc{in->V, in->A, in->B, in->blind, in->com, in->T, in->A3, in->z1, in->z2, in->dlog_pk, in->dlog_R, in->dlog_z};
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::g18::phase5c_kernel, batch * n_local, st, d, d_msg, d_y, d_R, d_l_i, d_rho_i, d_blind2, bc, d_u, d_t, d_com2, d_status);
  return MPE_OK;
}

int mpe_gg18_phase5d(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_u, const uint32_t* d_t,
                     const uint32_t* d_blind2, const uint32_t* d_com2, const uint32_t* d_B, int32_t* d_status, void* stream) {
  mpe::g18::Dim d;
  if (!ctx || !d_u || !d_t || !d_blind2 || !d_com2 || !d_B || !d_status || !mpe::g18::dim_of(S, h_signers, n_local, h_local, batch, ctx->enc, &d)) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::g18::phase5d_kernel, batch * n_local, st, d, d_u, d_t, d_blind2, d_com2, d_B, d_status);
  return MPE_OK;
}

int mpe_gg18_output_signature(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_s_own,
                              const uint32_t* d_s_all, const uint32_t* d_R, const uint32_t* d_msg, const uint32_t* d_y, uint32_t* d_r, uint32_t* d_s,
                              int32_t* d_recid, int32_t* d_status, void* stream) {
  mpe::g18::Dim d;
  if (!ctx || !d_s_own || !d_s_all || !d_R || !d_msg || !d_y || !d_r || !d_s || !d_recid || !d_status ||
      !mpe::g18::dim_of(S, h_signers, n_local, h_local, batch, ctx->enc, &d))
    return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::g18::output_kernel, batch * n_local, st, d, d_s_own, d_s_all, d_R, d_msg, d_y, d_r, d_s, d_recid, d_status);
  return MPE_OK;
}

}  // extern "C"
