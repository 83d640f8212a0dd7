// Keygen, the part that MAKES a wallet (src/protocols/multi_party_ecdsa/gg_2020/party_i.rs):
//   :260-320  the dealing at the end of phase1_verify_com_phase3_verify_correct_key_verify_dlog_phase2_distribute:
//             VerifiableSS::share(t, n, &u_i)                                                          -> mpe_vss_share
//   :355-363  the OK branch of phase2_verify_vss_construct_keypair_phase3_pok_dlog: y = sum y_j, x_i = sum of the received
//             shares, DLogProof::prove(&x_i)                                                           -> mpe_keygen_construct_keypair
//   :405-438  verify_dlog_proofs_check_against_vss with get_commitments_to_xi (:369-388)                -> mpe_keygen_verify_round3
// The verdicts of rounds 1 and 2 and the Feldman check of ONE (party, dealer) pair are in mpe_keygen.h.  What differs here from
// composing mpe_vss_point_commitment + mpe_ec_add + mpe_dlog_verify by hand: the commitment to x_i is the value, at i, of the SUM of
// the dealers' polynomials, so the n polynomials of a session are added once (r3_global_kernel, one lane per coefficient) and every
// party evaluates that one polynomial (r3_verdict_kernel) — t1 (n - 1) additions per session plus one Horner pass per party instead
// of n Horner passes per party — and the Horner step multiplies by the party index along the index's own bits (jac_mul_small: at most
// 5 doublings for the 32 parties a bad-actor mask holds) instead of through the 130 doublings of the full-width ladder.
// Included by mpe_lib.hip.
#pragma once
#include "mpe_keygen.h"

namespace mpe {
namespace kg {

// shares[b][j] = f_b(j + 1) mod q for f_b = sum_k coef[b][k] X^k (Horner), one (dealer, receiver) per lane
__global__ void __launch_bounds__(64) vss_eval_kernel(int B, int t1, int n, const uint32_t* __restrict__ coef, uint32_t* __restrict__ shares) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= B * n) return;
  const int b = g / n;
  ec::U256 idx = ec::u256_zero();
  idx.w[0] = (uint32_t)(g % n + 1);
  ec::U256 acc = ec::u256_zero();
  for (int k = t1 - 1; k >= 0; --k) acc = ec::sc_add(ec::sc_mul(acc, idx), ec::sc_reduce(coef + ((size_t)b * t1 + k) * 8, 8));
  ec::u256_store(shares + (size_t)g * 8, acc);
}

// x = sum_j shares[i][j] mod q, ysum = sum_j y[i][j]; one (session, receiving party) per lane.  jac_add_aff is exact for equal
// summands, for P + (-P) and for neutral operands on either side.
__global__ void __launch_bounds__(64) MPE_EC_OCC construct_sum_kernel(int B, int n, const uint32_t* __restrict__ shares, const uint32_t* __restrict__ y,
                                                                      uint32_t* __restrict__ x, uint32_t* __restrict__ ysum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  ec::U256 s = ec::u256_zero();
  ec::Jac acc = ec::jac_inf();
  for (int j = 0; j < n; ++j) {
    s = ec::sc_add(s, ec::sc_reduce(shares + ((size_t)i * n + j) * 8, 8));
    acc = ec::jac_add_aff(acc, ec::aff_load(y + ((size_t)i * n + j) * 16));
  }
  ec::u256_store(x + (size_t)i * 8, s);
  ec::aff_store(ysum + (size_t)i * 16, ec::jac_to_aff(acc));
}

// m P for a small m >= 1, along m's own bits (double-and-add from the top bit down); exact for every P, the neutral element included
__device__ inline ec::Jac jac_mul_small(uint32_t m, const ec::Jac& p) {
  ec::Jac r = p;
#pragma unroll 1
  for (int b = 30 - __clz((int)m); b >= 0; --b) {
    r = ec::jac_dbl(r);
    if ((m >> b) & 1u) r = ec::jac_add(r, p);
  }
  return r;
}

// the global polynomial of a session: glob[s][k] = sum_j commits[s][j][k], one (session, coefficient) per lane.  A row that is not a
// valid point is left out of the sum and marks its session (sess_bad[s] != 0).
__global__ void __launch_bounds__(64) MPE_EC_OCC r3_global_kernel(int S, int n, int t1, const uint32_t* __restrict__ commits, uint32_t* __restrict__ glob,
                                                                  uint32_t* __restrict__ sess_bad) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= S * t1) return;
  const int s = g / t1, k = g % t1;
  ec::Jac acc = ec::jac_inf();
  bool valid = true;
  for (int j = 0; j < n; ++j) {
    const ec::Aff c = ec::aff_load(commits + (((size_t)s * n + j) * t1 + k) * 16);
    const bool v = ec::aff_valid(c);
    valid = valid && v;
    if (v) acc = ec::jac_add_aff(acc, c);
  }
  ec::aff_store(glob + (size_t)g * 16, ec::jac_to_aff(acc));
  if (!valid) atomicOr(sess_bad + s, 1u);
}
// verify_dlog_proofs_check_against_vss for item (s, i): xi_commit = sum_k (i + 1)^k glob[s][k] (Horner), ok = DLogProof::verify (dl_ok, from
// dlog_verify_kernel) && xi_commit == pk && the session's commitments are all valid points
__global__ void __launch_bounds__(64) MPE_EC_OCC r3_verdict_kernel(int B, int n, int t1, const uint32_t* __restrict__ glob, const uint32_t* __restrict__ sess_bad,
                                                                   const uint32_t* __restrict__ pk, const uint8_t* __restrict__ dl_ok, uint8_t* __restrict__ ok,
                                                                   uint32_t* __restrict__ bad, uint32_t* __restrict__ xi_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const int s = i / n;
  const uint32_t m = (uint32_t)(i % n + 1);
  ec::Jac acc = ec::jac_inf();
  for (int k = t1 - 1; k >= 0; --k) {
    if (!ec::jac_is_inf(acc)) acc = jac_mul_small(m, acc);
    acc = ec::jac_add_aff(acc, ec::aff_load(glob + ((size_t)s * t1 + k) * 16));
  }
  const bool sbad = sess_bad[s] != 0;
  const bool v = dl_ok[i] && !sbad && ec::jac_eq_aff(acc, ec::aff_load(pk + (size_t)i * 16));
  ok[i] = v ? 1 : 0;
  if (!v && bad) atomicOr(bad + s, 1u << (i % n));
  if (xi_out) ec::aff_store(xi_out + (size_t)i * 16, ec::jac_to_aff(sbad ? ec::jac_inf() : acc));
}
}  // namespace kg
}  // namespace mpe

extern "C" {

// `VerifiableSS::share(t, n, &u_i)`: commitments through the comb tables of G (ec_mul_kernel without a point), shares by Horner
int mpe_vss_share(mpe_ctx* ctx, int batch, int t1, int n, const uint32_t* d_coef, uint32_t* d_commits, uint32_t* d_shares, void* stream) {
  if (!ctx || !d_coef || !d_commits || !d_shares || batch < 0 || t1 < 1 || t1 > 64 || n < 1 || n > 65535) return MPE_E_ARG;
  if ((int64_t)batch * t1 > INT32_MAX || (int64_t)batch * n > INT32_MAX) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::ec_mul_kernel, batch * t1, st, batch * t1, d_coef, 8, (const uint32_t*)nullptr, d_commits);
  MPE_LAUNCH_1D(mpe::kg::vss_eval_kernel, batch * n, st, batch, t1, n, d_coef, d_shares);
  return MPE_OK;
}

// the OK branch of `Keys::phase2_verify_vss_construct_keypair_phase3_pok_dlog` (party_i.rs:355-363); the proof is dlog_prove_kernel's
int mpe_keygen_construct_keypair(mpe_ctx* ctx, int batch, int n, const uint32_t* d_shares, const uint32_t* d_y, const uint32_t* d_nonce, uint32_t* d_x,
                                 uint32_t* d_ysum, uint32_t* d_pk, uint32_t* d_R, uint32_t* d_z, void* stream) {
  if (!ctx || !d_shares || !d_y || !d_nonce || !d_x || !d_ysum || !d_pk || !d_R || !d_z || batch < 0 || n < 1 || n > 65535) return MPE_E_ARG;
  if ((int64_t)batch * n > INT32_MAX) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  MPE_LAUNCH_1D(mpe::kg::construct_sum_kernel, batch, st, batch, n, d_shares, d_y, d_x, d_ysum);
  MPE_LAUNCH_1D(mpe::dlog_prove_kernel, batch, st, batch, ctx->enc, d_x, d_nonce, d_pk, d_R, d_z);
  return MPE_OK;
}

// `Keys::verify_dlog_proofs_check_against_vss` (party_i.rs:405-438) as the reference composes it
int mpe_keygen_verify_round3(mpe_ctx* ctx, int batch, int n_parties, int t1, const uint32_t* d_commits, const uint32_t* d_pk, const uint32_t* d_R,
                             const uint32_t* d_z, uint8_t* d_ok, uint32_t* d_bad_actors, uint32_t* d_xi_commit, void* stream) {
  using namespace mpe;
  if (!ctx || !d_commits || !d_pk || !d_R || !d_z || !d_ok || batch < 0 || n_parties < 1 || n_parties > 32 || batch % n_parties || t1 < 1 || t1 > 64) return MPE_E_ARG;
  if ((int64_t)(batch / n_parties) * t1 > INT32_MAX) return MPE_E_ARG;
  if (batch == 0) return MPE_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = batch / n_parties;
  MPE_TRY(ws_begin(ctx, st));
  uint32_t *glob = ws_array<uint32_t>(ctx, (size_t)S * t1 * 16), *sess_bad = ws_array<uint32_t>(ctx, (size_t)S);
  uint8_t* dl_ok = ws_array<uint8_t>(ctx, (size_t)batch);
  MPE_TRY(ws_ok(ctx));
  (void)hipMemsetAsync(sess_bad, 0, (size_t)S * 4, st);
  if (d_bad_actors) (void)hipMemsetAsync(d_bad_actors, 0, (size_t)S * 4, st);
  MPE_LAUNCH_1D(dlog_verify_kernel, batch, st, batch, ctx->enc, d_pk, d_R, d_z, dl_ok);                     // :419, the device code of mpe_dlog_verify
  MPE_LAUNCH_1D(kg::r3_global_kernel, S * t1, st, S, n_parties, t1, d_commits, glob, sess_bad);             // :373-381, once per session
  MPE_LAUNCH_1D(kg::r3_verdict_kernel, batch, st, batch, n_parties, t1, glob, sess_bad, d_pk, dl_ok, d_ok, d_bad_actors, d_xi_commit);   // :383-385, :420
  return MPE_OK;
}

}  // extern "C"
