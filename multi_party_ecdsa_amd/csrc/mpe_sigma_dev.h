// The transcripts of the four curv sigma proofs on secp256k1 (un-vendored curv-kzen 0.9) and of the hash
// commitments around them, as device functions: DLogProof, PedersenProof, HomoELGamalProof, ECDDHProof.  Two decisions are made here
// and nowhere else: which points enter a proof's challenge in which order (the canonical lists of include/mpecdsa_hip.h, permuted
// by enc.ord_*), and which equation its verifier accepts.  Every kernel that proves or verifies — the stand-alone entry points
// (mpe_proofs.h, mpe_sigma.h, mpe_blame.h), the GG20 rounds (mpe_gg20.h), MtA (mpe_mta.h), GG18 (mpe_gg18.h), Lindell
// (mpe_lindell_keygen.h) — calls these.  Per proof:
//   x_challenge   the caller's points placed into the canonical list, hashed in the order of enc.ord_x
//   x_holds       the acceptance equation over products that are already computed (Jacobian): what lane 0 of a lane-group kernel
//                 evaluates after its lanes have met in LDS
//   x_prove_body / x_verify_body   the whole proof for one item per lane: challenge, products, equation
// Every function is force-inlined and takes its points by reference: handing a pointer to a lane-private array to an out-of-line
// device function hung a kernel on gfx950 / ROCm 7.2.  The ladders they call stay out of line (MPE_HDN).
// Precondition of every verify body and every *_holds: all points have passed ec::aff_valid (the callers check, or validate_kernel).
#pragma once
#include "mpe_ec.h"

namespace mpe {
namespace sig {

// How a base is multiplied is a compile-time property of the call site: VAR = the variable-base ladder, GEN / H2 = the comb table of
// the generator / of base_point2 (then the point handed in must BE that generator: it still enters the challenge).
enum Base { VAR, GEN, H2 };
template <Base B>
__device__ __forceinline__ ec::Jac mul(const ec::U256& k, const ec::Aff& P) {
  if constexpr (B == GEN) return ec::jac_mul_gen(k);
  else if constexpr (B == H2) return ec::jac_mul_h2(k);
  else return ec::jac_mul(k, P);
}

// `pts` is the canonical list of the proof; `ord[i]` = which of them is hashed i-th.  The selection is a compare-and-select chain,
// never a dynamic index into the lane-private array.
template <int N>
__device__ __forceinline__ ec::U256 challenge(const ec::Aff (&pts)[N], const ec::Enc& enc, const uint8_t* ord) {
  ec::Sha256 s; ec::sha_init(s);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int o = ord[i];
    ec::Aff P = pts[0];
#pragma unroll
    for (int j = 1; j < N; ++j) if (o == j) P = pts[j];
    ec::sha_chain_point(s, P, enc);
  }
  const ec::U256 d = ec::sha_final(s);
  return ec::sc_reduce(d.w, 8);
}

// ---- DLogProof: pk = sk G, R = k G, c = H(R, G, pk) mod q, z = k - c sk;  accepts z G + c pk == R --------------------------------
__device__ __forceinline__ ec::U256 dlog_challenge(const ec::Aff& R, const ec::Aff& pk, const ec::Enc& enc) {
  const ec::Aff hp[3] = {R, ec::aff_gen(), pk};
  return challenge(hp, enc, enc.ord_dlog);
}
__device__ __forceinline__ bool dlog_holds(const ec::Jac& zG, const ec::Jac& cP, const ec::Aff& R) { return ec::jac_eq_aff(ec::jac_add(zG, cP), R); }
__device__ __forceinline__ void dlog_prove_body(const ec::U256& sk, const ec::U256& k, const ec::Enc& enc, ec::Aff& pk, ec::Aff& R, ec::U256& z) {
  R = ec::jac_to_aff(ec::jac_mul_gen(k));
  pk = ec::jac_to_aff(ec::jac_mul_gen(sk));
  z = ec::sc_sub(k, ec::sc_mul(dlog_challenge(R, pk, enc), sk));
}
__device__ __forceinline__ bool dlog_verify_body(const ec::Aff& pk, const ec::Aff& R, const ec::U256& z, const ec::Enc& enc) {
  const ec::U256 c = dlog_challenge(R, pk, enc);
  const ec::Jac zG = ec::jac_mul_gen(z), cP = ec::jac_mul(c, pk);
  return dlog_holds(zG, cP, R);
}

// ---- MessageB::verify_proofs_get_alpha after the decryption (mta/mod.rs:166-178): g^alpha == a B + B' and the DLogProofs of B, B' -
__device__ __forceinline__ bool mta_relation_holds(const ec::Jac& g_alpha, const ec::Jac& aB, const ec::Aff& Bt) {
  return ec::jac_eq(g_alpha, ec::jac_add_aff(aB, Bt));
}
__device__ __forceinline__ bool mta_alpha_holds(const ec::U256& alpha, const ec::U256& a, const ec::Aff& B, const ec::Aff& R1, const ec::U256& z1,
                                                const ec::Aff& Bt, const ec::Aff& R2, const ec::U256& z2, const ec::Enc& enc) {
  const ec::Jac g_alpha = ec::jac_mul_gen(alpha), aB = ec::jac_mul(a, B);
  const bool rel = mta_relation_holds(g_alpha, aB, Bt);
  const bool p1 = dlog_verify_body(B, R1, z1, enc), p2 = dlog_verify_body(Bt, R2, z2, enc);
  return rel && p1 && p2;
}

// ---- PedersenProof over (g, h) = (G, base_point2), party_i.rs:620-634: com = m g + r h, a1 = s1 g, a2 = s2 h, e = H(g, h, com, a1, a2),
// z1 = s1 + e m, z2 = s2 + e r;  accepts z1 g + z2 h == e com + a1 + a2 ------------------------------------------------------------------
__device__ __forceinline__ ec::U256 pedersen_challenge(const ec::Aff& com, const ec::Aff& a1, const ec::Aff& a2, const ec::Enc& enc) {
  const ec::Aff hp[5] = {ec::aff_gen(), ec::aff_h2(), com, a1, a2};
  return challenge(hp, enc, enc.ord_pedersen);
}
__device__ __forceinline__ bool pedersen_holds(const ec::Jac& z1G, const ec::Jac& z2H, const ec::Jac& eC, const ec::Aff& a1, const ec::Aff& a2) {
  return ec::jac_eq(ec::jac_add(z1G, z2H), ec::jac_add_aff(ec::jac_add_aff(eC, a1), a2));
}
// com, a1, a2 are the caller's (fixed-base products of its own scalars: GG20 computes them ahead of the round, ped_ahead_kernel)
__device__ __forceinline__ void pedersen_prove_body(const ec::U256& m, const ec::U256& r, const ec::U256& s1, const ec::U256& s2, const ec::Aff& com,
                                                    const ec::Aff& a1, const ec::Aff& a2, const ec::Enc& enc, ec::U256& e, ec::U256& z1, ec::U256& z2) {
  e = pedersen_challenge(com, a1, a2, enc);
  z1 = ec::sc_add(s1, ec::sc_mul(e, m));
  z2 = ec::sc_add(s2, ec::sc_mul(e, r));
}
__device__ __forceinline__ bool pedersen_verify_body(const ec::Aff& com, const ec::Aff& a1, const ec::Aff& a2, const ec::U256& z1, const ec::U256& z2,
                                                     const ec::Enc& enc) {
  const ec::U256 e = pedersen_challenge(com, a1, a2, enc);
  const ec::Jac z1G = ec::jac_mul_gen(z1), z2H = ec::jac_mul_h2(z2), eC = ec::jac_mul(e, com);
  return pedersen_holds(z1G, z2H, eC, a1, a2);
}

// ---- HomoELGamalProof over the statement (G, H, Y, D, E), witness (x, r), party_i.rs:778-833: A3 = s2 G, T = s1 H + s2 Y,
// e = H(T, A3, G, H, Y, D, E), z1 = s1 + e x (s1 when x = 0), z2 = s2 + e r;  accepts z1 H + z2 Y == e D + T and z2 G == e E + A3 ------
__device__ __forceinline__ ec::U256 heg_challenge(const ec::Aff& T, const ec::Aff& A3, const ec::Aff& G, const ec::Aff& H, const ec::Aff& Y,
                                                  const ec::Aff& D, const ec::Aff& E, const ec::Enc& enc) {
  const ec::Aff hp[7] = {T, A3, G, H, Y, D, E};
  return challenge(hp, enc, enc.ord_heg);
}
__device__ __forceinline__ bool heg_holds(const ec::Jac& z1H, const ec::Jac& z2Y, const ec::Jac& eD, const ec::Aff& T, const ec::Jac& z2G,
                                          const ec::Jac& eE, const ec::Aff& A3) {
  return ec::jac_eq(ec::jac_add(z1H, z2Y), ec::jac_add_aff(eD, T)) && ec::jac_eq(z2G, ec::jac_add_aff(eE, A3));
}
template <Base BG = VAR, Base BH = VAR, Base BY = VAR>
__device__ __forceinline__ void heg_prove_body(const ec::U256& x, const ec::U256& r, const ec::U256& s1, const ec::U256& s2, const ec::Aff& G,
                                               const ec::Aff& H, const ec::Aff& Y, const ec::Aff& D, const ec::Aff& E, const ec::Enc& enc,
                                               ec::Aff& T, ec::Aff& A3, ec::U256& z1, ec::U256& z2) {
  A3 = ec::jac_to_aff(mul<BG>(s2, G));
  T = ec::jac_to_aff(ec::jac_add(mul<BH>(s1, H), mul<BY>(s2, Y)));
  const ec::U256 e = heg_challenge(T, A3, G, H, Y, D, E, enc);
  z1 = ec::u256_is_zero(x) ? s1 : ec::sc_add(s1, ec::sc_mul(e, x));
  z2 = ec::sc_add(s2, ec::sc_mul(e, r));
}
template <Base BG = VAR, Base BH = VAR, Base BY = VAR>
__device__ __forceinline__ bool heg_verify_body(const ec::Aff& G, const ec::Aff& H, const ec::Aff& Y, const ec::Aff& D, const ec::Aff& E, const ec::Aff& T,
                                                const ec::Aff& A3, const ec::U256& z1, const ec::U256& z2, const ec::Enc& enc) {
  const ec::U256 e = heg_challenge(T, A3, G, H, Y, D, E, enc);
  const ec::Jac z1H = mul<BH>(z1, H), z2Y = mul<BY>(z2, Y), eD = ec::jac_mul(e, D);
  const ec::Jac z2G = mul<BG>(z2, G), eE = ec::jac_mul(e, E);
  return heg_holds(z1H, z2Y, eD, T, z2G, eE, A3);
}

// ---- ECDDHProof over (g1, h1, g2, h2), witness x (h1 = x g1, h2 = x g2), blame.rs:258-320: a1 = s g1, a2 = s g2,
// e = H(g1, h1, g2, h2, a1, a2), z = s + e x;  accepts z g1 == e h1 + a1 and z g2 == e h2 + a2.  The two sides are the same equation:
// ecddh_holds is ONE side, so that a verifier keeps the second pair of ladders behind the first comparison's && ---------------------
__device__ __forceinline__ ec::U256 ecddh_challenge(const ec::Aff& g1, const ec::Aff& h1, const ec::Aff& g2, const ec::Aff& h2, const ec::Aff& a1,
                                                    const ec::Aff& a2, const ec::Enc& enc) {
  const ec::Aff hp[6] = {g1, h1, g2, h2, a1, a2};
  return challenge(hp, enc, enc.ord_ecddh);
}
__device__ __forceinline__ bool ecddh_holds(const ec::Jac& zg, const ec::Jac& eh, const ec::Aff& a) { return ec::jac_eq(zg, ec::jac_add_aff(eh, a)); }
template <Base B1 = VAR, Base B2 = VAR>
__device__ __forceinline__ void ecddh_prove_body(const ec::U256& x, const ec::U256& s, const ec::Aff& g1, const ec::Aff& h1, const ec::Aff& g2,
                                                 const ec::Aff& h2, const ec::Enc& enc, ec::Aff& a1, ec::Aff& a2, ec::U256& z) {
  a1 = ec::jac_to_aff(mul<B1>(s, g1));
  a2 = ec::jac_to_aff(mul<B2>(s, g2));
  z = ec::sc_add(s, ec::sc_mul(ecddh_challenge(g1, h1, g2, h2, a1, a2, enc), x));
}
template <Base B1 = VAR, Base B2 = VAR>
__device__ __forceinline__ bool ecddh_verify_body(const ec::Aff& g1, const ec::Aff& h1, const ec::Aff& g2, const ec::Aff& h2, const ec::Aff& a1,
                                                  const ec::Aff& a2, const ec::U256& z, const ec::Enc& enc) {
  const ec::U256 e = ecddh_challenge(g1, h1, g2, h2, a1, a2, enc);
  return ecddh_holds(mul<B1>(z, g1), ec::jac_mul(e, h1), a1) && ecddh_holds(mul<B2>(z, g2), ec::jac_mul(e, h2), a2);
}

// ---- commitments and digests -----------------------------------------------------------------------------------------------------
// HashCommitment(compressed point as BigInt, blind)  (party_i.rs:577-580)
__device__ __forceinline__ ec::U256 commit_point(const ec::Aff& P, const uint32_t* blind, const ec::Enc& enc) {
  ec::Sha256 s; ec::sha_init(s);
  ec::sha_point_compressed(s, P);
  ec::sha_bigint(s, blind, 8, enc);
  return ec::sha_final(s);
}
// HashCommitment::create_commitment_with_user_defined_randomness(m, blind) for a 256-bit m: SHA-256 over BigInt::to_bytes of both
// (minimal big-endian bytes; what zero gives is enc.zero_bytes) — the rule commit_point applies to its blind factor
__device__ __forceinline__ ec::U256 commit_bigint(const uint32_t* m, const uint32_t* blind, const ec::Enc& enc) {
  ec::Sha256 s; ec::sha_init(s);
  ec::sha_bigint(s, m, 8, enc);
  ec::sha_bigint(s, blind, 8, enc);
  return ec::sha_final(s);
}
// Sha256::new().chain_points([p...]).result_bigint(): the digest as an integer, NOT reduced mod q (lindell_2017/party_two.rs:347-349
// over two points, gg_2018/party_i.rs:527-529 over three)
template <class... P>
__device__ __forceinline__ ec::U256 points_digest(const ec::Enc& enc, const P&... pts) {
  ec::Sha256 s; ec::sha_init(s);
  (ec::sha_chain_point(s, pts, enc), ...);
  return ec::sha_final(s);
}

}  // namespace sig
}  // namespace mpe
