// Test-only device library: the one-item-per-lane layer (csrc/mpe_fe.h, mpe_sc.h, mpe_jac.h, the SHA-256 and comb table of mpe_ec.h,
// the word helpers of mpe_small.h) behind a batched C interface, so that tests/test_fe_gpu.py can run the case tables of
// tests/fe_cases.py WHERE THE CODE RUNS: compiled by hipcc for gfx950 with the product's flags, the ladders / inversions / GLV split as
// out-of-line callees (MPE_HDN) of kernels capped by MPE_EC_OCC, the loops under `#pragma unroll 1`.  The device twin of
// tools/model/fe_host.cpp: the same operations under the same names (ecd_ for feh_ / ech_ / sch_), one row per lane.
//   hipcc <HIPCC_FLAGS of __graft_entry__.py> -shared tests/hip/ec_dev.hip -o tests/hip/libec_dev.so        (tests/hip_build.py)
// The product library links none of this.
//
// Every row operation has ONE signature: (rows, up to five input columns, up to three output columns, arg) -- raw device pointers,
// rows of the fixed widths tests/fe_cases.py:OPS states; it launches one kernel of 64-thread blocks on the null stream, waits for it
// and returns the HIP error code.  The kernels keep the house discipline: operands are loaded into values and handed on by value or
// reference; no pointer to a lane-private array reaches an out-of-line function (jac_mul_comb and sc_reduce get pointers to global
// memory, as in the product).
#include "../../multi_party_ecdsa_amd/csrc/mpe_ec.h"
#include "../../multi_party_ecdsa_amd/csrc/mpe_small.h"
using namespace mpe::ec;
namespace sm = mpe::sm;

#define ECD_NO_OCC
#define ECD_IN const uint32_t* __restrict__
#define ECD_OUT uint32_t* __restrict__
// body: `i` is the row; i0..i4, o0..o2 and arg are the entry's arguments
#define ECD_ROW_OP(name, OCC, ...)                                                                                                     \
  __global__ void __launch_bounds__(64) OCC k_##name(int n, ECD_IN i0, ECD_IN i1, ECD_IN i2, ECD_IN i3, ECD_IN i4, ECD_OUT o0,          \
                                                     ECD_OUT o1, ECD_OUT o2, int arg) {                                                 \
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;                                                                             \
    if (i >= (size_t)n) return;                                                                                                         \
    __VA_ARGS__                                                                                                                         \
  }                                                                                                                                     \
  extern "C" int ecd_##name(int n, const uint32_t* i0, const uint32_t* i1, const uint32_t* i2, const uint32_t* i3, const uint32_t* i4,  \
                            uint32_t* o0, uint32_t* o1, uint32_t* o2, int arg) {                                                        \
    if (n < 0 || !ecd_arg_ok_##name(arg)) return (int)hipErrorInvalidValue;                                                             \
    return ecd_run(n, [&](dim3 g) { hipLaunchKernelGGL(k_##name, g, dim3(64), 0, 0, n, i0, i1, i2, i3, i4, o0, o1, o2, arg); });        \
  }
#define ECD_ANY_ARG(name) static bool ecd_arg_ok_##name(int) { return true; }

template <class F>
static int ecd_run(int n, F launch) {
  if (n > 0) launch(dim3((unsigned)((n + 63) / 64)));
  const hipError_t e = hipGetLastError();
  return (int)(e != hipSuccess ? e : hipDeviceSynchronize());
}

__device__ __forceinline__ Fe fe_load(const uint32_t* p) { Fe r; for (int j = 0; j < 10; ++j) r.n[j] = p[j]; return r; }
__device__ __forceinline__ void fe_store(uint32_t* p, const Fe& a) { for (int j = 0; j < 10; ++j) p[j] = a.n[j]; }
__device__ __forceinline__ void fe_store_words(uint32_t* p, const Fe& a) { u256_store(p, fe_to_u256(fe_normalize(a))); }

// ---- base field: limbs in (any magnitude the caller likes), canonical words and / or raw limbs out ------------------------------------
ECD_ANY_ARG(feh_mul) ECD_ROW_OP(feh_mul, ECD_NO_OCC, const Fe r = fe_mul(fe_load(i0 + i * 10), fe_load(i1 + i * 10)); fe_store_words(o0 + i * 8, r); fe_store(o1 + i * 10, r);)
ECD_ANY_ARG(feh_sqr) ECD_ROW_OP(feh_sqr, ECD_NO_OCC, const Fe r = fe_sqr(fe_load(i0 + i * 10)); fe_store_words(o0 + i * 8, r); fe_store(o1 + i * 10, r);)
ECD_ANY_ARG(feh_weak) ECD_ROW_OP(feh_weak, ECD_NO_OCC, fe_store(o0 + i * 10, fe_weak(fe_load(i0 + i * 10)));)
ECD_ANY_ARG(feh_normalize) ECD_ROW_OP(feh_normalize, ECD_NO_OCC, fe_store_words(o0 + i * 8, fe_load(i0 + i * 10));)
ECD_ANY_ARG(feh_is_zero) ECD_ROW_OP(feh_is_zero, ECD_NO_OCC, o0[i] = fe_is_zero(fe_load(i0 + i * 10)) ? 1u : 0u;)
ECD_ANY_ARG(feh_neg) ECD_ROW_OP(feh_neg, ECD_NO_OCC, fe_store(o0 + i * 10, fe_neg(fe_load(i0 + i * 10), i1[i]));)
ECD_ANY_ARG(feh_from_words) ECD_ROW_OP(feh_from_words, ECD_NO_OCC, fe_store(o0 + i * 10, fe_from_u256(u256_load(i0 + i * 8)));)
ECD_ANY_ARG(feh_inv) ECD_ROW_OP(feh_inv, MPE_EC_OCC, fe_store_words(o0 + i * 8, fe_inv(fe_load(i0 + i * 10)));)
ECD_ANY_ARG(feh_add) ECD_ROW_OP(feh_add, ECD_NO_OCC, fe_store(o0 + i * 10, fe_add(fe_load(i0 + i * 10), fe_load(i1 + i * 10)));)
ECD_ANY_ARG(feh_sub) ECD_ROW_OP(feh_sub, ECD_NO_OCC, fe_store(o0 + i * 10, fe_sub(fe_load(i0 + i * 10), fe_load(i1 + i * 10), i2[i]));)
ECD_ANY_ARG(feh_mul_int) ECD_ROW_OP(feh_mul_int, ECD_NO_OCC, fe_store(o0 + i * 10, fe_mul_int(fe_load(i0 + i * 10), i1[i]));)
ECD_ANY_ARG(feh_eq) ECD_ROW_OP(feh_eq, ECD_NO_OCC, o0[i] = fe_eq(fe_load(i0 + i * 10), fe_load(i1 + i * 10), i2[i]) ? 1u : 0u;)

// ---- points: x[8] | y[8] rows, all-zero = infinity ------------------------------------------------------------------------------------
ECD_ANY_ARG(ech_mul) ECD_ROW_OP(ech_mul, MPE_EC_OCC, aff_store(o0 + i * 16, jac_to_aff(jac_mul(u256_load(i0 + i * 8), aff_load(i1 + i * 16))));)
ECD_ANY_ARG(ech_mul_w4) ECD_ROW_OP(ech_mul_w4, MPE_EC_OCC, aff_store(o0 + i * 16, jac_to_aff(jac_mul_w4(u256_load(i0 + i * 8), aff_load(i1 + i * 16))));)
ECD_ANY_ARG(ech_add) ECD_ROW_OP(ech_add, MPE_EC_OCC, aff_store(o0 + i * 16, jac_to_aff(jac_add_aff(jac_from_aff(aff_load(i0 + i * 16)), aff_load(i1 + i * 16))));)
// (a P) + (b Q) through the general Jacobian addition
ECD_ANY_ARG(ech_add_jac) ECD_ROW_OP(ech_add_jac, MPE_EC_OCC,
  const Jac p = jac_mul(u256_load(i0 + i * 8), aff_load(i1 + i * 16));
  const Jac q = jac_mul(u256_load(i2 + i * 8), aff_load(i3 + i * 16));
  aff_store(o0 + i * 16, jac_to_aff(jac_add(p, q)));)
ECD_ANY_ARG(ech_eq) ECD_ROW_OP(ech_eq, MPE_EC_OCC,
  const Jac j = jac_mul(u256_load(i0 + i * 8), aff_load(i1 + i * 16));
  const Aff q = aff_load(i2 + i * 16);
  o0[i] = (jac_eq_aff(j, q) ? 1u : 0u) | (jac_eq(j, jac_from_aff(q)) ? 2u : 0u);)
// jac_eq of (a P) and (b Q): two ladder outputs (i4 != 0), or P and Q as they are (Z = 1)
ECD_ANY_ARG(ech_eq_jac) ECD_ROW_OP(ech_eq_jac, MPE_EC_OCC,
  const Aff P = aff_load(i1 + i * 16); const Aff Q = aff_load(i3 + i * 16);
  const bool ladder = i4[i] != 0;
  const Jac p = ladder ? jac_mul(u256_load(i0 + i * 8), P) : jac_from_aff(P);
  const Jac q = ladder ? jac_mul(u256_load(i2 + i * 8), Q) : jac_from_aff(Q);
  o0[i] = jac_eq(p, q) ? 1u : 0u;)
ECD_ANY_ARG(ech_on_curve) ECD_ROW_OP(ech_on_curve, ECD_NO_OCC, o0[i] = aff_on_curve(aff_load(i0 + i * 16)) ? 1u : 0u;)
// o0 = -J, o1 = J + (-J), for J = k P out of the ladder (Y of magnitude 3; i2 != 0) or J = P as it is (Z = 1)
ECD_ANY_ARG(ech_neg) ECD_ROW_OP(ech_neg, MPE_EC_OCC,
  const Aff P = aff_load(i1 + i * 16);
  const Jac j = i2[i] != 0 ? jac_mul(u256_load(i0 + i * 8), P) : jac_from_aff(P);
  const Jac m = jac_neg(j);
  aff_store(o0 + i * 16, jac_to_aff(m)); aff_store(o1 + i * 16, jac_to_aff(jac_add(j, m)));)
// k G (arg = 0) or k base_point2 (arg = 1) from this library's own COMB, which ecd_comb_build fills
static bool ecd_arg_ok_ech_mul_comb(int arg) { return arg == 0 || arg == 1; }
ECD_ROW_OP(ech_mul_comb, MPE_EC_OCC, aff_store(o0 + i * 16, jac_to_aff(jac_mul_fixed(u256_load(i0 + i * 8), arg)));)

__global__ void __launch_bounds__(64) k_comb_copy(uint32_t* __restrict__ out) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e < 2 * 64 * 15 * 20) out[e] = (&COMB[0][0][0][0])[e];
}
extern "C" int ecd_comb_build(void) {
  return ecd_run(1, [&](dim3) { hipLaunchKernelGGL(ec_comb_build_kernel, dim3(2), dim3(64), 0, 0); });
}
// out: 2 x 64 x 15 x 20 words
extern "C" int ecd_comb_copy(uint32_t* out) {
  return ecd_run(1, [&](dim3) { hipLaunchKernelGGL(k_comb_copy, dim3(2 * 64 * 15 * 20 / 64), dim3(64), 0, 0, out); });
}

// ---- scalar field -----------------------------------------------------------------------------------------------------------------------
ECD_ANY_ARG(sch_split) ECD_ROW_OP(sch_split, MPE_EC_OCC,
  const GlvSplit s = sc_split_lambda(u256_load(i0 + i * 8));
  u256_store(o0 + i * 8, s.r1); u256_store(o1 + i * 8, s.r2); o2[i * 2] = s.neg1 ? 1u : 0u; o2[i * 2 + 1] = s.neg2 ? 1u : 0u;)
// rows of `arg` words, 1 .. 90
static bool ecd_arg_ok_sch_reduce(int arg) { return arg >= 1 && arg <= 90; }
ECD_ROW_OP(sch_reduce, ECD_NO_OCC, u256_store(o0 + i * 8, sc_reduce(i0 + i * (size_t)arg, arg));)
ECD_ANY_ARG(sch_mul) ECD_ROW_OP(sch_mul, ECD_NO_OCC, u256_store(o0 + i * 8, sc_mul(u256_load(i0 + i * 8), u256_load(i1 + i * 8)));)
ECD_ANY_ARG(sch_inv) ECD_ROW_OP(sch_inv, MPE_EC_OCC, u256_store(o0 + i * 8, sc_inv(u256_load(i0 + i * 8)));)
ECD_ANY_ARG(sch_add) ECD_ROW_OP(sch_add, ECD_NO_OCC, u256_store(o0 + i * 8, sc_add(u256_load(i0 + i * 8), u256_load(i1 + i * 8)));)
ECD_ANY_ARG(sch_sub) ECD_ROW_OP(sch_sub, ECD_NO_OCC, u256_store(o0 + i * 8, sc_sub(u256_load(i0 + i * 8), u256_load(i1 + i * 8)));)
ECD_ANY_ARG(sch_neg) ECD_ROW_OP(sch_neg, ECD_NO_OCC, u256_store(o0 + i * 8, sc_neg(u256_load(i0 + i * 8)));)

// ---- SHA-256 (device only) --------------------------------------------------------------------------------------------------------------
// A chain of up to 14 big-integer fields per row, used as hash_kernel (csrc/mpe_proofs.h) uses sha_init / sha_bigint / sha_final.
// desc: 43 words per row -- the number of fields, then (word offset into data, nwords, plus1) per field; plus1 hashes the value + 1
// out of nwords + 1 words (HF_BIGINT_PLUS1).  A row whose descriptor points outside data[0 .. data_words) gets an all-ones digest.
constexpr int ECD_SHA_FIELDS = 14, ECD_SHA_DESC = 1 + 3 * ECD_SHA_FIELDS;
__global__ void __launch_bounds__(64) MPE_EC_OCC k_sha_bigints(int n, Enc enc, const uint32_t* __restrict__ data, uint32_t data_words,
                                                               const uint32_t* __restrict__ desc, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= (size_t)n) return;
  const uint32_t* d = desc + i * ECD_SHA_DESC;
  bool ok = d[0] <= (uint32_t)ECD_SHA_FIELDS;
  for (uint32_t k = 0; ok && k < d[0]; ++k) {
    const uint32_t off = d[1 + 3 * k], nw = d[2 + 3 * k];
    ok = nw >= 1 && nw <= 129 && off <= data_words && nw <= data_words - off;
  }
  if (!ok) { for (int j = 0; j < 8; ++j) out[i * 8 + j] = 0xFFFFFFFFu; return; }
  Sha256 s;
  sha_init(s);
  for (uint32_t k = 0; k < d[0]; ++k) {
    const uint32_t* p = data + d[1 + 3 * k];
    const int words = (int)d[2 + 3 * k];
    if (d[3 + 3 * k]) {
      uint32_t t[130];
      const uint32_t one[1] = {1};
      t[words] = sm::add(t, words, p, words, one, 1);
      sha_bigint(s, t, words + 1, enc);
    } else {
      sha_bigint(s, p, words, enc);
    }
  }
  u256_store(out + i * 8, sha_final(s));
}
static Enc ecd_enc(int zero_bytes, int chain_point) {
  Enc e = {};
  e.zero_bytes = (uint8_t)zero_bytes; e.chain_point = (uint8_t)chain_point;
  return e;
}
extern "C" int ecd_sha_bigints(int n, const uint32_t* data, uint32_t data_words, const uint32_t* desc, uint32_t* out, int zero_bytes) {
  if (n < 0 || (zero_bytes != 0 && zero_bytes != 1)) return (int)hipErrorInvalidValue;
  const Enc enc = ecd_enc(zero_bytes, 0);
  return ecd_run(n, [&](dim3 g) { hipLaunchKernelGGL(k_sha_bigints, g, dim3(64), 0, 0, n, enc, data, data_words, desc, out); });
}
// cnt[i] <= max_pts points per row (rows of max_pts x 16 words): chain = H(sha_chain_point of each, in the form enc.chain_point names),
// comp = H(sha_point_compressed of each)
__global__ void __launch_bounds__(64) MPE_EC_OCC k_sha_points(int n, Enc enc, const uint32_t* __restrict__ pts, int max_pts, const uint32_t* __restrict__ cnt,
                                                              uint32_t* __restrict__ chain, uint32_t* __restrict__ comp) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= (size_t)n) return;
  const int c = cnt[i] <= (uint32_t)max_pts ? (int)cnt[i] : 0;
  Sha256 s;
  sha_init(s);
  for (int k = 0; k < c; ++k) sha_chain_point(s, aff_load(pts + (i * max_pts + k) * 16), enc);
  u256_store(chain + i * 8, sha_final(s));
  sha_init(s);
  for (int k = 0; k < c; ++k) sha_point_compressed(s, aff_load(pts + (i * max_pts + k) * 16));
  u256_store(comp + i * 8, sha_final(s));
}
extern "C" int ecd_sha_points(int n, const uint32_t* pts, int max_pts, const uint32_t* cnt, uint32_t* chain, uint32_t* comp, int chain_point) {
  if (n < 0 || max_pts < 1 || (chain_point != 0 && chain_point != 1)) return (int)hipErrorInvalidValue;
  const Enc enc = ecd_enc(0, chain_point);
  return ecd_run(n, [&](dim3 g) { hipLaunchKernelGGL(k_sha_points, g, dim3(64), 0, 0, n, enc, pts, max_pts, cnt, chain, comp); });
}

// ---- sm:: word helpers (device only) ----------------------------------------------------------------------------------------------------
// Rows in global memory throughout (the helpers take operands there or in per-lane scratch): a [n x na], b [n x nb], r [n x nr],
// flag [n], t1 / t2 [n x nr] scratch of inv2adic.
//   op 0  mul      r[na + nb] = a b                          op 3  sub  r[nr] = a - b, flag = borrow
//   op 1  mullo    r[nr] = low words of a b (na = nb = nr)   op 4  cmp  flag = -1 | 0 | 1
//   op 2  add      r[nr] = a + b, flag = carry               op 5  inv2adic  r[nr] = a^-1 mod 2^(32 nr) (na = nr)
__global__ void __launch_bounds__(64) k_sm(int n, int op, const uint32_t* __restrict__ a, int na, const uint32_t* __restrict__ b, int nb,
                                           uint32_t* __restrict__ r, int nr, uint32_t* __restrict__ flag, uint32_t* __restrict__ t1, uint32_t* __restrict__ t2) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= (size_t)n) return;
  const uint32_t* x = a + i * na;
  const uint32_t* y = b + i * nb;
  uint32_t* o = r + i * nr;
  if (op == 0) sm::mul(o, x, na, y, nb);
  else if (op == 1) sm::mullo(o, x, y, nr);
  else if (op == 2) flag[i] = sm::add(o, nr, x, na, y, nb);
  else if (op == 3) flag[i] = sm::sub(o, nr, x, na, y, nb);
  else if (op == 4) flag[i] = (uint32_t)sm::cmp(x, na, y, nb);
  else sm::inv2adic(o, x, nr, t1 + i * nr, t2 + i * nr);
}
extern "C" int ecd_sm(int op, int n, const uint32_t* a, int na, const uint32_t* b, int nb, uint32_t* r, int nr, uint32_t* flag, uint32_t* t1, uint32_t* t2) {
  bool ok = n >= 0 && op >= 0 && op <= 5 && na >= 1 && nb >= 1 && nr >= 1 && na <= 129 && nb <= 129 && nr <= 258;
  if (op == 0) ok = ok && nr == na + nb;
  if (op == 1 || op == 5) ok = ok && na == nr && nb == nr;
  if (op == 2 || op == 3) ok = ok && nr >= na && nr >= nb;
  if (!ok) return (int)hipErrorInvalidValue;
  return ecd_run(n, [&](dim3 g) { hipLaunchKernelGGL(k_sm, g, dim3(64), 0, 0, n, op, a, na, b, nb, r, nr, flag, t1, t2); });
}
