// BIP32 public derivation (CKDpub) along a path of non-hardened indices, one row per lane:
//   per level   I = HMAC-SHA512(key = chain code, data = serP(K) | ser32(i)),   tweak += I_L (mod q),   K += I_L G,   chain code = I_R
// The tweak is what a GG20 session adds to every key share (mpe_gg20_session_create_tweaks): x' = x + tweak, y' = y + tweak G = K.
// The HMAC of a level is four compressions of mpe_sha512.h (inner key block, the 37-byte message's block, outer key block, the inner
// digest's block), built in registers and run through ONE inlined compress() site; I_L G comes from the comb tables (jac_mul_gen), and
// one field inversion per level brings K back to the affine form serP needs.
// A failed row never reads as "tweak 0" (which would sign for the parent): its tweak is all ones (>= q: a session refuses it with
// MPE_GG20_STATUS_BAD_TWEAK), its child key and chain code are zero.
// Included by mpe_lib.hip after mpe_sha512.h.
#pragma once
#include "mpe_ec.h"
#include "mpe_sha512.h"

namespace mpe {
namespace b32 {

__global__ void __launch_bounds__(64) MPE_EC_OCC bip32_derive_kernel(int batch, int n_parents, const uint32_t* __restrict__ parent_pub,
                          const uint8_t* __restrict__ parent_cc, const int32_t* __restrict__ parent_idx, const uint32_t* __restrict__ path,
                          const int32_t* __restrict__ depth, int max_depth, uint32_t* __restrict__ tweak, uint32_t* __restrict__ child_pub,
                          uint8_t* __restrict__ child_cc, int32_t* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const int pidx = parent_idx ? parent_idx[b] : 0, dep = depth[b];
  int st = 0;
  if ((unsigned)pidx >= (unsigned)n_parents || dep < 0 || dep > max_depth) st = MPE_BIP32_STATUS_DEPTH;
  else
    for (int l = 0; l < dep; ++l) if (path[(size_t)b * max_depth + l] >> 31) st = MPE_BIP32_STATUS_HARDENED;
  ec::Aff K; K.inf = true;
  ec::U256 t = ec::u256_zero();
  uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;             // the chain code, big-endian words
  if (!st) {
    K = ec::aff_load(parent_pub + (size_t)pidx * 16);
    if (!ec::aff_valid(K)) st = MPE_BIP32_STATUS_INVALID;       // not a public key: off the curve, non-canonical, infinity
    const uint8_t* cc = parent_cc + (size_t)pidx * 32;
    c0 = s512::key_word(cc, 32, 0); c1 = s512::key_word(cc, 32, 8); c2 = s512::key_word(cc, 32, 16); c3 = s512::key_word(cc, 32, 24);
  }
  for (int l = 0; l < dep && !st; ++l) {
    const uint32_t idx = path[(size_t)b * max_depth + l];
    // serP(K) | ser32(i) | 0x80: 0x02 + parity, x big-endian (w[7] is the top word), the index — 37 bytes, padded into one block
    const uint64_t m0 = ((uint64_t)(2u + (K.y.w[0] & 1u)) << 56) | ((uint64_t)K.x.w[7] << 24) | (K.x.w[6] >> 8);
    const uint64_t m1 = ((uint64_t)(K.x.w[6] & 0xffu) << 56) | ((uint64_t)K.x.w[5] << 24) | (K.x.w[4] >> 8);
    const uint64_t m2 = ((uint64_t)(K.x.w[4] & 0xffu) << 56) | ((uint64_t)K.x.w[3] << 24) | (K.x.w[2] >> 8);
    const uint64_t m3 = ((uint64_t)(K.x.w[2] & 0xffu) << 56) | ((uint64_t)K.x.w[1] << 24) | (K.x.w[0] >> 8);
    const uint64_t m4 = ((uint64_t)(K.x.w[0] & 0xffu) << 56) | ((uint64_t)idx << 24) | (0x80ull << 16);
    s512::State s;
    s512::init(s);
    uint64_t i0 = 0, i1 = 0, i2 = 0, i3 = 0, i4 = 0, i5 = 0, i6 = 0, i7 = 0;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      uint64_t w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15;
      if (c == 0 || c == 2) {
        const uint64_t pad = c ? 0x5c5c5c5c5c5c5c5cull : 0x3636363636363636ull;
        if (c) { i0 = s.a; i1 = s.b; i2 = s.c; i3 = s.d; i4 = s.e; i5 = s.f; i6 = s.g; i7 = s.h; s512::init(s); }
        w0 = c0 ^ pad; w1 = c1 ^ pad; w2 = c2 ^ pad; w3 = c3 ^ pad;
        w4 = w5 = w6 = w7 = w8 = w9 = w10 = w11 = w12 = w13 = w14 = w15 = pad;
      } else if (c == 1) {
        w0 = m0; w1 = m1; w2 = m2; w3 = m3; w4 = m4;
        w5 = w6 = w7 = w8 = w9 = w10 = w11 = w12 = w13 = w14 = 0; w15 = (128u + 37u) * 8u;
      } else {
        w0 = i0; w1 = i1; w2 = i2; w3 = i3; w4 = i4; w5 = i5; w6 = i6; w7 = i7;
        w8 = 0x8000000000000000ull; w9 = w10 = w11 = w12 = w13 = w14 = 0; w15 = (128u + 64u) * 8u;
      }
      s512::compress(s, w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15);
    }
    ec::U256 il;                                         // I_L as an integer
    il.w[7] = (uint32_t)(s.a >> 32); il.w[6] = (uint32_t)s.a; il.w[5] = (uint32_t)(s.b >> 32); il.w[4] = (uint32_t)s.b;
    il.w[3] = (uint32_t)(s.c >> 32); il.w[2] = (uint32_t)s.c; il.w[1] = (uint32_t)(s.d >> 32); il.w[0] = (uint32_t)s.d;
    if (ec::u256_ge(il, ec::FQ)) { st = MPE_BIP32_STATUS_INVALID; break; }
    const ec::Jac Kn = ec::jac_add(ec::jac_mul_gen(il), ec::jac_from_aff(K));
    if (Kn.inf) { st = MPE_BIP32_STATUS_INVALID; break; }
    K = ec::jac_to_aff(Kn);
    t = ec::sc_add(t, il);
    c0 = s.e; c1 = s.f; c2 = s.g; c3 = s.h;
  }
  if (st) {
    for (int j = 0; j < 8; ++j) tweak[(size_t)b * 8 + j] = 0xFFFFFFFFu;
    for (int j = 0; j < 16; ++j) child_pub[(size_t)b * 16 + j] = 0u;
    c0 = c1 = c2 = c3 = 0;
  } else {
    ec::u256_store(tweak + (size_t)b * 8, t);
    ec::aff_store(child_pub + (size_t)b * 16, K);
  }
  uint8_t* o = child_cc + (size_t)b * 32;
  s512::store_be64(o, c0); s512::store_be64(o + 8, c1); s512::store_be64(o + 16, c2); s512::store_be64(o + 24, c3);
  status[b] = st;
}

}  // namespace b32
}  // namespace mpe

extern "C" {

int mpe_bip32_derive(mpe_ctx* ctx, int batch, int n_parents, const uint32_t* d_parent_pub, const uint8_t* d_parent_cc, const int32_t* d_parent_idx,
                     const uint32_t* d_path, const int32_t* d_depth, int max_depth, uint32_t* d_tweak, uint32_t* d_child_pub, uint8_t* d_child_cc,
                     int32_t* d_status, void* stream) {
  if (!ctx || batch < 0 || n_parents < 1 || max_depth < 1 || max_depth > MPE_BIP32_MAX_DEPTH) return MPE_E_ARG;
  if (!d_parent_pub || !d_parent_cc || !d_path || !d_depth || !d_tweak || !d_child_pub || !d_child_cc || !d_status) return MPE_E_ARG;
  if (!batch) return MPE_OK;
  hipLaunchKernelGGL(mpe::b32::bip32_derive_kernel, dim3(mpe::blocks_for(batch, 64)), dim3(64), 0, (hipStream_t)stream, batch, n_parents, d_parent_pub,
                     d_parent_cc, d_parent_idx, d_path, d_depth, max_depth, d_tweak, d_child_pub, d_child_cc, d_status);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mpe_set_error("bip32_derive_kernel", e); return MPE_E_HIP; }
  return MPE_OK;
}

}  // extern "C"
