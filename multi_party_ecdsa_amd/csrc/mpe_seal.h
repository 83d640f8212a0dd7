// Sealed records: ChaCha20-Poly1305 (RFC 8439 §2.8) on the device, so that presignature records and key shares leave the device
// encrypted under a wrapping key.  The block function is the sampler's (smp::chacha20_block, mpe_sample.h: state[12] = counter,
// state[13..15] = the 96-bit nonce); this file adds Poly1305 and the AEAD construction:
//   one-time Poly1305 key = the first 32 bytes of block 0;  payload XOR the keystream of blocks 1, 2, ...;
//   tag = Poly1305(pad16(aad) | pad16(ciphertext) | len(aad) as u64 LE | len(ciphertext) as u64 LE).
// THE SEALED ROW (this library's own layout; words are taken as their little-endian byte image throughout): w + 10 words for a
// payload of w words, 1 <= w <= MPE_SEAL_MAX_WORDS:
//   [0] MPE_SEAL_MAGIC | [1] kind | [2] w | [3..5] nonce = (row index within the call, low and high 32 bits of nonce_hi) as
//   state[13..15] | [6 .. 6+w) ciphertext | [6+w .. 10+w) tag;    AAD = words [0..2] as 12 bytes: kind and length are authenticated.
// Poly1305: the 130-bit accumulator in 5 x 26-bit limbs, 5 r precomputed, 64-bit multiply-adds; the limbs are scalar members and
// every limb loop is written out, so the state stays in registers (no per-lane array is indexed at run time).
// Kernels: one row per lane, 64 lanes per workgroup; a lane's keystream block lives in its LDS row, which is zeroed before the kernel ends.
// Opening authenticates first and decrypts second: a row whose header or tag does not match gets an all-zero plaintext row and status
// MPE_SEAL_REFUSED; unauthenticated plaintext is never written to global memory.
// Compiles for the host too (MPE_SEAL_HOST: the includer then supplies smp::Seed and smp::chacha20_block with the device signature)
// so that tests/test_seal_cpu.py drives the Poly1305 core and the row functions the kernels run.
// Included by mpe_lib.hip after mpe_sample.h.
#pragma once
#include <stdint.h>
#include <stddef.h>
#ifdef MPE_SEAL_HOST
#include "../../include/mpecdsa_hip.h"
#define MPE_SL inline
#else
#include "mpe_sample.h"
#define MPE_SL __device__ __forceinline__
#endif

namespace mpe {
namespace seal {

constexpr uint32_t M26 = 0x3ffffffu;
constexpr int HEAD = 6, EXTRA = 10;        // words in front of the ciphertext; sealed words - payload words

struct Poly {
  uint32_t r0, r1, r2, r3, r4;             // r, clamped
  uint32_t s1, s2, s3, s4;                 // 5 r
  uint32_t h0, h1, h2, h3, h4;             // the accumulator
};

// r = the clamped low half of the one-time key (k[0..3] little-endian words), h = 0
MPE_SL void poly_init(Poly& P, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {
  P.r0 = k0 & 0x3ffffffu;
  P.r1 = ((k0 >> 26) | (k1 << 6)) & 0x3ffff03u;
  P.r2 = ((k1 >> 20) | (k2 << 12)) & 0x3ffc0ffu;
  P.r3 = ((k2 >> 14) | (k3 << 18)) & 0x3f03fffu;
  P.r4 = (k3 >> 8) & 0x00fffffu;
  P.s1 = P.r1 * 5u; P.s2 = P.r2 * 5u; P.s3 = P.r3 * 5u; P.s4 = P.r4 * 5u;
  P.h0 = P.h1 = P.h2 = P.h3 = P.h4 = 0u;
}

// h = (h + m + hibit 2^128) r mod 2^130 - 5, partially reduced (limbs <= 26 bits, h1 one more); hibit = 1 for a whole 16-byte block
MPE_SL void poly_block(Poly& P, uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, uint32_t hibit) {
  const uint64_t h0 = P.h0 + (m0 & M26);
  const uint64_t h1 = P.h1 + (((m0 >> 26) | (m1 << 6)) & M26);
  const uint64_t h2 = P.h2 + (((m1 >> 20) | (m2 << 12)) & M26);
  const uint64_t h3 = P.h3 + (((m2 >> 14) | (m3 << 18)) & M26);
  const uint64_t h4 = P.h4 + ((m3 >> 8) | (hibit << 24));
  uint64_t d0 = h0 * P.r0 + h1 * P.s4 + h2 * P.s3 + h3 * P.s2 + h4 * P.s1;
  uint64_t d1 = h0 * P.r1 + h1 * P.r0 + h2 * P.s4 + h3 * P.s3 + h4 * P.s2;
  uint64_t d2 = h0 * P.r2 + h1 * P.r1 + h2 * P.r0 + h3 * P.s4 + h4 * P.s3;
  uint64_t d3 = h0 * P.r3 + h1 * P.r2 + h2 * P.r1 + h3 * P.r0 + h4 * P.s4;
  uint64_t d4 = h0 * P.r4 + h1 * P.r3 + h2 * P.r2 + h3 * P.r1 + h4 * P.r0;
  d1 += d0 >> 26; d2 += d1 >> 26; d3 += d2 >> 26; d4 += d3 >> 26;
  const uint64_t f = (d0 & M26) + (d4 >> 26) * 5u;           // 2^130 = 5
  P.h0 = (uint32_t)(f & M26);
  P.h1 = (uint32_t)((d1 & M26) + (f >> 26));
  P.h2 = (uint32_t)(d2 & M26); P.h3 = (uint32_t)(d3 & M26); P.h4 = (uint32_t)(d4 & M26);
}

// tag = ((h mod 2^130 - 5) + s) mod 2^128: the full carry, then h - (2^130 - 5) selected without a branch when it is not negative
MPE_SL void poly_finish(const Poly& P, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t& t0, uint32_t& t1, uint32_t& t2, uint32_t& t3) {
  uint32_t h0 = P.h0, h1 = P.h1, h2 = P.h2, h3 = P.h3, h4 = P.h4, c;
  c = h1 >> 26; h1 &= M26; h2 += c;
  c = h2 >> 26; h2 &= M26; h3 += c;
  c = h3 >> 26; h3 &= M26; h4 += c;
  c = h4 >> 26; h4 &= M26; h0 += c * 5u;
  c = h0 >> 26; h0 &= M26; h1 += c;                          // once more up the limbs: h0 .. h3 < 2^26 exactly, h4 <= 2^26, h < 2^130 + 2^27
  c = h1 >> 26; h1 &= M26; h2 += c;
  c = h2 >> 26; h2 &= M26; h3 += c;
  c = h3 >> 26; h3 &= M26; h4 += c;
  uint32_t g0 = h0 + 5u;
  c = g0 >> 26; g0 &= M26;
  uint32_t g1 = h1 + c; c = g1 >> 26; g1 &= M26;
  uint32_t g2 = h2 + c; c = g2 >> 26; g2 &= M26;
  uint32_t g3 = h3 + c; c = g3 >> 26; g3 &= M26;
  const uint32_t g4 = h4 + c - (1u << 26);                   // bit 31 set: h + 5 < 2^130, keep h
  const uint32_t keep = 0u - (g4 >> 31), take = ~keep;
  h0 = (h0 & keep) | (g0 & take); h1 = (h1 & keep) | (g1 & take); h2 = (h2 & keep) | (g2 & take);
  h3 = (h3 & keep) | (g3 & take); h4 = (h4 & keep) | (g4 & take);
  const uint32_t w0 = h0 | (h1 << 26), w1 = (h1 >> 6) | (h2 << 20), w2 = (h2 >> 12) | (h3 << 14), w3 = (h3 >> 18) | (h4 << 8);
  uint64_t a = (uint64_t)w0 + s0; t0 = (uint32_t)a;
  a = (uint64_t)w1 + s1 + (a >> 32); t1 = (uint32_t)a;
  a = (uint64_t)w2 + s2 + (a >> 32); t2 = (uint32_t)a;
  a = (uint64_t)w3 + s3 + (a >> 32); t3 = (uint32_t)a;      // the carry out of 128 bits is dropped
}

// the MAC on its own over `bytes` bytes (key: r [4] | s [4] as words): the last, partial block gets the byte 1 behind it and no high bit
MPE_SL void poly1305_bytes(const uint32_t* key, const uint8_t* msg, size_t bytes, uint32_t* tag) {
  Poly P;
  poly_init(P, key[0], key[1], key[2], key[3]);
  for (size_t o = 0; o < bytes; o += 16) {
    const size_t left = bytes - o;
    uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    for (int j = 0; j < 16; ++j) {
      const uint32_t b = (size_t)j < left ? (uint32_t)msg[o + j] : ((size_t)j == left ? 1u : 0u);
      const uint32_t v = b << (8 * (j & 3));
      if (j < 4) m0 |= v; else if (j < 8) m1 |= v; else if (j < 12) m2 |= v; else m3 |= v;
    }
    poly_block(P, m0, m1, m2, m3, left >= 16 ? 1u : 0u);
  }
  poly_finish(P, key[4], key[5], key[6], key[7], tag[0], tag[1], tag[2], tag[3]);
}

// The MAC of a sealed row whose ciphertext word j is ct(j), asked for once per word in ascending order.  Block 0 of the row's keystream
// is taken into blk (16 words owned by the caller: an LDS row on the device); the one-time key is in registers before the first ct(j),
// so ct may use blk for the payload's keystream.
template <class Ct>
MPE_SL void row_tag(const smp::Seed& key, uint32_t n13, uint32_t n14, uint32_t n15, uint32_t kind, uint32_t w, Ct ct, uint32_t* blk,
                    uint32_t& t0, uint32_t& t1, uint32_t& t2, uint32_t& t3) {
  smp::chacha20_block(key, 0u, n13, n14, n15, blk);
  Poly P;
  poly_init(P, blk[0], blk[1], blk[2], blk[3]);
  const uint32_t s0 = blk[4], s1 = blk[5], s2 = blk[6], s3 = blk[7];
  poly_block(P, MPE_SEAL_MAGIC, kind, w, 0u, 1u);            // pad16(aad)
  for (uint32_t j = 0; j < w; j += 4) {                      // pad16(ciphertext)
    const uint32_t c0 = ct(j);
    const uint32_t c1 = j + 1 < w ? ct(j + 1) : 0u;
    const uint32_t c2 = j + 2 < w ? ct(j + 2) : 0u;
    const uint32_t c3 = j + 3 < w ? ct(j + 3) : 0u;
    poly_block(P, c0, c1, c2, c3, 1u);
  }
  poly_block(P, 12u, 0u, 4u * w, 0u, 1u);                    // the two lengths in bytes
  poly_finish(P, s0, s1, s2, s3, t0, t1, t2, t3);
}

// seals one row in one pass: plain word j = src(j); out: the w + 10 words of the sealed row
template <class Src>
MPE_SL void seal_row(const smp::Seed& key, uint32_t n13, uint32_t n14, uint32_t n15, uint32_t kind, uint32_t w, Src src, uint32_t* out, uint32_t* blk) {
  out[0] = MPE_SEAL_MAGIC; out[1] = kind; out[2] = w; out[3] = n13; out[4] = n14; out[5] = n15;
  uint32_t* const ct = out + HEAD;
  uint32_t t0, t1, t2, t3;
  row_tag(key, n13, n14, n15, kind, w, [&](uint32_t j) {
    if ((j & 15u) == 0u) smp::chacha20_block(key, 1u + (j >> 4), n13, n14, n15, blk);
    const uint32_t c = src(j) ^ blk[j & 15u];
    ct[j] = c;
    return c;
  }, blk, t0, t1, t2, t3);
  ct[w] = t0; ct[w + 1] = t1; ct[w + 2] = t2; ct[w + 3] = t3;
  for (int j = 0; j < 16; ++j) blk[j] = 0u;
}

// opens one row of kind `kind` and w payload words: authenticate, then decrypt.  Returns 0, or MPE_SEAL_REFUSED with plain[] all zero.
// The tag is compared without an early exit: the XORs of its four words, ORed (with the header's verdict).
MPE_SL int open_row(const smp::Seed& key, uint32_t kind, uint32_t w, const uint32_t* in, uint32_t* plain, uint32_t* blk) {
  const uint32_t n13 = in[3], n14 = in[4], n15 = in[5];
  const uint32_t* const ct = in + HEAD;
  uint32_t t0, t1, t2, t3;
  row_tag(key, n13, n14, n15, kind, w, [ct](uint32_t j) { return ct[j]; }, blk, t0, t1, t2, t3);
  const uint32_t diff = (in[0] ^ MPE_SEAL_MAGIC) | (in[1] ^ kind) | (in[2] ^ w) | (t0 ^ ct[w]) | (t1 ^ ct[w + 1]) | (t2 ^ ct[w + 2]) | (t3 ^ ct[w + 3]);
  if (diff == 0u) {
    for (uint32_t j = 0; j < w; ++j) {
      if ((j & 15u) == 0u) smp::chacha20_block(key, 1u + (j >> 4), n13, n14, n15, blk);
      plain[j] = ct[j] ^ blk[j & 15u];
    }
  } else {
    for (uint32_t j = 0; j < w; ++j) plain[j] = 0u;
  }
  for (int j = 0; j < 16; ++j) blk[j] = 0u;
  return diff == 0u ? 0 : MPE_SEAL_REFUSED;
}

#ifndef MPE_SEAL_HOST
// a row's plain words gathered from up to three arrays ([count][w[i]] each): one array for caller rows and records, x | p | q for key shares
struct Src3 { const uint32_t* p[3]; uint32_t w[3]; };
struct Gather {
  const uint32_t *a, *b, *c; uint32_t wa, wb;
  __device__ __forceinline__ uint32_t operator()(uint32_t j) const { return j < wa ? a[j] : (j < wa + wb ? b[j - wa] : c[j - wa - wb]); }
};
__device__ __forceinline__ smp::Seed load_key(const uint32_t* d_key) {
  smp::Seed k;
  k.k[0] = d_key[0]; k.k[1] = d_key[1]; k.k[2] = d_key[2]; k.k[3] = d_key[3]; k.k[4] = d_key[4]; k.k[5] = d_key[5]; k.k[6] = d_key[6]; k.k[7] = d_key[7];
  return k;
}

// sealed [count][w + 10].  skip (may be null): a row whose word is non-zero has no record to seal (an export that lost its claim) and
// gets an all-zero sealed row.
__global__ void __launch_bounds__(64) seal_kernel(int count, const uint32_t* __restrict__ d_key, uint32_t kind, uint32_t w, Src3 src, uint32_t n14,
                                                  uint32_t n15, uint32_t* __restrict__ sealed, const int32_t* __restrict__ skip) {
  __shared__ uint32_t ks[64][17];
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= count) return;
  uint32_t* const out = sealed + (size_t)g * (w + EXTRA);
  if (skip && skip[g]) { for (uint32_t j = 0; j < w + EXTRA; ++j) out[j] = 0u; return; }
  const smp::Seed key = load_key(d_key);
  const Gather rd{src.p[0] + (size_t)g * src.w[0], src.p[1] ? src.p[1] + (size_t)g * src.w[1] : nullptr,
                  src.p[2] ? src.p[2] + (size_t)g * src.w[2] : nullptr, src.w[0], src.w[1]};
  seal_row(key, (uint32_t)g, n14, n15, kind, w, rd, out, ks[threadIdx.x]);
}

// plain [count][w], status [count] (0 or MPE_SEAL_REFUSED)
__global__ void __launch_bounds__(64) unseal_kernel(int count, const uint32_t* __restrict__ d_key, uint32_t kind, uint32_t w,
                                                    const uint32_t* __restrict__ sealed, uint32_t* __restrict__ plain, int32_t* __restrict__ status) {
  __shared__ uint32_t ks[64][17];
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= count) return;
  const smp::Seed key = load_key(d_key);
  const int code = open_row(key, kind, w, sealed + (size_t)g * (w + EXTRA), plain + (size_t)g * w, ks[threadIdx.x]);
  if (status) status[g] = code;
}

// tag [count][4] = Poly1305 under key row g ([count][8]: r | s) of message row g ([count][bytes])
__global__ void __launch_bounds__(64) poly1305_kernel(int count, const uint32_t* __restrict__ key, const uint8_t* __restrict__ msg, size_t bytes,
                                                      uint32_t* __restrict__ tag) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= count) return;
  uint32_t t[4];
  poly1305_bytes(key + (size_t)g * 8, msg + (size_t)g * bytes, bytes, t);
  tag[(size_t)g * 4] = t[0]; tag[(size_t)g * 4 + 1] = t[1]; tag[(size_t)g * 4 + 2] = t[2]; tag[(size_t)g * 4 + 3] = t[3];
}
#endif


#ifndef MPE_SEAL_HOST
static int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mpe_set_error(what, e); return MPE_E_HIP; }
  return MPE_OK;
}
static int launch_seal(const uint32_t* d_key, uint32_t kind, int count, int words, Src3 src, uint64_t nonce_hi, uint32_t* d_sealed, const int32_t* d_skip,
                       hipStream_t st) {
  hipLaunchKernelGGL(seal_kernel, dim3(blocks_for(count, 64)), dim3(64), 0, st, count, d_key, kind, (uint32_t)words, src, (uint32_t)nonce_hi,
                     (uint32_t)(nonce_hi >> 32), d_sealed, d_skip);
  return launched("seal_kernel");
}
static int launch_unseal(const uint32_t* d_key, uint32_t kind, int count, int words, const uint32_t* d_sealed, uint32_t* d_plain, int32_t* d_status,
                         hipStream_t st) {
  hipLaunchKernelGGL(unseal_kernel, dim3(blocks_for(count, 64)), dim3(64), 0, st, count, d_key, kind, (uint32_t)words, d_sealed, d_plain, d_status);
  return launched("unseal_kernel");
}
static bool shape_ok(int count, int words) { return count >= 0 && words >= 1 && words <= MPE_SEAL_MAX_WORDS; }
#endif

}  // namespace seal
}  // namespace mpe

#ifndef MPE_SEAL_HOST
// the wrapping key: 32 bytes of device memory owned by the object, zeroed before they are freed
struct mpe_wrap_key {
  mpe_ctx* ctx = nullptr;
  uint32_t* d_key = nullptr;
};

extern "C" {

int mpe_wrap_key_create(mpe_ctx* ctx, const uint8_t* h_key32, mpe_wrap_key** out) {
  if (!ctx || !h_key32 || !out) return MPE_E_ARG;
  mpe_wrap_key* k = new (std::nothrow) mpe_wrap_key();
  if (!k) return MPE_E_NOMEM;
  k->ctx = ctx;
  hipError_t e = hipMalloc((void**)&k->d_key, 32);
  if (e != hipSuccess) { delete k; mpe_set_error("hipMalloc(wrapping key)", e); return MPE_E_NOMEM; }
  e = hipMemcpy(k->d_key, h_key32, 32, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(k->d_key); delete k; mpe_set_error("hipMemcpy(wrapping key)", e); return MPE_E_HIP; }
  *out = k;
  return MPE_OK;
}

int mpe_wrap_key_destroy(mpe_wrap_key* key) {
  if (!key) return MPE_E_ARG;
  (void)hipDeviceSynchronize();                          // calls on any stream may still read the key
  (void)hipMemset(key->d_key, 0, 32);
  (void)hipDeviceSynchronize();
  (void)hipFree(key->d_key);
  delete key;
  return MPE_OK;
}

int mpe_seal(mpe_ctx* ctx, const mpe_wrap_key* key, uint32_t kind, int count, int words, const uint32_t* d_plain, uint64_t nonce_hi, uint32_t* d_sealed,
             void* stream) {
  if (!ctx || !key || kind < MPE_SEAL_KIND_USER || !mpe::seal::shape_ok(count, words) || (count && (!d_plain || !d_sealed))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  return mpe::seal::launch_seal(key->d_key, kind, count, words, mpe::seal::Src3{{d_plain, nullptr, nullptr}, {(uint32_t)words, 0u, 0u}}, nonce_hi, d_sealed,
                                nullptr, (hipStream_t)stream);
}

int mpe_unseal(mpe_ctx* ctx, const mpe_wrap_key* key, uint32_t kind, int count, int words, const uint32_t* d_sealed, uint32_t* d_plain, int32_t* d_status,
               void* stream) {
  if (!ctx || !key || kind < MPE_SEAL_KIND_USER || !mpe::seal::shape_ok(count, words) || (count && (!d_plain || !d_sealed))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  return mpe::seal::launch_unseal(key->d_key, kind, count, words, d_sealed, d_plain, d_status, (hipStream_t)stream);
}

int mpe_poly1305(mpe_ctx* ctx, int count, const uint32_t* d_key, const uint8_t* d_msg, size_t msg_bytes, uint32_t* d_tag, void* stream) {
  if (!ctx || count < 0 || (count && (!d_key || !d_tag || (msg_bytes && !d_msg)))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  hipLaunchKernelGGL(mpe::seal::poly1305_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, (hipStream_t)stream, count, d_key, d_msg, msg_bytes, d_tag);
  return mpe::seal::launched("poly1305_kernel");
}

int mpe_gg20_sealed_presig_words(const mpe_gg20_presig_pool* p) { return p ? mpe_gg20_presig_record_words(p) + mpe::seal::EXTRA : MPE_E_ARG; }

// Sealed export / import stage the clear records in the pool's context's workspace — a region mpe_ctx_scratch_audit counts — between the
// slot kernel and the AEAD kernel, and zero that stage in stream order before they return: afterwards no device buffer outside the pool
// holds a clear record.
int mpe_gg20_sealed_presig_export(mpe_gg20_presig_pool* p, const mpe_wrap_key* key, int count, const int32_t* d_slot, uint64_t nonce_hi,
                                  uint32_t* d_sealed, int32_t* d_status, void* stream) {
  if (!p || !key || count < 0 || (count && (!d_slot || !d_sealed))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  hipStream_t st = (hipStream_t)stream;
  const int W = mpe_gg20_presig_record_words(p);
  const size_t stage_bytes = ((size_t)count * W + (size_t)count) * 4;      // the records, then the row statuses
  MPE_TRY(mpe::ws_begin(p->ctx, st));
  uint32_t* stage = mpe::ws_array<uint32_t>(p->ctx, (size_t)count * W + (size_t)count);
  MPE_TRY(mpe::ws_ok(p->ctx));
  int32_t* code = (int32_t*)(stage + (size_t)count * W);
  hipLaunchKernelGGL(mpe::psg::presig_export_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, st, p->v, count, d_slot, p->K->y, stage, code);
  int rc = mpe::seal::launched("presig_export_kernel");
  if (rc == MPE_OK)
    rc = mpe::seal::launch_seal(key->d_key, MPE_SEAL_KIND_PRESIG, count, W, mpe::seal::Src3{{stage, nullptr, nullptr}, {(uint32_t)W, 0u, 0u}}, nonce_hi,
                                d_sealed, code, st);
  if (rc == MPE_OK && d_status && hipMemcpyAsync(d_status, code, (size_t)count * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = MPE_E_HIP;
  const hipError_t e = hipMemsetAsync(stage, 0, stage_bytes, st);        // whatever happened above
  if (e != hipSuccess && rc == MPE_OK) { mpe_set_error("presig export (stage wipe)", e); rc = MPE_E_HIP; }
  return rc;
}

int mpe_gg20_sealed_presig_import(mpe_gg20_presig_pool* p, const mpe_wrap_key* key, int count, const int32_t* d_slot, const uint32_t* d_sealed,
                                  int32_t* d_status, void* stream) {
  if (!p || !key || count < 0 || (count && (!d_slot || !d_sealed))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  hipStream_t st = (hipStream_t)stream;
  const int W = mpe_gg20_presig_record_words(p);
  const size_t stage_bytes = ((size_t)count * W + (size_t)count) * 4;      // the records, then the AEAD's verdicts
  MPE_TRY(mpe::ws_begin(p->ctx, st));
  uint32_t* stage = mpe::ws_array<uint32_t>(p->ctx, (size_t)count * W + (size_t)count);
  MPE_TRY(mpe::ws_ok(p->ctx));
  int32_t* refused = (int32_t*)(stage + (size_t)count * W);
  // authenticate, then claim: a row the AEAD refuses (its stage row is zero) never reaches the slot's state word
  int rc = mpe::seal::launch_unseal(key->d_key, MPE_SEAL_KIND_PRESIG, count, W, d_sealed, stage, refused, st);
  if (rc == MPE_OK) {
    hipLaunchKernelGGL(mpe::psg::presig_import_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, st, p->v, count, d_slot, p->K->y, stage, d_status,
                       refused);
    rc = mpe::seal::launched("presig_import_kernel");
  }
  const hipError_t e = hipMemsetAsync(stage, 0, stage_bytes, st);
  if (e != hipSuccess && rc == MPE_OK) { mpe_set_error("presig import (stage wipe)", e); rc = MPE_E_HIP; }
  return rc;
}

int mpe_gg20_keyshare_seal(mpe_ctx* ctx, const mpe_wrap_key* key, int count, const uint32_t* d_x, const uint32_t* d_p, const uint32_t* d_q,
                           uint64_t nonce_hi, uint32_t* d_sealed, void* stream) {
  if (!ctx || !key || count < 0 || (count && (!d_x || !d_p || !d_q || !d_sealed))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  return mpe::seal::launch_seal(key->d_key, MPE_SEAL_KIND_KEYSHARE, count, MPE_GG20_KEYSHARE_WORDS, mpe::seal::Src3{{d_x, d_p, d_q}, {8u, 32u, 32u}}, nonce_hi,
                                d_sealed, nullptr, (hipStream_t)stream);
}

int mpe_gg20_keys_create_sealed(mpe_ctx* ctx, int t, int n, int n_signers, int n_sets, const int32_t* h_sets, int nkeysets, int n_own,
                                const int32_t* h_own, const mpe_wrap_key* key, const uint32_t* d_sealed_shares, const uint32_t* d_N,
                                const uint32_t* d_Nt, const uint32_t* d_h1, const uint32_t* d_h2, const uint32_t* d_y, const uint32_t* d_X,
                                mpe_gg20_keys** out, void* stream) {
  if (!ctx || !key || !d_sealed_shares || !out || nkeysets < 1 || n_own < 1 || (long long)nkeysets * n_own > (1ll << 24)) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int rows = nkeysets * n_own, W = MPE_GG20_KEYSHARE_WORDS;
  // clear rows [rows][72], then x [rows][8] | p [rows][32] | q [rows][32] as the existing path takes them, then the row statuses: one
  // allocation of this call, zeroed before it is freed
  const size_t words = (size_t)rows * W * 2, bytes = words * 4 + (size_t)rows * 4;
  uint32_t* clear = nullptr;
  hipError_t e = hipMalloc((void**)&clear, bytes);
  if (e != hipSuccess) { mpe_set_error("hipMalloc(key shares)", e); return MPE_E_NOMEM; }
  uint32_t *x = clear + (size_t)rows * W, *pp = x + (size_t)rows * 8, *qq = pp + (size_t)rows * 32;
  int32_t* d_code = (int32_t*)(clear + words);
  std::vector<int32_t> code((size_t)rows, 0);
  int rc = mpe::seal::launch_unseal(key->d_key, MPE_SEAL_KIND_KEYSHARE, rows, W, d_sealed_shares, clear, d_code, st);
  if (rc == MPE_OK) {
    e = hipMemcpy2DAsync(x, 8 * 4, clear, (size_t)W * 4, 8 * 4, (size_t)rows, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpy2DAsync(pp, 32 * 4, clear + 8, (size_t)W * 4, 32 * 4, (size_t)rows, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpy2DAsync(qq, 32 * 4, clear + 40, (size_t)W * 4, 32 * 4, (size_t)rows, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(code.data(), d_code, (size_t)rows * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { mpe_set_error("mpe_gg20_keys_create_sealed", e); rc = MPE_E_HIP; }
  }
  if (rc == MPE_OK)
    for (int r = 0; r < rows; ++r)
      if (code[(size_t)r] != 0) { mpe_set_error_msg("mpe_gg20_keys_create_sealed: a sealed key share was refused (MPE_SEAL_REFUSED)"); rc = MPE_E_ARG; break; }
  mpe_gg20_keys* made = nullptr;
  if (rc == MPE_OK) rc = mpe_gg20_keys_create_sets(ctx, t, n, n_signers, n_sets, h_sets, nkeysets, n_own, h_own, x, pp, qq, d_N, d_Nt, d_h1, d_h2, d_y, d_X, &made, stream);
  (void)hipStreamSynchronize(st);                        // the key object has taken its copies
  (void)hipMemsetAsync(clear, 0, bytes, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(clear);
  if (rc == MPE_OK) *out = made;
  return rc;
}

}  // extern "C"
#endif
