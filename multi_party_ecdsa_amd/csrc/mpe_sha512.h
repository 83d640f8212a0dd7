// SHA-512 (FIPS 180-4) and HMAC-SHA512 (RFC 2104) on the device: what BIP32 derivation (mpe_bip32.h) hashes with.
// One item per lane, 64 lanes per workgroup.  The compression function is written out: 80 rounds, the eight working variables renamed
// from round to round instead of moved, the message schedule a rolling window of sixteen NAMED 64-bit registers w0 .. w15 (slot t mod 16
// holds W[t]) — no per-lane array is indexed at run time, so nothing goes to scratch.  The 64-bit rotations are two alignbit operations
// on the 32-bit halves; the round constants sit in a __constant__ table and are read with compile-time indices (uniform: they end up
// in scalar registers).
// compress() is inlined; every kernel calls it from ONE site inside its block loop, so each kernel carries one copy.
// Bytes are read one by one (a row of msg_bytes bytes has no alignment to speak of); lengths are per call, so the block loops and the
// choice of what a block holds are uniform over the wave.
// Compiles for the host too (MPE_SHA512_HOST) so that a stand-alone program can drive the same rounds and padding.
// Included by mpe_lib.hip.
#pragma once
#include <stdint.h>
#include <stddef.h>
#ifdef MPE_SHA512_HOST
#define MPE_S5 inline
#define MPE_S5_CONST static const
#else
#define MPE_S5 __device__ __forceinline__
#define MPE_S5_CONST __device__ __constant__ const
#endif

namespace mpe {
namespace s512 {

MPE_S5_CONST uint64_t K512[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
    0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
    0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
    0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
    0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
    0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
    0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

// x rotated right by n bits, 0 < n < 64, n != 32: the halves of the result are two funnel shifts over the halves of x
template <int n>
MPE_S5 uint64_t rotr(uint64_t x) {
  static_assert(n > 0 && n < 64 && n != 32, "rotr");
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  const uint32_t rl = n < 32 ? __builtin_amdgcn_alignbit(hi, lo, n & 31) : __builtin_amdgcn_alignbit(lo, hi, n & 31);
  const uint32_t rh = n < 32 ? __builtin_amdgcn_alignbit(lo, hi, n & 31) : __builtin_amdgcn_alignbit(hi, lo, n & 31);
  return ((uint64_t)rh << 32) | rl;
#else
  return (x >> n) | (x << (64 - n));
#endif
}
MPE_S5 uint64_t big_sigma0(uint64_t x) { return rotr<28>(x) ^ rotr<34>(x) ^ rotr<39>(x); }
MPE_S5 uint64_t big_sigma1(uint64_t x) { return rotr<14>(x) ^ rotr<18>(x) ^ rotr<41>(x); }
MPE_S5 uint64_t small_sigma0(uint64_t x) { return rotr<1>(x) ^ rotr<8>(x) ^ (x >> 7); }
MPE_S5 uint64_t small_sigma1(uint64_t x) { return rotr<19>(x) ^ rotr<61>(x) ^ (x >> 6); }
MPE_S5 uint64_t ch(uint64_t e, uint64_t f, uint64_t g) { return g ^ (e & (f ^ g)); }
MPE_S5 uint64_t maj(uint64_t a, uint64_t b, uint64_t c) { return (a & b) | (c & (a | b)); }

struct State { uint64_t a, b, c, d, e, f, g, h; };
MPE_S5 void init(State& s) {
  s.a = 0x6a09e667f3bcc908ull; s.b = 0xbb67ae8584caa73bull; s.c = 0x3c6ef372fe94f82bull; s.d = 0xa54ff53a5f1d36f1ull;
  s.e = 0x510e527fade682d1ull; s.f = 0x9b05688c2b3e6c1full; s.g = 0x1f83d9abfb41bd6bull; s.h = 0x5be0cd19137e2179ull;
}

#define MPE_S5_RND(a, b, c, d, e, f, g, h, w, i)                            \
  t1 = h + big_sigma1(e) + ch(e, f, g) + K512[i] + w;                        \
  t2 = big_sigma0(a) + maj(a, b, c);                                         \
  d += t1; h = t1 + t2;
#define MPE_S5_RND16(i)                                                                                                  \
  MPE_S5_RND(a, b, c, d, e, f, g, h, w0, i + 0)  MPE_S5_RND(h, a, b, c, d, e, f, g, w1, i + 1)                            \
  MPE_S5_RND(g, h, a, b, c, d, e, f, w2, i + 2)  MPE_S5_RND(f, g, h, a, b, c, d, e, w3, i + 3)                            \
  MPE_S5_RND(e, f, g, h, a, b, c, d, w4, i + 4)  MPE_S5_RND(d, e, f, g, h, a, b, c, w5, i + 5)                            \
  MPE_S5_RND(c, d, e, f, g, h, a, b, w6, i + 6)  MPE_S5_RND(b, c, d, e, f, g, h, a, w7, i + 7)                            \
  MPE_S5_RND(a, b, c, d, e, f, g, h, w8, i + 8)  MPE_S5_RND(h, a, b, c, d, e, f, g, w9, i + 9)                            \
  MPE_S5_RND(g, h, a, b, c, d, e, f, w10, i + 10) MPE_S5_RND(f, g, h, a, b, c, d, e, w11, i + 11)                         \
  MPE_S5_RND(e, f, g, h, a, b, c, d, w12, i + 12) MPE_S5_RND(d, e, f, g, h, a, b, c, w13, i + 13)                         \
  MPE_S5_RND(c, d, e, f, g, h, a, b, w14, i + 14) MPE_S5_RND(b, c, d, e, f, g, h, a, w15, i + 15)
// W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16] into slot t mod 16 (which holds W[t-16]); in order, so that the slots of t-2 and
// t-7 already hold this pass's values where t-2, t-7 fall into it
#define MPE_S5_SCHED(wt, wt1, wt9, wt14) wt += small_sigma1(wt14) + wt9 + small_sigma0(wt1);
#define MPE_S5_SCHED16                                                                                                    \
  MPE_S5_SCHED(w0, w1, w9, w14)   MPE_S5_SCHED(w1, w2, w10, w15)  MPE_S5_SCHED(w2, w3, w11, w0)   MPE_S5_SCHED(w3, w4, w12, w1)   \
  MPE_S5_SCHED(w4, w5, w13, w2)   MPE_S5_SCHED(w5, w6, w14, w3)   MPE_S5_SCHED(w6, w7, w15, w4)   MPE_S5_SCHED(w7, w8, w0, w5)    \
  MPE_S5_SCHED(w8, w9, w1, w6)    MPE_S5_SCHED(w9, w10, w2, w7)   MPE_S5_SCHED(w10, w11, w3, w8)  MPE_S5_SCHED(w11, w12, w4, w9)  \
  MPE_S5_SCHED(w12, w13, w5, w10) MPE_S5_SCHED(w13, w14, w6, w11) MPE_S5_SCHED(w14, w15, w7, w12) MPE_S5_SCHED(w15, w0, w8, w13)

// one 1024-bit block, as sixteen big-endian words
MPE_S5 void compress(State& s, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint64_t w4, uint64_t w5, uint64_t w6, uint64_t w7,
                     uint64_t w8, uint64_t w9, uint64_t w10, uint64_t w11, uint64_t w12, uint64_t w13, uint64_t w14, uint64_t w15) {
  uint64_t a = s.a, b = s.b, c = s.c, d = s.d, e = s.e, f = s.f, g = s.g, h = s.h, t1, t2;
  MPE_S5_RND16(0) MPE_S5_SCHED16 MPE_S5_RND16(16) MPE_S5_SCHED16 MPE_S5_RND16(32) MPE_S5_SCHED16 MPE_S5_RND16(48) MPE_S5_SCHED16 MPE_S5_RND16(64)
  s.a += a; s.b += b; s.c += c; s.d += d; s.e += e; s.f += f; s.g += g; s.h += h;
}
#undef MPE_S5_RND
#undef MPE_S5_RND16
#undef MPE_S5_SCHED
#undef MPE_S5_SCHED16

// The big-endian word at byte `pos` (a multiple of 8) of a byte stream m[0 .. len), then the byte `mark`, then zeros, with `bits` in the
// eight bytes that end at `padded`.  A PADDED message: mark = 0x80, padded = padded_bytes(len), bits = the bit count of everything
// hashed (a prefix block included).  A key block: mark = 0, padded = 0 (no word ends there).
MPE_S5 uint32_t padded_bytes(uint32_t len) { return (len + 17u + 127u) & ~127u; }
MPE_S5 uint64_t stream_word(const uint8_t* m, uint32_t len, uint32_t pos, uint32_t padded, uint64_t bits, uint64_t mark) {
  if (pos + 8u == padded) return bits;
  uint64_t v = 0;
  if (pos + 8u <= len) {
    for (int k = 0; k < 8; ++k) v = (v << 8) | m[pos + k];
    return v;
  }
  if (pos > len) return 0;
  for (uint32_t k = 0; k < 8u; ++k) {
    const uint32_t p = pos + k;
    v = (v << 8) | (p < len ? (uint64_t)m[p] : (p == len ? mark : 0ull));
  }
  return v;
}
MPE_S5 uint64_t padded_word(const uint8_t* m, uint32_t len, uint32_t pos, uint32_t padded, uint64_t bits) {
  return stream_word(m, len, pos, padded, bits, 0x80ull);
}
// the same of a key block: key[0 .. len) and zeros, len <= 128
MPE_S5 uint64_t key_word(const uint8_t* key, uint32_t len, uint32_t pos) { return stream_word(key, len, pos, 0u, 0ull, 0ull); }
MPE_S5 void store_be64(uint8_t* p, uint64_t v) { for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (56 - 8 * k)); }
MPE_S5 void store_digest(uint8_t* out, const State& s) {
  store_be64(out, s.a); store_be64(out + 8, s.b); store_be64(out + 16, s.c); store_be64(out + 24, s.d);
  store_be64(out + 32, s.e); store_be64(out + 40, s.f); store_be64(out + 48, s.g); store_be64(out + 56, s.h);
}

#define MPE_S5_WORDS(F)                                                                                                          \
  w0 = F(0); w1 = F(8); w2 = F(16); w3 = F(24); w4 = F(32); w5 = F(40); w6 = F(48); w7 = F(56);                                   \
  w8 = F(64); w9 = F(72); w10 = F(80); w11 = F(88); w12 = F(96); w13 = F(104); w14 = F(112); w15 = F(120);
#define MPE_S5_COMPRESS(s) compress(s, w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15)

// digest of m[0 .. len)
MPE_S5 void sha512_item(const uint8_t* m, uint32_t len, uint8_t* out) {
  State s;
  init(s);
  const uint32_t padded = padded_bytes(len);
  const uint64_t bits = (uint64_t)len * 8u;
  for (uint32_t base = 0; base < padded; base += 128u) {
    uint64_t w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15;
#define MPE_S5_MSG(o) padded_word(m, len, base + (o), padded, bits)
    MPE_S5_WORDS(MPE_S5_MSG)
    MPE_S5_COMPRESS(s);
  }
  store_digest(out, s);
}

// HMAC(key, m) = H((K ^ opad) | H((K ^ ipad) | m)) with key_len <= 128 (the key is zero-extended to a block, never hashed).  One block
// loop: block 0 the inner key block, blocks 1 .. nb the padded message behind it, then the outer key block and the inner digest's block.
MPE_S5 void hmac_sha512_item(const uint8_t* key, uint32_t key_len, const uint8_t* m, uint32_t len, uint8_t* out) {
  State s;
  init(s);
  const uint32_t padded = padded_bytes(len), nb = padded / 128u;
  const uint64_t bits = (uint64_t)(128u + len) * 8u;
  uint64_t i0 = 0, i1 = 0, i2 = 0, i3 = 0, i4 = 0, i5 = 0, i6 = 0, i7 = 0;      // the inner digest
#pragma unroll 1
  for (uint32_t it = 0; it < nb + 3u; ++it) {
    // what this block reads, as ONE stream: the key (zero-extended, XOR pad), a block of the padded message, or nothing (the digest's block)
    const bool key_block = it == 0 || it == nb + 1u, msg_block = it >= 1u && it <= nb;
    const uint8_t* src = key_block ? key : m;
    const uint32_t slen = key_block ? key_len : (msg_block ? len : 0u), base = msg_block ? (it - 1u) * 128u : 0u, end = msg_block ? padded : 0u;
    const uint64_t mark = msg_block ? 0x80ull : 0ull, pad = !key_block ? 0ull : (it ? 0x5c5c5c5c5c5c5c5cull : 0x3636363636363636ull);
    if (it == nb + 1u) { i0 = s.a; i1 = s.b; i2 = s.c; i3 = s.d; i4 = s.e; i5 = s.f; i6 = s.g; i7 = s.h; init(s); }
    uint64_t w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15;
#define MPE_S5_ANY(o) (stream_word(src, slen, base + (o), end, bits, mark) ^ pad)
    MPE_S5_WORDS(MPE_S5_ANY)
    if (it == nb + 2u) {
      w0 = i0; w1 = i1; w2 = i2; w3 = i3; w4 = i4; w5 = i5; w6 = i6; w7 = i7;
      w8 = 0x8000000000000000ull; w15 = (128u + 64u) * 8u;
    }
    MPE_S5_COMPRESS(s);
  }
  store_digest(out, s);
}
#undef MPE_S5_MSG
#undef MPE_S5_ANY

#ifndef MPE_SHA512_HOST
__global__ void __launch_bounds__(64) sha512_kernel(int batch, const uint8_t* __restrict__ msg, uint32_t msg_bytes, uint8_t* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= batch) return;
  sha512_item(msg + (size_t)g * msg_bytes, msg_bytes, out + (size_t)g * 64);
}
__global__ void __launch_bounds__(64) hmac_sha512_kernel(int batch, const uint8_t* __restrict__ key, uint32_t key_bytes, const uint8_t* __restrict__ msg,
                                                         uint32_t msg_bytes, uint8_t* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= batch) return;
  hmac_sha512_item(key + (size_t)g * key_bytes, key_bytes, msg + (size_t)g * msg_bytes, msg_bytes, out + (size_t)g * 64);
}
#endif

}  // namespace s512
}  // namespace mpe

#ifndef MPE_SHA512_HOST
extern "C" {

int mpe_sha512(mpe_ctx* ctx, int batch, const uint8_t* d_msg, int msg_bytes, uint8_t* d_out, void* stream) {
  if (!ctx || batch < 0 || msg_bytes < 0 || msg_bytes > MPE_SHA512_MAX_MSG_BYTES || (batch && (!d_out || (msg_bytes && !d_msg)))) return MPE_E_ARG;
  if (!batch) return MPE_OK;
  hipLaunchKernelGGL(mpe::s512::sha512_kernel, dim3(mpe::blocks_for(batch, 64)), dim3(64), 0, (hipStream_t)stream, batch, d_msg, (uint32_t)msg_bytes, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mpe_set_error("sha512_kernel", e); return MPE_E_HIP; }
  return MPE_OK;
}

int mpe_hmac_sha512(mpe_ctx* ctx, int batch, const uint8_t* d_key, int key_bytes, const uint8_t* d_msg, int msg_bytes, uint8_t* d_out, void* stream) {
  if (!ctx || batch < 0 || msg_bytes < 0 || msg_bytes > MPE_SHA512_MAX_MSG_BYTES || key_bytes < 0) return MPE_E_ARG;
  if (key_bytes > 128) { mpe_set_error_msg("mpe_hmac_sha512: keys longer than a block (128 bytes) are not supported"); return MPE_E_ARG; }
  if (batch && (!d_out || (msg_bytes && !d_msg) || (key_bytes && !d_key))) return MPE_E_ARG;
  if (!batch) return MPE_OK;
  hipLaunchKernelGGL(mpe::s512::hmac_sha512_kernel, dim3(mpe::blocks_for(batch, 64)), dim3(64), 0, (hipStream_t)stream, batch, d_key, (uint32_t)key_bytes, d_msg,
                     (uint32_t)msg_bytes, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mpe_set_error("hmac_sha512_kernel", e); return MPE_E_HIP; }
  return MPE_OK;
}

}  // extern "C"
#endif
