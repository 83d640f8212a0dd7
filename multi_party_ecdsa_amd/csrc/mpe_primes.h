// Key MATERIAL on the device: batched primality test, the prime search of kzen-paillier, Paillier key pairs and the
// ring-Pedersen parameters (N~, h1, h2) — `Keys::create` of src/protocols/multi_party_ecdsa/gg_2020/party_i.rs:159-177, i.e.
// `Paillier::keypair()` plus `generate_h1_h2_N_tilde()` (:137-156).  Included by mpe_lib.hip after mpe_keygen.h.
//
// The search rule is kzen-paillier's `sample_prime` [RECALLED: kzen-paillier 0.4 `keygen.rs`, un-vendored]:
//   loop { c = BigInt::sample(bits) with bit 0 and bit bits-1 set; if is_prime(c) return c }
// Attempts are FRESH draws (no incremental search), so attempt a of item g is a pure function of (seed, stream, g, a): a 1024-bit
// candidate is exactly 128 keystream bytes, bytes [128 a, 128 a + 128) of the item's stream (mpe_sample.h: ChaCha20, key = seed,
// state[12] = block counter, state[13] = item, state[14..15] = stream id), i.e. blocks 2a and 2a + 1, read as a big-endian integer.
// The result of an item is the candidate of the LOWEST attempt that passes the primality test below with 8 rounds.
// DELIBERATE DIVERGENCE (the same as sampler_max_attempts): the reference loops forever, the device gives up after max_attempts
// candidates (default 16384: the density of primes among odd 1024-bit numbers is ~1/355, so an item gives up with probability
// ~e^-46), writes a zero row, attempt -1, and counts in *fail.
//
// Primality test (mpe_is_probable_prime): trial division by every odd prime below 6370 (the bound of ck_small_factor_kernel) from
// a constant table, then strong-probable-prime (Miller-Rabin) tests to the FIXED bases 2, 3, 5, 7, ... — sound for self-generated
// candidates and fixtures, not for adversarially chosen numbers (composites that pass fixed bases can be constructed).
//
// Pass structure of the search (every loop is bounded by max_attempts; no workgroup waits on another):
//   sieve_kernel      one candidate per lane: 2 ChaCha20 blocks, residues modulo ~400 products (< 2^26) of table primes as
//                     sum_i w_i (2^(32 i) mod M) — 32 multiply-adds with scalar table operands, one multiply-high reduction — and
//                     multiply-high divisibility tests of the residue; survivors (~13 %) are appended to a list (one atomic per wave)
//   mr_kernel round 1 on the survivors (wave-distributed Montgomery engine, Cfg1024: 32 candidates per wave, units from a queue);
//                     who passes (~2 %) is appended to a second list
//   mr_kernel rounds 2..8 on that list; who passes lowers best[item] with atomicMin
//   finalize_kernel   items with a best attempt write their row; the others form the item list of the next pass
// A pass covers attempts [a0, a0 + A) of every unfinished item, A a power of two chosen so that a pass has ~2^20 candidates.
// The SAFE search (`sample_safe_prime`: c and (c - 1) / 2 both prime) is further down, with its joint sieve and its own pass rule.
#pragma once
#include <mutex>
#include "mpe_keygen.h"
#include "mpe_sample.h"

namespace mpe {
namespace pr {

constexpr int SIEVE_BOUND = 6370;                  // trial division by every odd prime below this
constexpr int DEFAULT_MAX_ATTEMPTS = 16384;
constexpr int SEARCH_ROUNDS = 8;
constexpr int PASS_CANDIDATES = 1 << 20;
constexpr int MIN_BLOCK_LOG = 4, MAX_BLOCK_LOG = 10;   // attempts per item and pass: 16 .. 1024

// ---------------------------------------------------------------------------------------------
// the constant table of the sieve (public data; built once per device on the host, never freed)
// ---------------------------------------------------------------------------------------------
struct SieveTab {
  int nprod;                  // products M_j < 2^26 of consecutive table primes
  const uint32_t* M;          // [nprod]
  const uint32_t* inv_lo;     // [nprod]  floor(2^64 / M_j), low and high word
  const uint32_t* inv_hi;     // [nprod]
  const uint32_t* first;      // [nprod + 1]  primes first[j] .. first[j+1]-1 divide M_j
  const uint32_t* pw;         // [nprod][32]  2^(32 i) mod M_j
  const uint32_t* prime;      // [nprimes]
  const uint32_t* pinv;       // [nprimes]  floor(2^32 / p)
};

static int sieve_table(int device, SieveTab* out) {
  static std::once_flag once[64];
  static SieveTab tabs[64];
  static hipError_t err[64];
  if (device < 0 || device >= 64) return MPE_E_ARG;
  std::call_once(once[device], [device]() {
    std::vector<uint32_t> primes;
    for (uint32_t p = 3; p < (uint32_t)SIEVE_BOUND; p += 2) {
      bool is = true;
      for (uint32_t d = 3; d * d <= p; d += 2) if (p % d == 0) { is = false; break; }
      if (is) primes.push_back(p);
    }
    std::vector<uint32_t> M, first;
    uint64_t cur = 1;
    for (size_t k = 0; k < primes.size(); ++k) {
      if (cur == 1) first.push_back((uint32_t)k);
      if (cur * primes[k] >= (1ull << 26)) { M.push_back((uint32_t)cur); cur = 1; first.push_back((uint32_t)k); }
      cur *= primes[k];
    }
    M.push_back((uint32_t)cur);
    first.push_back((uint32_t)primes.size());
    const size_t np = M.size(), nq = primes.size();
    std::vector<uint32_t> blob(np * 3 + (np + 1) + np * 32 + 2 * nq);
    uint32_t* b = blob.data();
    uint32_t *hM = b, *hlo = hM + np, *hhi = hlo + np, *hfirst = hhi + np, *hpw = hfirst + np + 1, *hprime = hpw + np * 32, *hpinv = hprime + nq;
    for (size_t j = 0; j < np; ++j) {
      hM[j] = M[j];
      const uint64_t inv = ~0ull / M[j];                      // = floor(2^64 / M): M is odd and > 1
      hlo[j] = (uint32_t)inv; hhi[j] = (uint32_t)(inv >> 32);
      uint64_t pwr = 1;
      for (int i = 0; i < 32; ++i) { hpw[j * 32 + i] = (uint32_t)pwr; pwr = (pwr << 32) % M[j]; }
    }
    for (size_t j = 0; j <= np; ++j) hfirst[j] = first[j];
    for (size_t k = 0; k < nq; ++k) { hprime[k] = primes[k]; hpinv[k] = (uint32_t)((1ull << 32) / primes[k]); }
    uint32_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, blob.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d, blob.data(), blob.size() * 4, hipMemcpyHostToDevice);
    err[device] = e;
    SieveTab t;
    t.nprod = (int)np;
    t.M = d; t.inv_lo = d + np; t.inv_hi = d + 2 * np; t.first = d + 3 * np; t.pw = t.first + np + 1; t.prime = t.pw + np * 32; t.pinv = t.prime + nq;
    tabs[device] = t;
  });
  if (err[device] != hipSuccess) { mpe_set_error("sieve table", err[device]); return MPE_E_HIP; }
  *out = tabs[device];
  return MPE_OK;
}

// the smallest table prime of products [j0, j1) that divides the odd integer w (32 words), or 0.  JOINT: or that divides (w - 1) / 2,
// which an odd prime l does exactly when w = 1 (mod l) — the same residue serves both numbers.  The product loop is wave-uniform
// (scalar table operands); lanes with on == false only wait.
template <bool JOINT>
__device__ __forceinline__ uint32_t small_factor_range(const uint32_t (&w)[32], bool on, const SieveTab& T, int j0, int j1) {
  uint32_t found = on ? 0u : 1u;
#pragma unroll 1
  for (int j = j0; j < j1; ++j) {
    if (__ballot(found == 0u) == 0ull) break;
    const uint32_t* __restrict__ pw = T.pw + (size_t)j * 32;
    uint64_t acc = 0;                                         // < 32 * 2^32 * 2^26 = 2^63
#pragma unroll
    for (int i = 0; i < 32; ++i) acc += (uint64_t)w[i] * pw[i];
    const uint32_t M = T.M[j];
    const uint64_t inv = ((uint64_t)T.inv_hi[j] << 32) | T.inv_lo[j];
    const uint64_t q = __umul64hi(acc, inv);                  // floor(acc / M) or one less
    uint32_t r = (uint32_t)acc - (uint32_t)q * M;             // acc - q M < 2 M < 2^27
    if (r >= M) r -= M;
    const int k1 = (int)T.first[j + 1];
#pragma unroll 1
    for (int k = (int)T.first[j]; k < k1; ++k) {
      const uint32_t p = T.prime[k];
      const uint32_t t = r - __umulhi(r, T.pinv[k]) * p;      // r mod p, or that + p
      if (found == 0u && (t == 0u || t == p || (JOINT && (t == 1u || t == p + 1u)))) found = p;
    }
  }
  return on ? found : 0u;
}
__device__ __forceinline__ uint32_t small_factor(const uint32_t (&w)[32], bool on, const SieveTab& T) { return small_factor_range<false>(w, on, T, 0, T.nprod); }

// candidate of (item, attempt): words 16 h .. 16 h + 15 of the big-endian reading of blocks 2a, 2a + 1 come from block 2a + 1 - h
__device__ __forceinline__ void candidate_half(const smp::Seed& key, uint32_t item, uint32_t sid_lo, uint32_t sid_hi, uint32_t attempt, int h, uint32_t (&o)[16]) {
  uint32_t ks[16];
  smp::chacha20_block(key, 2u * attempt + (uint32_t)(1 - h), item, sid_lo, sid_hi, ks);
#pragma unroll
  for (int k = 0; k < 16; ++k) o[15 - k] = __builtin_bswap32(ks[k]);
  if (h == 0) o[0] |= 1u;                                     // bit 0
  else o[15] |= 0x80000000u;                                  // bit 1023
}

// position of this lane's entry in a list that every flagged lane of the wave appends to (one atomic per wave); -1 without flag
__device__ __forceinline__ int wave_append(bool flag, int32_t* __restrict__ cnt) {
  const uint64_t m = __ballot(flag);
  if (m == 0ull) return -1;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(cnt, __popcll(m));
  base = __shfl(base, leader);
  return flag ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

// where the candidates of a launch come from: rows of caller values, or the stream of (item, attempt)
struct Source {
  const uint32_t* rows;       // [.][32], or nullptr: candidate id = (u << logA) | j is attempt a0 + j of item items[u]
  smp::Seed key;
  uint32_t sid_lo, sid_hi;
  const int32_t* items;
  int a0, logA;
};

// ---------------------------------------------------------------------------------------------
// sieve of the search: thread c = (u << logA) | j
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) sieve_kernel(int U, Source src, int max_attempts, SieveTab T, int32_t* __restrict__ list, int32_t* __restrict__ cnt) {
  const unsigned c = blockIdx.x * 64u + threadIdx.x;
  const unsigned u = c >> src.logA, j = c & ((1u << src.logA) - 1u);
  const bool on = u < (unsigned)U && src.a0 + (int)j < max_attempts;
  uint32_t w[32];
  {
    const uint32_t item = (uint32_t)src.items[on ? u : 0u], a = (uint32_t)src.a0 + j;
    uint32_t lo[16], hi[16];
    candidate_half(src.key, item, src.sid_lo, src.sid_hi, a, 0, lo);
    candidate_half(src.key, item, src.sid_lo, src.sid_hi, a, 1, hi);
#pragma unroll
    for (int k = 0; k < 16; ++k) { w[k] = lo[k]; w[16 + k] = hi[k]; }
  }
  const uint32_t f = small_factor(w, on, T);
  const int pos = wave_append(on && f == 0u, cnt);
  if (pos >= 0) list[pos] = (int32_t)c;
}

// ---------------------------------------------------------------------------------------------
// joint sieve of the SAFE search, in two launches.  Head: thread c = (u << logA) | j as above; a candidate whose bit 1 is clear is out
// before any product ((c - 1) / 2 would be even), the others meet the first SAFE_HEAD_PRODUCTS products (the primes up to 107) with
// the joint test; ~1.8 % of a pass reach the list.  Tail: the remaining products on that list with every lane of a wave in use —
// the list IS the compaction of live lanes (units of 64 entries from a queue; the candidate is rebuilt from its id: two ChaCha20
// blocks against ~400 products); ~0.5 % of a pass reach the second list.
// ---------------------------------------------------------------------------------------------
constexpr int SAFE_HEAD_PRODUCTS = 6;

__device__ __forceinline__ void candidate_words(const Source& src, unsigned c, uint32_t (&w)[32]) {
  const unsigned u = c >> src.logA, j = c & ((1u << src.logA) - 1u);
  const uint32_t item = (uint32_t)src.items[u], a = (uint32_t)src.a0 + j;
  uint32_t lo[16], hi[16];
  candidate_half(src.key, item, src.sid_lo, src.sid_hi, a, 0, lo);
  candidate_half(src.key, item, src.sid_lo, src.sid_hi, a, 1, hi);
#pragma unroll
  for (int k = 0; k < 16; ++k) { w[k] = lo[k]; w[16 + k] = hi[k]; }
}

__global__ void __launch_bounds__(64) safe_sieve_head_kernel(int U, Source src, int max_attempts, SieveTab T, int32_t* __restrict__ list, int32_t* __restrict__ cnt) {
  const unsigned c = blockIdx.x * 64u + threadIdx.x;
  const unsigned u = c >> src.logA, j = c & ((1u << src.logA) - 1u);
  const bool in = u < (unsigned)U && src.a0 + (int)j < max_attempts;
  uint32_t w[32];
  candidate_words(src, in ? c : 0u, w);
  const bool on = in && (w[0] & 2u) != 0u;
  const int head = T.nprod < SAFE_HEAD_PRODUCTS ? T.nprod : SAFE_HEAD_PRODUCTS;
  const uint32_t f = small_factor_range<true>(w, on, T, 0, head);
  const int pos = wave_append(on && f == 0u, cnt);
  if (pos >= 0) list[pos] = (int32_t)c;
}

__global__ void __launch_bounds__(64) safe_sieve_tail_kernel(const int32_t* __restrict__ count, int cap, const int32_t* __restrict__ list, Source src, SieveTab T,
                                                             int32_t* __restrict__ queue, int32_t* __restrict__ list2, int32_t* __restrict__ cnt2) {
  int total = *count;
  if (total > cap) total = cap;
  const int lane = threadIdx.x & 63;
  const int head = T.nprod < SAFE_HEAD_PRODUCTS ? T.nprod : SAFE_HEAD_PRODUCTS;
#pragma unroll 1
  for (;;) {
    int unit = 0;
    if (lane == 0) unit = atomicAdd(queue, 1);
    unit = __builtin_amdgcn_readfirstlane(unit);
    if ((long long)unit * 64 >= (long long)total) break;
    const int pos = unit * 64 + lane;
    const bool on = pos < total;
    const int32_t id = list[on ? pos : total - 1];
    uint32_t w[32];
    candidate_words(src, (unsigned)id, w);
    const uint32_t f = small_factor_range<true>(w, on, T, head, T.nprod);
    const int p2 = wave_append(on && f == 0u, cnt2);
    if (p2 >= 0 && p2 < cap) list2[p2] = id;
  }
}

// table side of mpe_is_probable_prime: ok[i] = "prime by the table alone"; values the table cannot decide go to the list
__global__ void __launch_bounds__(64) table_kernel(int B, const uint32_t* __restrict__ n, SieveTab T, uint8_t* __restrict__ ok, int32_t* __restrict__ list,
                                                   int32_t* __restrict__ cnt) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const bool in = i < B;
  uint32_t w[32];
  uint32_t hi = 0;
#pragma unroll
  for (int k = 0; k < 32; ++k) { w[k] = in ? n[(size_t)i * 32 + k] : 0u; if (k) hi |= w[k]; }
  const bool small = hi == 0u, odd = (w[0] & 1u) != 0u;
  const bool sieve = in && odd && !(small && w[0] < 2u);
  const uint32_t f = small_factor(w, sieve, T);
  int v = 0;                                                  // 0 composite (or < 2), 1 prime, 2 undecided
  if (in && !odd) v = (small && w[0] == 2u) ? 1 : 0;
  else if (sieve) v = f ? ((small && w[0] == f) ? 1 : 0) : ((small && w[0] < (uint32_t)SIEVE_BOUND * (uint32_t)SIEVE_BOUND) ? 1 : 2);
  if (in) ok[i] = v == 1 ? 1 : 0;
  const int pos = wave_append(v == 2, cnt);
  if (pos >= 0) list[pos] = i;
}

// ---------------------------------------------------------------------------------------------
// Miller-Rabin on the wave-distributed Montgomery engine: one candidate per lane group, units of GROUPS list entries from a queue.
// Per candidate: n's limbs and -n^-1, R mod n by doublings, then per round (base a = the round's prime) ONE pass over the bits
// of n - 1 = 2^s d from the top: square, multiply by a where the bit is set (a is small: the Montgomery residue is scaled limb by
// limb and rippled, no second multiplication), which yields a^d at bit s and its squarings below; where a group stands at or below
// its bit s the residue leaves the Montgomery domain (a multiplication by 1) and is compared with 1 (at bit s only) and n - 1.
// The operation sequence depends on the candidate through the positions of those comparisons (s) and the early exit of a wave whose
// groups are all decided — never on the bits of d: the multiplier of the scaling is selected, not branched on.
// Results: ok[id] (rows), or an append to list2 (round 1 of the search), or atomicMin(best[item slot], attempt in block).
// HALF (the safe search): the number under test is (c - 1) / 2 = c >> 1 of the stream's candidate c, 1023 bits.
// ---------------------------------------------------------------------------------------------
__device__ const uint32_t kBases[16] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53};

template <class C, bool HALF = false>
__global__ void __launch_bounds__(64) mr_kernel(const int32_t* __restrict__ count, int cap, const int32_t* __restrict__ list, Source src, int first_base, int rounds,
                                                int32_t* __restrict__ queue, uint8_t* __restrict__ ok, int32_t* __restrict__ list2, int32_t* __restrict__ cnt2,
                                                int32_t* __restrict__ best) {
  static_assert(C::BITS == 1024 && C::TPI == 2, "one candidate per pair of lanes");
  __shared__ uint32_t lds[C::LDS_WORDS];
  __shared__ uint32_t nws[C::GROUPS][33];
  const Lane ln = make_lane<C>();
  uint32_t* gl = lds + ln.g * C::STRIDE;
  uint32_t* nw = nws[ln.g];
  int total = *count;
  if (total > cap) total = cap;
#pragma unroll 1
  for (;;) {
    int unit = 0;
    if (ln.lane == 0) unit = atomicAdd(queue, 1);
    unit = __builtin_amdgcn_readfirstlane(unit);
    if ((long long)unit * C::GROUPS >= (long long)total) break;
    const int pos = unit * C::GROUPS + ln.g;
    const bool active = pos < total;
    const int id = list[active ? pos : total - 1];
    // ---- the candidate's 32 words -> nw ----
    if (src.rows) {
      for (int q = ln.t; q < 32; q += C::TPI) nw[q] = src.rows[(size_t)id * 32 + q];
    } else {
      const unsigned u = (unsigned)id >> src.logA, j = (unsigned)id & ((1u << src.logA) - 1u);
      uint32_t o[16];
      candidate_half(src.key, (uint32_t)src.items[u], src.sid_lo, src.sid_hi, (uint32_t)src.a0 + j, ln.t, o);
#pragma unroll
      for (int k = 0; k < 16; ++k) nw[16 * ln.t + k] = o[k];
      if (HALF) {                                             // shift right by one across the two lanes' halves
        wave_lds_sync();
        const uint32_t in = ln.t == 0 ? nw[16] : 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = (o[k] >> 1) | ((k < 15 ? o[k + 1] : in) << 31);
        wave_lds_sync();
#pragma unroll
        for (int k = 0; k < 16; ++k) nw[16 * ln.t + k] = o[k];
      }
    }
    wave_lds_sync();
    for (int q = ln.t; q <= (C::W * C::K - 1) / 32 + 1; q += C::TPI) gl[q] = q < 32 ? nw[q] : 0u;
    wave_lds_sync();
    uint32_t n[C::L];
    limbs_from_words<C>(n, gl, ln);
    wave_lds_sync();
    const uint32_t n0 = nw[0];
    uint32_t inv = n0;
#pragma unroll
    for (int i = 0; i < 5; ++i) inv *= 2u - n0 * inv;
    const uint32_t n0inv = (0u - inv) & C::MASK;
    int bl = 1;                                              // bit length of n, and s = the trailing zeros of n - 1 (both lanes read the same words)
    for (int q = 31; q >= 0; --q) { const uint32_t w = nw[q]; if (w) { bl = q * 32 + (32 - __clz(w)); break; } }
    int s = 1;
    for (int q = 0; q < 32; ++q) { const uint32_t w = q ? nw[q] : (nw[0] & ~1u); if (w) { s = q * 32 + __ffs(w) - 1; break; } }
    // ---- one = R mod n: 2^(bl-1) < n doubled up to 2^(W K) ----
    uint32_t one[C::L];
    {
      int64_t x[C::L];
#pragma unroll
      for (int i = 0; i < C::L; ++i) x[i] = (ln.t * C::L + i == (bl - 1) / C::W) ? ((int64_t)1 << ((bl - 1) % C::W)) : 0;
      const int doublings = C::W * C::K - (bl - 1);
      int dmax = doublings;
      for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(dmax, off); dmax = o > dmax ? o : dmax; }
#pragma unroll 1
      for (int d = 0; d < dmax; ++d) {
        const int64_t f = d < doublings ? 2 : 1;
#pragma unroll
        for (int i = 0; i < C::L; ++i) x[i] *= f;
        full_normalize<C>(x, ln);
        const bool ge = cmp_ge<C>(x, n, ln);
#pragma unroll
        for (int i = 0; i < C::L; ++i) x[i] -= ge ? (int64_t)n[i] : 0;
        full_normalize<C>(x, ln);
      }
#pragma unroll
      for (int i = 0; i < C::L; ++i) one[i] = (uint32_t)x[i];
    }
    int top = bl - 1;
    for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(top, off); top = o > top ? o : top; }

    bool alive = active;
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
      if (__ballot(alive) == 0ull) break;
      const uint32_t a = kBases[first_base + r];
      uint32_t x[C::L];
#pragma unroll
      for (int i = 0; i < C::L; ++i) x[i] = one[i];
      bool pass = false, checking = false;
      int i = top;
#pragma unroll 1
      while (i >= 1) {
        if (!checking) {
          put_limbs<C>(gl, x, ln);
        } else {
#pragma unroll
          for (int k = 0; k < C::L; ++k) gl[ln.t * C::L + k] = (ln.t == 0 && k == 0) ? 1u : 0u;
        }
        wave_lds_sync();
        uint32_t y[C::L];
        montmul<C>(y, x, gl, n, n0inv, ln);
        wave_lds_sync();
        if (!checking) {
          // x <- x^2 * (bit i of n - 1 ? a : 1): value < 2 a n <= 106 n, far below R = 2^20 * 2^1024; limbs rippled back below 2^W + 2^7
          const uint32_t mult = ((nw[i >> 5] >> (i & 31)) & 1u) ? a : 1u;
          uint64_t carry = 0;
#pragma unroll
          for (int k = 0; k < C::L; ++k) {
            const uint64_t v = (uint64_t)y[k] * mult + carry;
            x[k] = (uint32_t)v & C::MASK;
            carry = v >> C::W;
          }
          uint32_t cin = pull_prev((uint32_t)carry);
          if (ln.t0) cin = 0;
          x[0] += cin;
          if (__ballot(alive && !pass && i <= s) != 0ull) checking = true;
          else --i;
        } else {
          reduce_once<C>(y, n, ln);                            // x / R mod n, canonical
          bool e1 = true, em = true;
#pragma unroll
          for (int k = 0; k < C::L; ++k) {
            const uint32_t w1 = (ln.t == 0 && k == 0) ? 1u : 0u, wm = n[k] - w1;      // n is odd: n - 1 only changes limb 0
            e1 = e1 && y[k] == w1;
            em = em && y[k] == wm;
          }
          const int sh = ln.g * C::TPI;
          const bool g1 = ((__ballot(e1) >> sh) & 3ull) == 3ull, gm = ((__ballot(em) >> sh) & 3ull) == 3ull;
          if (alive && i <= s && ((i == s && g1) || gm)) pass = true;
          checking = false;
          if (__ballot(alive && !pass) == 0ull) break;
          --i;
        }
      }
      alive = alive && pass;
    }
    if (active && ln.t0) {
      if (ok) ok[id] = alive ? 1 : 0;
      if (alive && list2) { const int p = atomicAdd(cnt2, 1); if (p < cap) list2[p] = id; }
      if (alive && best) atomicMin(best + ((unsigned)id >> src.logA), (int)((unsigned)id & ((1u << src.logA) - 1u)));
    }
    wave_lds_sync();
  }
}

// ---------------------------------------------------------------------------------------------
// bookkeeping of the search
// ---------------------------------------------------------------------------------------------
__global__ void iota_kernel(int n, int32_t* __restrict__ items, int32_t* __restrict__ best) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { items[i] = i; best[i] = 0x7fffffff; }
}
// slot u: its best attempt of this pass, if any, becomes the item's result; otherwise the item goes to the next pass
__global__ void __launch_bounds__(64) finalize_kernel(int U, Source src, int32_t* __restrict__ best, uint32_t* __restrict__ out, int32_t* __restrict__ attempt,
                                                      int32_t* __restrict__ next, int32_t* __restrict__ next_cnt) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  const bool in = u < U;
  const int item = src.items[in ? u : 0];
  const int b = in ? best[u] : 0;
  const bool won = in && b < (1 << src.logA);
  if (in) best[u] = 0x7fffffff;
  if (won) {
    uint32_t lo[16], hi[16];
    candidate_half(src.key, (uint32_t)item, src.sid_lo, src.sid_hi, (uint32_t)(src.a0 + b), 0, lo);
    candidate_half(src.key, (uint32_t)item, src.sid_lo, src.sid_hi, (uint32_t)(src.a0 + b), 1, hi);
    for (int k = 0; k < 16; ++k) { out[(size_t)item * 32 + k] = lo[k]; out[(size_t)item * 32 + 16 + k] = hi[k]; }
    if (attempt) attempt[item] = src.a0 + b;
  }
  const int pos = wave_append(in && !won, next_cnt);
  if (pos >= 0) next[pos] = item;
}
__global__ void giveup_kernel(int U, const int32_t* __restrict__ items, uint32_t* __restrict__ out, int32_t* __restrict__ attempt, int32_t* __restrict__ fail) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int item = items[u];
  for (int k = 0; k < 32; ++k) out[(size_t)item * 32 + k] = 0u;
  if (attempt) attempt[item] = -1;
  if (fail) atomicAdd(fail, 1);
}

static int block_log(int U, int max_log = MAX_BLOCK_LOG, int pass = PASS_CANDIDATES) {
  int want = pass / (U > 0 ? U : 1), lg = MIN_BLOCK_LOG;
  while (lg < max_log && (2 << lg) <= want) ++lg;
  return lg;
}
static long long attempts_in_block(int a0, int logA, int max_attempts) { return max_attempts - a0 < (1 << logA) ? max_attempts - a0 : (1 << logA); }
static size_t pass_candidates(int batch, int pass = PASS_CANDIDATES) {
  const size_t a = (size_t)batch << MIN_BLOCK_LOG;
  return a > (size_t)pass ? a : (size_t)pass;
}

static int mr_grid(const mpe_ctx* ctx, size_t entries) {
  const size_t units = (entries + Cfg1024::GROUPS - 1) / Cfg1024::GROUPS, cap = (size_t)ctx->cus * 8;
  return (int)(units < cap ? (units ? units : 1) : cap);
}

// d_out [batch][32], d_attempt [batch] or nullptr, *d_fail += the items that gave up.  Synchronises `st` once per pass.
static int search_primes(mpe_ctx* ctx, int batch, const smp::Seed& key, uint64_t sid, int max_attempts, uint32_t* d_out, int32_t* d_attempt, int32_t* d_fail,
                         hipStream_t st) {
  if (batch == 0) return MPE_OK;
  SieveTab T;
  MPE_TRY(sieve_table(ctx->device, &T));
  const size_t capC = pass_candidates(batch);
  int32_t* items[2] = {ws_array<int32_t>(ctx, batch), ws_array<int32_t>(ctx, batch)};
  int32_t* best = ws_array<int32_t>(ctx, batch);
  int32_t* list1 = ws_array<int32_t>(ctx, capC);
  int32_t* list2 = ws_array<int32_t>(ctx, capC);
  int32_t* cnt = ws_array<int32_t>(ctx, 8);                   // [0] survivors, [1] round-1 passers, [2] next items, [3], [4] unit queues
  MPE_TRY(ws_ok(ctx));                                       // (the caller began the workspace use, the search only allocates)
  hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(batch, 256)), dim3(256), 0, st, batch, items[0], best);
  int U = batch, a0 = 0, cur = 0;
  while (U > 0 && a0 < max_attempts) {                        // at most max_attempts / 16 passes
    const int logA = block_log(U);
    const size_t C = (size_t)U << logA;                       // <= capC
    Source src{nullptr, key, (uint32_t)sid, (uint32_t)(sid >> 32), items[cur], a0, logA};
    (void)hipMemsetAsync(cnt, 0, 8 * sizeof(int32_t), st);
    hipLaunchKernelGGL(sieve_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, U, src, max_attempts, T, list1, cnt);
    hipLaunchKernelGGL(mr_kernel<Cfg1024>, dim3(mr_grid(ctx, C)), dim3(64), 0, st, (const int32_t*)cnt, (int)C, (const int32_t*)list1, src, 0, 1, cnt + 3,
                       (uint8_t*)nullptr, list2, cnt + 1, (int32_t*)nullptr);
    hipLaunchKernelGGL(mr_kernel<Cfg1024>, dim3(mr_grid(ctx, C / 8)), dim3(64), 0, st, (const int32_t*)(cnt + 1), (int)C, (const int32_t*)list2, src, 1,
                       SEARCH_ROUNDS - 1, cnt + 4, (uint8_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, best);
    hipLaunchKernelGGL(finalize_kernel, dim3(blocks_for(U, 64)), dim3(64), 0, st, U, src, best, d_out, d_attempt, items[cur ^ 1], cnt + 2);
    int32_t h_cnt[3] = {0, 0, 0};
    hipError_t e = hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { mpe_set_error("prime search", e); return MPE_E_HIP; }
    const int h_next = h_cnt[2];
    if (h_next < 0 || h_next > U) { mpe_set_error_msg("prime search: corrupt item count"); return MPE_E_HIP; }
    ctx->search_counts[0] += (long long)U * attempts_in_block(a0, logA, max_attempts);    // mpe_prime_search_counts: attempts, the two list lengths
    ctx->search_counts[1] += h_cnt[0]; ctx->search_counts[2] += h_cnt[1];
    U = h_next; cur ^= 1; a0 += 1 << logA;
  }
  if (U > 0) hipLaunchKernelGGL(giveup_kernel, dim3(blocks_for(U, 256)), dim3(256), 0, st, U, (const int32_t*)items[cur], d_out, d_attempt, d_fail);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mpe_set_error("prime search", e); return MPE_E_HIP; }
  return MPE_OK;
}

// ---------------------------------------------------------------------------------------------
// The SAFE search: kzen-paillier's `sample_safe_prime` [RECALLED: kzen-paillier 0.4 `keygen.rs`, un-vendored]:
//   loop { q = sample_prime(bits); if is_prime((q - 1) / 2) return q }
// Every call of sample_prime goes on with fresh draws, so on the statement above the result of an item is the candidate c of the
// LOWEST attempt a < max_attempts for which c AND (c - 1) / 2 pass the primality test (table primes, 8 rounds) — a pure function of
// (seed, stream, item), whatever the batch, the pass size and the order of the tests.  The density of such attempts is
// 2 C2 / (ln 2^1023 ln 2^1024) ~ 2.6e-6 (C2 ~ 0.66), ~380 000 attempts per result; the default (and largest) cap 2^24 gives up with
// probability ~e^-44.
// A pass: joint sieve (head, tail) -> round 1 on c -> round 1 on (c - 1) / 2 -> rounds 2..8 on c -> rounds 2..8 on (c - 1) / 2 ->
// atomicMin into best; then finalize_kernel / giveup_kernel as above.  A pass fills ~2^safe_pass_log candidates (a context option,
// default 24) WHATEVER the batch, up to 2^20 attempts per item: 1 024 attempts per item and pass would synchronise the host hundreds
// of times for a small batch, and the six Miller-Rabin stages of a pass are a chain of 16 exponentiations one behind the other whose
// lists (0.5 % of the pass and less) must be long enough to fill the device.
// ---------------------------------------------------------------------------------------------
constexpr int SAFE_DEFAULT_MAX_ATTEMPTS = 1 << 24;
constexpr int SAFE_MAX_BLOCK_LOG = 20;

// entries of a survivor list: a pass never holds more than batch << SAFE_MAX_BLOCK_LOG candidates, so a small batch does not pay for the
// whole pass size (batch 1: 2^20 entries, 4 MB a list, instead of 2^24)
static size_t safe_pass_capacity(int batch, int pass) {
  const size_t most = (size_t)batch << SAFE_MAX_BLOCK_LOG;
  return pass_candidates(batch, (int)(most < (size_t)pass ? most : (size_t)pass));
}

static int search_safe_primes(mpe_ctx* ctx, int batch, const smp::Seed& key, uint64_t sid, int max_attempts, uint32_t* d_out, int32_t* d_attempt, int32_t* d_fail,
                              hipStream_t st) {
  if (batch == 0) return MPE_OK;
  SieveTab T;
  MPE_TRY(sieve_table(ctx->device, &T));
  const int pass = 1 << ctx->safe_pass_log;
  const size_t capC = safe_pass_capacity(batch, pass);
  int32_t* items[2] = {ws_array<int32_t>(ctx, batch), ws_array<int32_t>(ctx, batch)};
  int32_t* best = ws_array<int32_t>(ctx, batch);
  int32_t* list[3] = {ws_array<int32_t>(ctx, capC), ws_array<int32_t>(ctx, capC), ws_array<int32_t>(ctx, capC)};
  // [0] head survivors, [1] sieve survivors, [2] round 1 on c, [3] round 1 on the half, [4] rounds 2..8 on c, [5] next items, [8..12] unit queues
  int32_t* cnt = ws_array<int32_t>(ctx, 16);
  MPE_TRY(ws_ok(ctx));
  hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(batch, 256)), dim3(256), 0, st, batch, items[0], best);
  int32_t* const none = nullptr;
  int U = batch, a0 = 0, cur = 0;
  while (U > 0 && a0 < max_attempts) {
    const int logA = block_log(U, SAFE_MAX_BLOCK_LOG, pass);
    const size_t C = (size_t)U << logA;                       // <= capC
    const int cap = (int)C;
    Source src{nullptr, key, (uint32_t)sid, (uint32_t)(sid >> 32), items[cur], a0, logA};
    (void)hipMemsetAsync(cnt, 0, 16 * sizeof(int32_t), st);
    hipLaunchKernelGGL(safe_sieve_head_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, U, src, max_attempts, T, list[0], cnt);
    hipLaunchKernelGGL(safe_sieve_tail_kernel, dim3(mr_grid(ctx, C / 32)), dim3(64), 0, st, (const int32_t*)cnt, cap, (const int32_t*)list[0], src, T, cnt + 8,
                       list[1], cnt + 1);
    hipLaunchKernelGGL((mr_kernel<Cfg1024, false>), dim3(mr_grid(ctx, C / 16)), dim3(64), 0, st, (const int32_t*)(cnt + 1), cap, (const int32_t*)list[1], src, 0, 1,
                       cnt + 9, (uint8_t*)nullptr, list[2], cnt + 2, none);
    hipLaunchKernelGGL((mr_kernel<Cfg1024, true>), dim3(mr_grid(ctx, C / 64)), dim3(64), 0, st, (const int32_t*)(cnt + 2), cap, (const int32_t*)list[2], src, 0, 1,
                       cnt + 10, (uint8_t*)nullptr, list[0], cnt + 3, none);
    hipLaunchKernelGGL((mr_kernel<Cfg1024, false>), dim3(mr_grid(ctx, C / 64)), dim3(64), 0, st, (const int32_t*)(cnt + 3), cap, (const int32_t*)list[0], src, 1,
                       SEARCH_ROUNDS - 1, cnt + 11, (uint8_t*)nullptr, list[1], cnt + 4, none);
    hipLaunchKernelGGL((mr_kernel<Cfg1024, true>), dim3(mr_grid(ctx, C / 64)), dim3(64), 0, st, (const int32_t*)(cnt + 4), cap, (const int32_t*)list[1], src, 1,
                       SEARCH_ROUNDS - 1, cnt + 12, (uint8_t*)nullptr, none, none, best);
    hipLaunchKernelGGL(finalize_kernel, dim3(blocks_for(U, 64)), dim3(64), 0, st, U, src, best, d_out, d_attempt, items[cur ^ 1], cnt + 5);
    int32_t h_cnt[6] = {0, 0, 0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { mpe_set_error("safe prime search", e); return MPE_E_HIP; }
    const int h_next = h_cnt[5];
    if (h_next < 0 || h_next > U) { mpe_set_error_msg("safe prime search: corrupt item count"); return MPE_E_HIP; }
    ctx->search_counts[3] += (long long)U * attempts_in_block(a0, logA, max_attempts);    // mpe_prime_search_counts: attempts, the five list lengths
    for (int i = 0; i < 5; ++i) ctx->search_counts[4 + i] += h_cnt[i];
    U = h_next; cur ^= 1; a0 += 1 << logA;
  }
  if (U > 0) hipLaunchKernelGGL(giveup_kernel, dim3(blocks_for(U, 256)), dim3(256), 0, st, U, (const int32_t*)items[cur], d_out, d_attempt, d_fail);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mpe_set_error("safe prime search", e); return MPE_E_HIP; }
  return MPE_OK;
}

// ---------------------------------------------------------------------------------------------
// key material: one lane per key / statement (glue; the primes above are the cost)
// ---------------------------------------------------------------------------------------------
// N = p q; a key one of whose primes gave up has every row zeroed and counts once in *fail
__global__ void keypair_kernel(int nk, uint32_t* __restrict__ p, uint32_t* __restrict__ q, uint32_t* __restrict__ N, int32_t* __restrict__ fail) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nk) return;
  uint32_t a[32], b[32], r[64];
  sm::copy(a, p + (size_t)k * 32, 32);
  sm::copy(b, q + (size_t)k * 32, 32);
  if (sm::is_zero(a, 32) || sm::is_zero(b, 32)) {
    sm::zero(p + (size_t)k * 32, 32); sm::zero(q + (size_t)k * 32, 32); sm::zero(N + (size_t)k * 64, 64);
    if (fail) atomicAdd(fail, 1);
    return;
  }
  sm::mul(r, a, 32, b, 32);
  sm::copy(N + (size_t)k * 64, r, 64);
}
// N~ = p~ q~, phi = (p~ - 1)(q~ - 1); a failed item gets the harmless odd modulus 3 in nt_ms (the rows the ladders read) and phi = 0
__global__ void nt_setup_kernel(int n, const uint32_t* __restrict__ pt, const uint32_t* __restrict__ qt, uint32_t* __restrict__ nt_ms, uint32_t* __restrict__ phi,
                                int32_t* __restrict__ bad) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint32_t a[32], b[32], r[64], one[1] = {1};
  sm::copy(a, pt + (size_t)k * 32, 32);
  sm::copy(b, qt + (size_t)k * 32, 32);
  const bool isbad = sm::is_zero(a, 32) || sm::is_zero(b, 32);
  bad[k] = isbad ? 1 : 0;
  if (isbad) {
    sm::zero(nt_ms + (size_t)k * 64, 64); nt_ms[(size_t)k * 64] = 3u;
    sm::zero(phi + (size_t)k * 64, 64);
    return;
  }
  sm::mul(r, a, 32, b, 32);
  sm::copy(nt_ms + (size_t)k * 64, r, 64);
  sm::sub(a, 32, a, 32, one, 1);
  sm::sub(b, 32, b, 32, one, 1);
  sm::mul(r, a, 32, b, 32);
  sm::copy(phi + (size_t)k * 64, r, 64);
}
// xi = sample_below(phi) with fresh bytes per attempt until gcd(xi, phi) = 1 (party_i.rs:146-150); phi is even, so xi must be odd and
// the odd-modulus gcd runs with the roles swapped
__global__ void __launch_bounds__(64) xi_kernel(int n, smp::Seed key, uint32_t sid_lo, uint32_t sid_hi, const uint32_t* __restrict__ phi, uint32_t* __restrict__ xi,
                                                int max_attempts, int32_t* __restrict__ bad) {
  __shared__ uint32_t ks[64][17];
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n || bad[k]) return;
  smp::Stream s{&key, (uint32_t)k, sid_lo, sid_hi, ks[threadIdx.x], 0xffffffffu, 0ull};
  const uint32_t* bd = phi + (size_t)k * 64;
  uint32_t* o = xi + (size_t)k * 64;
  bool done = false;
  for (int att = 0; att < max_attempts && !done; ++att) {
    smp::draw_item<0>(s, bd, 64, 0, 0, o, 64, 1, nullptr, nullptr);       // one attempt: zeros when the draw is not below phi
    if (!(o[0] & 1u)) continue;
    uint32_t a[64], m[64];
    sm::copy(a, bd, 64);
    sm::copy(m, o, 64);
    done = smp::coprime_odd(a, m, 64);
  }
  if (!done) { sm::zero(o, 64); bad[k] = 1; }
}
// xi^-1 mod phi = (1 + phi t) / xi with t = (-phi^-1) mod xi: an exact division by the odd xi, done 2-adically like the L function
// (mpe_paillier.h dec_lfunc_kernel); outputs xhi = phi - xi, xhi_inv = phi - xi^-1.  Failed items: every row zero, one count.
__global__ void nt_final_kernel(int n, const uint32_t* __restrict__ nt_ms, const uint32_t* __restrict__ phi, const uint32_t* __restrict__ xi,
                                const uint32_t* __restrict__ phi_inv, const uint8_t* __restrict__ inv_ok, const int32_t* __restrict__ bad, uint32_t* __restrict__ Nt,
                                uint32_t* __restrict__ h1, uint32_t* __restrict__ h2, uint32_t* __restrict__ xhi, uint32_t* __restrict__ xhi_inv, int32_t* __restrict__ fail) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const size_t o = (size_t)k * 64;
  if (bad[k] || !inv_ok[k]) {
    sm::zero(Nt + o, 64); sm::zero(h1 + o, 64); sm::zero(h2 + o, 64); sm::zero(xhi + o, 64); sm::zero(xhi_inv + o, 64);
    if (fail) atomicAdd(fail, 1);
    return;
  }
  uint32_t f[64], x[64], t[64], u[64], iv[64], t1[64], t2[64], one[1] = {1};
  sm::copy(f, phi + o, 64);
  sm::copy(x, xi + o, 64);
  sm::copy(t, phi_inv + o, 64);
  if (!sm::is_zero(t, 64)) sm::sub(t, 64, x, 64, t, 64);      // t = xi - phi^-1 (0 stays 0: xi = 1)
  sm::mullo(u, f, t, 64);
  sm::add(u, 64, u, 64, one, 1);                              // (1 + phi t) mod 2^2048
  sm::inv2adic(iv, x, 64, t1, t2);
  sm::mullo(t, u, iv, 64);                                    // the quotient: it is below phi < 2^2048
  sm::copy(Nt + o, nt_ms + o, 64);
  sm::sub(u, 64, f, 64, x, 64);
  sm::copy(xhi + o, u, 64);
  sm::sub(u, 64, f, 64, t, 64);
  sm::copy(xhi_inv + o, u, 64);
}

}  // namespace pr
}  // namespace mpe

extern "C" {

int mpe_is_probable_prime(mpe_ctx* ctx, int batch, const uint32_t* d_n, int rounds, uint8_t* d_ok, void* stream) {
  if (!ctx || !d_n || !d_ok || batch < 0 || rounds < 1 || rounds > 16) return MPE_E_ARG;
  if (batch == 0) return MPE_OK;
  using namespace mpe;
  hipStream_t st = (hipStream_t)stream;
  pr::SieveTab T;
  MPE_TRY(pr::sieve_table(ctx->device, &T));
  MPE_TRY(ws_begin(ctx, st));
  int32_t* list = ws_array<int32_t>(ctx, batch);
  int32_t* cnt = ws_array<int32_t>(ctx, 8);
  MPE_TRY(ws_ok(ctx));
  (void)hipMemsetAsync(cnt, 0, 8 * sizeof(int32_t), st);
  hipLaunchKernelGGL(pr::table_kernel, dim3(blocks_for(batch, 64)), dim3(64), 0, st, batch, d_n, T, d_ok, list, cnt);
  pr::Source src{d_n, smp::Seed{}, 0u, 0u, nullptr, 0, 0};
  hipLaunchKernelGGL(pr::mr_kernel<Cfg1024>, dim3(pr::mr_grid(ctx, (size_t)batch)), dim3(64), 0, st, (const int32_t*)cnt, batch, (const int32_t*)list, src, 0, rounds,
                     cnt + 3, d_ok, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mpe_set_error("mpe_is_probable_prime", e); return MPE_E_HIP; }
  return MPE_OK;
}

int mpe_sample_prime(mpe_ctx* ctx, int batch, const uint8_t* h_seed32, uint64_t stream_id, int bits, int max_attempts, uint32_t* d_out, int32_t* d_attempt,
                     int32_t* d_fail, void* stream) {
  if (!ctx || !h_seed32 || !d_out || batch < 0 || batch > (1 << 22) || bits != 1024 || max_attempts < 0 || max_attempts > (1 << 24)) return MPE_E_ARG;
  if (batch == 0) return MPE_OK;
  using namespace mpe;
  MPE_TRY(ws_begin(ctx, (hipStream_t)stream));
  return pr::search_primes(ctx, batch, smp::seed_of(h_seed32), stream_id, max_attempts ? max_attempts : pr::DEFAULT_MAX_ATTEMPTS, d_out, d_attempt, d_fail,
                           (hipStream_t)stream);
}

int mpe_sample_safe_prime(mpe_ctx* ctx, int batch, const uint8_t* h_seed32, uint64_t stream_id, int bits, int max_attempts, uint32_t* d_out, int32_t* d_attempt,
                          int32_t* d_fail, void* stream) {
  if (!ctx || !h_seed32 || !d_out || batch < 0 || batch > (1 << 22) || bits != 1024 || max_attempts < 0 || max_attempts > (1 << 24)) return MPE_E_ARG;
  if (batch == 0) return MPE_OK;
  using namespace mpe;
  MPE_TRY(ws_begin(ctx, (hipStream_t)stream));
  return pr::search_safe_primes(ctx, batch, smp::seed_of(h_seed32), stream_id, max_attempts ? max_attempts : pr::SAFE_DEFAULT_MAX_ATTEMPTS, d_out, d_attempt, d_fail,
                                (hipStream_t)stream);
}

int mpe_prime_search_counts(mpe_ctx* ctx, int64_t* h_out9, int reset) {
  if (!ctx || !h_out9) return MPE_E_ARG;
  for (int i = 0; i < 9; ++i) { h_out9[i] = ctx->search_counts[i]; if (reset) ctx->search_counts[i] = 0; }
  return MPE_OK;
}

namespace mpe {
namespace pr {
// one search of the key-material calls: plain (`sample_prime`) or safe (`sample_safe_prime`), the cap's default with it
static int search_any(mpe_ctx* ctx, bool safe, int n, const smp::Seed& key, uint64_t sid, int max_attempts, uint32_t* d_out, hipStream_t st) {
  if (safe) return search_safe_primes(ctx, n, key, sid, max_attempts ? max_attempts : SAFE_DEFAULT_MAX_ATTEMPTS, d_out, nullptr, nullptr, st);
  return search_primes(ctx, n, key, sid, max_attempts ? max_attempts : DEFAULT_MAX_ATTEMPTS, d_out, nullptr, nullptr, st);
}

static int paillier_keygen(mpe_ctx* ctx, bool safe, int nkeys, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_p, uint32_t* d_q, uint32_t* d_N,
                           int32_t* d_fail, hipStream_t st) {
  if (!ctx || !h_seed32 || !d_p || !d_q || !d_N || nkeys < 0 || nkeys > (1 << 22) || (counter >> 56) != 0 || max_attempts < 0 || max_attempts > (1 << 24))
    return MPE_E_ARG;
  if (nkeys == 0) return MPE_OK;
  const smp::Seed key = smp::seed_of(h_seed32);
  uint32_t* prime[2] = {d_p, d_q};
  for (int f = 0; f < 2; ++f) {                                // field f draws stream counter | f << 56 (the convention of mpe_gg20_sample_nonces)
    MPE_TRY(ws_begin(ctx, st));
    MPE_TRY(search_any(ctx, safe, nkeys, key, counter | ((uint64_t)f << 56), max_attempts, prime[f], st));
  }
  MPE_LAUNCH_1D(keypair_kernel, nkeys, st, nkeys, d_p, d_q, d_N, d_fail);
  return MPE_OK;
}
}  // namespace pr
}  // namespace mpe

int mpe_paillier_keygen(mpe_ctx* ctx, int nkeys, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_p, uint32_t* d_q, uint32_t* d_N,
                        int32_t* d_fail, void* stream) {
  return mpe::pr::paillier_keygen(ctx, false, nkeys, h_seed32, counter, max_attempts, d_p, d_q, d_N, d_fail, (hipStream_t)stream);
}
int mpe_paillier_keygen_safe_primes(mpe_ctx* ctx, int nkeys, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_p, uint32_t* d_q, uint32_t* d_N,
                                    int32_t* d_fail, void* stream) {
  return mpe::pr::paillier_keygen(ctx, true, nkeys, h_seed32, counter, max_attempts, d_p, d_q, d_N, d_fail, (hipStream_t)stream);
}

namespace mpe {
namespace pr {
static int ntilde_generate(mpe_ctx* ctx, bool safe, int count, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_Nt, uint32_t* d_h1, uint32_t* d_h2,
                           uint32_t* d_xhi, uint32_t* d_xhi_inv, int32_t* d_fail, hipStream_t st) {
  if (!ctx || !h_seed32 || !d_Nt || !d_h1 || !d_h2 || !d_xhi || !d_xhi_inv || count < 0 || count > (1 << 22) || (counter >> 56) != 0 || max_attempts < 0 ||
      max_attempts > (1 << 24))
    return MPE_E_ARG;
  if (count == 0) return MPE_OK;
  const smp::Seed key = smp::seed_of(h_seed32);
  auto sid = [&](int f) { return counter | ((uint64_t)f << 56); };
  // the secrets of the call (p~, q~, phi, xi, phi^-1 mod xi) live in the context workspace: mpe_ctx_wipe covers them.  The two prime
  // searches allocate behind these arrays, one after the other.
  MPE_TRY(ws_begin(ctx, st));
  uint32_t* pt = ws_array<uint32_t>(ctx, (size_t)count * 32);
  uint32_t* qt = ws_array<uint32_t>(ctx, (size_t)count * 32);
  uint32_t* nt_ms = ws_array<uint32_t>(ctx, (size_t)count * 64);
  uint32_t* phi = ws_array<uint32_t>(ctx, (size_t)count * 64);
  uint32_t* xi = ws_array<uint32_t>(ctx, (size_t)count * 64);
  uint32_t* phi_inv = ws_array<uint32_t>(ctx, (size_t)count * 64);
  int32_t* bad = ws_array<int32_t>(ctx, count);
  uint8_t* inv_ok = ws_array<uint8_t>(ctx, count);
  MPE_TRY(ws_ok(ctx));
  MPE_TRY(search_any(ctx, safe, count, key, sid(2), max_attempts, pt, st));
  MPE_TRY(search_any(ctx, safe, count, key, sid(3), max_attempts, qt, st));
  MPE_LAUNCH_1D(nt_setup_kernel, count, st, count, pt, qt, nt_ms, phi, bad);
  (void)hipMemsetAsync(xi, 0, (size_t)count * 64 * 4, st);
  MPE_TRY(smp::launch_sample(count, h_seed32, sid(4), 0, nt_ms, 64, nullptr, count, 0, 64, d_h1, nullptr, st, nullptr, ctx->sampler_max_attempts, bad));
  hipLaunchKernelGGL(xi_kernel, dim3(blocks_for(count, 64)), dim3(64), 0, st, count, key, (uint32_t)sid(5), (uint32_t)(sid(5) >> 32), (const uint32_t*)phi, xi,
                     ctx->sampler_max_attempts, bad);
  hipLaunchKernelGGL(modinv_lane_kernel<64>, dim3(blocks_for(count, 64)), dim3(64), 0, st, count, (const uint32_t*)xi, Rows{nullptr, nullptr, 1, 0, 0},
                     rows(phi, 64), (const uint8_t*)nullptr, phi_inv, inv_ok);
  mpe_modset* ms = nullptr;
  MPE_TRY(modset_create_dev(ctx, 2048, count, nt_ms, &ms, st));
  int rc = launch_modexp(ctx, ms, count, Rows{nullptr, nullptr, 1, 0, 0}, rows(d_h1, 64), no_rows(), rows(xi, 64), 64, d_h2, st);     // h2 = h1^xi mod N~
  if (rc == MPE_OK) {
    hipLaunchKernelGGL(nt_final_kernel, dim3(blocks_for(count, 64)), dim3(64), 0, st, count, (const uint32_t*)nt_ms, (const uint32_t*)phi, (const uint32_t*)xi,
                       (const uint32_t*)phi_inv, (const uint8_t*)inv_ok, (const int32_t*)bad, d_Nt, d_h1, d_h2, d_xhi, d_xhi_inv, d_fail);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);        // the moduli set is released below
    if (e != hipSuccess) { mpe_set_error("mpe_ntilde_generate", e); rc = MPE_E_HIP; }
  } else {
    (void)hipStreamSynchronize(st);
  }
  mpe_modset_destroy(ms);
  return rc;
}
}  // namespace pr
}  // namespace mpe

int mpe_ntilde_generate(mpe_ctx* ctx, int count, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_Nt, uint32_t* d_h1, uint32_t* d_h2,
                        uint32_t* d_xhi, uint32_t* d_xhi_inv, int32_t* d_fail, void* stream) {
  return mpe::pr::ntilde_generate(ctx, false, count, h_seed32, counter, max_attempts, d_Nt, d_h1, d_h2, d_xhi, d_xhi_inv, d_fail, (hipStream_t)stream);
}
int mpe_ntilde_generate_safe_primes(mpe_ctx* ctx, int count, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_Nt, uint32_t* d_h1,
                                    uint32_t* d_h2, uint32_t* d_xhi, uint32_t* d_xhi_inv, int32_t* d_fail, void* stream) {
  return mpe::pr::ntilde_generate(ctx, true, count, h_seed32, counter, max_attempts, d_Nt, d_h1, d_h2, d_xhi, d_xhi_inv, d_fail, (hipStream_t)stream);
}

}  // extern "C"
