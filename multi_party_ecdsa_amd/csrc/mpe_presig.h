// The presignature pool: GG20's offline / online split as a device object.  `CompletedOfflineStage`
// (gg_2020/state_machine/sign/rounds.rs:647-661) is a value in the reference — it leaves `OfflineStage::pick_output` and enters
// `SignManual::new` whenever the message arrives; here one pool SLOT holds that value for the pool's L local parties:
//   per party  k_i [8], sigma_i [8], R [16]          per slot  the key-set index, the signer-set index and one 32-bit STATE word
// in structure-of-arrays form, [capacity][L][w] per field.  After `sign` the slot also keeps m [8] and, per party, r [8] and the own
// s_i [8] for the completion.  The pool's memory is its own allocation, zeroed before it is freed.
//
// States: EMPTY -> READY (deposit, import) -> SIGNED (sign) -> EMPTY (complete); READY -> EMPTY (export); any -> EMPTY (discard);
// BUSY while the one row that owns a transition works on the slot.  Every transition starts with ONE device-scope atomicCAS on the
// state word, taken BEFORE any secret of the slot is read; the row that loses it touches nothing and reports a status.  However calls,
// streams and duplicate indices interleave, at most one partial signature is ever computed from one k_i.  No kernel spins on a state
// word and no workgroup waits for another: the CAS is tried once per row.
// Visibility between kernels that run at the same time on different streams: the winner's agent-scope acquire behind the CAS, an
// agent-scope release in front of the atomic store that ends the transition (the payload pointers are plain, never const __restrict__:
// vector loads behind the acquire).
// Kernels: one row (slot) per lane, 64 lanes per workgroup; the row loops over the L local parties.
// Included by mpe_lib.hip.
#pragma once
#include "mpe_gg20.h"

namespace mpe {
namespace psg {

enum : uint32_t { EMPTY = 0, READY = 1, SIGNED = 2, BUSY = 3 };
constexpr uint32_t REC_VERSION = MPE_GG20_PRESIG_RECORD_VERSION;
constexpr int REC_HEAD = 28;               // version | mask | L | ordinals [8] | key set | y [16]
constexpr int REC_PARTY = 32;              // k_i [8] | sigma_i [8] | R [16]

// what the kernels see of a pool
struct View {
  uint32_t* state;                         // [cap]
  int32_t* keyset;                         // [cap]
  int32_t* sigset;                         // [cap] the signer set (of the key object) the slot's session signed with
  uint32_t *k, *sigma, *R;                 // [cap][L][8], [cap][L][8], [cap][L][16]
  uint32_t *m, *r, *s_own;                 // [cap][8], [cap][L][8], [cap][L][8]: written by sign, read by complete
  int cap, L, S, K;
  int loc[8];                              // local slot -> signer ordinal
  uint32_t loc4;                           // the same, four bits each: a row's loop over the parties reads it without indexing loc[]
  const uint32_t* masks;                   // [nsets] the key object's signer sets as bit masks over party indices (a record's mask word)
  int nsets;
};

// the claim: true for the one row that moves the slot from `from` to BUSY
__device__ __forceinline__ bool claim(uint32_t* word, uint32_t from) {
  const bool won = atomicCAS(word, from, (uint32_t)BUSY) == from;
  if (won) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return won;
}
// ends the transition of the row that holds the claim
__device__ __forceinline__ void settle(uint32_t* word, uint32_t to) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(word, to, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void zero_words(uint32_t* p, int n) { for (int j = 0; j < n; ++j) p[j] = 0u; }
__device__ __forceinline__ void copy_words(uint32_t* dst, const uint32_t* src, int n) { for (int j = 0; j < n; ++j) dst[j] = src[j]; }
// everything a slot holds but its state word
__device__ __forceinline__ void wipe_slot(const View& P, int slot) {
  const size_t pl = (size_t)slot * P.L;
  zero_words(P.k + pl * 8, 8 * P.L); zero_words(P.sigma + pl * 8, 8 * P.L); zero_words(P.R + pl * 16, 16 * P.L);
  zero_words(P.m + (size_t)slot * 8, 8); zero_words(P.r + pl * 8, 8 * P.L); zero_words(P.s_own + pl * 8, 8 * P.L);
  P.keyset[slot] = 0; P.sigset[slot] = 0;
}

// deposit: row b of a session behind round 6 -> slot d_slot[b].  kq, sigma_i, R: the session's [B][L] arrays.
__global__ void __launch_bounds__(64) presig_deposit_kernel(View P, int B, const int32_t* __restrict__ d_slot, const uint32_t* __restrict__ kq,
                                                            const uint32_t* __restrict__ sigma_i, const uint32_t* __restrict__ R,
                                                            const int32_t* __restrict__ sess_status, const int32_t* __restrict__ ks,
                                                            const int32_t* __restrict__ ss, int32_t* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  bool healthy = true;
  for (int li = 0; li < P.L; ++li) healthy = healthy && gg::resolve_status(sess_status, (size_t)B * P.L, b * P.L + li, 6, nullptr, nullptr) == 0;
  const int slot = d_slot[b];
  int code = 0;
  if (!healthy) code = MPE_GG20_PRESIG_SESSION_FAILED;
  else if (slot < 0 || slot >= P.cap) code = MPE_GG20_PRESIG_DEPOSIT_RANGE;
  else if (!claim(P.state + slot, EMPTY)) code = MPE_GG20_PRESIG_DEPOSIT_NOT_EMPTY;
  if (code == 0) {
    const size_t pl = (size_t)slot * P.L, pi = (size_t)b * P.L;
    copy_words(P.k + pl * 8, kq + pi * 8, 8 * P.L);
    copy_words(P.sigma + pl * 8, sigma_i + pi * 8, 8 * P.L);
    copy_words(P.R + pl * 16, R + pi * 16, 16 * P.L);
    P.keyset[slot] = ks ? ks[b] : 0;
    P.sigset[slot] = ss ? ss[b] : 0;         // (a healthy session's index is one of the key object's: r0_kernel)
    settle(P.state + slot, READY);
  }
  if (status) status[b] = code;
}

// sign: Round7::new / phase7_local_sig (party_i.rs:850-871) for READY slots: s_i = m k_i + r sigma_i, m and r reduced as r7_kernel
// reduces them; m, r, s_i stay in the slot for the completion, k_i and sigma_i are zeroed here.  s_out [L][count][8].
__global__ void __launch_bounds__(64) presig_sign_kernel(View P, int count, const int32_t* __restrict__ d_slot, const uint32_t* __restrict__ msg,
                                                         uint32_t* __restrict__ s_out, int32_t* __restrict__ status) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const int slot = d_slot[g];
  int code = 0;
  if (slot < 0 || slot >= P.cap) code = MPE_GG20_PRESIG_SIGN_RANGE;
  else if (!claim(P.state + slot, READY)) code = MPE_GG20_PRESIG_SIGN_NOT_READY;
  if (code == 0) {
    const ec::U256 m = ec::sc_reduce(msg + (size_t)g * 8, 8);
    ec::u256_store(P.m + (size_t)slot * 8, m);
#pragma unroll 1
    for (int li = 0; li < P.L; ++li) {
      const size_t pl = (size_t)slot * P.L + li;
      const ec::U256 r = ec::sc_reduce(P.R + pl * 16, 8);
      const ec::U256 si = ec::sc_add(ec::sc_mul(m, ec::u256_load(P.k + pl * 8)), ec::sc_mul(r, ec::u256_load(P.sigma + pl * 8)));
      zero_words(P.k + pl * 8, 8); zero_words(P.sigma + pl * 8, 8);
      ec::u256_store(P.r + pl * 8, r);
      ec::u256_store(P.s_own + pl * 8, si);
      ec::u256_store(s_out + ((size_t)li * count + g) * 8, si);
    }
    settle(P.state + slot, SIGNED);
  } else {
    for (int li = 0; li < P.L; ++li) zero_words(s_out + ((size_t)li * count + g) * 8, 8);
  }
  if (status) status[g] = code;
}

// complete: SignManual::complete -> output_signature + verify (party_i.rs:873-936) for SIGNED slots, the body of complete_kernel fed
// through the slot gather.  in: the partial signatures of all S senders, row g of sender j at record in.off[j] + g.
// r_out, s_out [L][count][8], recid_out, status [L][count]; the slot is EMPTY afterwards whatever the verdict.
__global__ void __launch_bounds__(64) MPE_EC_OCC presig_complete_kernel(View P, int count, const int32_t* __restrict__ d_slot, gg::Slab in,
                                                                        const uint32_t* __restrict__ y, uint32_t* __restrict__ r_out,
                                                                        uint32_t* __restrict__ s_out, int32_t* __restrict__ recid_out,
                                                                        int32_t* __restrict__ status) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const int slot = d_slot[g];
  int code = 0;
  if (slot < 0 || slot >= P.cap) code = MPE_GG20_PRESIG_COMPLETE_RANGE;
  else if (!claim(P.state + slot, SIGNED)) code = MPE_GG20_PRESIG_COMPLETE_NOT_SIGNED;
#pragma unroll 1
  for (int li = 0; li < P.L; ++li) {
    const size_t o = (size_t)li * count + g;
    ec::U256 r = ec::u256_zero(), s = ec::u256_zero();
    int recid = 0, st = code;
    if (code == 0) {
      const size_t pl = (size_t)slot * P.L + li;
      const int i = (int)((P.loc4 >> (4 * li)) & 15u);
      s = ec::u256_load(P.s_own + pl * 8);
      for (int j = 0; j < P.S; ++j) if (j != i) s = ec::sc_add(s, ec::sc_reduce(gg::rec_of(in, j, g) + gg::M7.s_i.off, 8));
      const ec::U256 m = ec::u256_load(P.m + (size_t)slot * 8);
      r = ec::u256_load(P.r + pl * 8);
      const ec::U256 ry = ec::sc_reduce(P.R + pl * 16 + 8, 8);
      if (!gg::output_signature_check(s, recid, m, r, ry, y + (size_t)P.keyset[slot] * 16)) {
        st = MPE_GG20_PRESIG_VERIFY_FAILED; r = ec::u256_zero(); s = ec::u256_zero(); recid = 0;
      }
    }
    if (r_out) ec::u256_store(r_out + o * 8, r);
    if (s_out) ec::u256_store(s_out + o * 8, s);
    if (recid_out) recid_out[o] = recid;
    if (status) status[o] = st;
  }
  if (code == 0) {         // what a SIGNED slot still holds (sign zeroed k_i and sigma_i)
    const size_t pl = (size_t)slot * P.L;
    zero_words(P.R + pl * 16, 16 * P.L); zero_words(P.m + (size_t)slot * 8, 8); zero_words(P.r + pl * 8, 8 * P.L); zero_words(P.s_own + pl * 8, 8 * P.L);
    P.keyset[slot] = 0; P.sigset[slot] = 0;
    settle(P.state + slot, EMPTY);
  }
}

// the offline stage as one call (mpe_gg20_presign_sets): the sibling of sign_finish_kernel.  A row's status = its session's smallest
// non-zero party status behind round 6 — what mpe_gg20_sign would report, 92 for a bad set index included, not the deposit's blanket
// 803 — otherwise the deposit's 801 / 802, otherwise 0.  sess_status: the session's per-round words, which the deposit's wipe leaves.
__global__ void presign_finish_kernel(int B, int L, int b0, const int32_t* __restrict__ sess_status, const int32_t* __restrict__ dep,
                                      int32_t* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int st = 0;
  for (int li = 0; li < L; ++li) {
    const int s = gg::resolve_status(sess_status, (size_t)B * L, b * L + li, 6, nullptr, nullptr);
    if (s && (!st || s < st)) st = s;
  }
  status[(size_t)b0 + b] = st ? st : dep[b];
}

// the online step in one launch, for a pool that holds all S signers (L == S): the claim of presig_sign_kernel, every party's
// s_i = m k_i + r sigma_i with k_i and sigma_i zeroed at once, the sum, then output_signature's low-s rule and verify ONCE, and the
// slot back to EMPTY with the wipe.  One verify is exact: the S parties of the composed path (sign + complete) verify the same sum s
// under the same y, and the same (m, r, R.y) when the slot's parties hold one R — the argument of dedup_verify.  A healthy offline
// stage leaves one R; a slot whose parties hold different ones (only an import can make it) is 701 here without a verify, as at least one
// party's verify of the composed path fails on it but for a negligible chance.  r_out, s_out [count][8], zero unless status is 0.
__global__ void __launch_bounds__(64) MPE_EC_OCC presig_sign_online_kernel(View P, int count, const int32_t* __restrict__ d_slot,
                                                                           const uint32_t* __restrict__ msg, const uint32_t* __restrict__ y,
                                                                           uint32_t* __restrict__ r_out, uint32_t* __restrict__ s_out,
                                                                           int32_t* __restrict__ recid_out, int32_t* __restrict__ status) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const int slot = d_slot[g];
  int code = 0, recid = 0;
  if (slot < 0 || slot >= P.cap) code = MPE_GG20_PRESIG_SIGN_RANGE;
  else if (!claim(P.state + slot, READY)) code = MPE_GG20_PRESIG_SIGN_NOT_READY;
  ec::U256 r = ec::u256_zero(), s = ec::u256_zero();
  if (code == 0) {
    const size_t p0 = (size_t)slot * P.L;
    const ec::U256 m = ec::sc_reduce(msg + (size_t)g * 8, 8);
    r = ec::sc_reduce(P.R + p0 * 16, 8);
    const ec::U256 ry = ec::sc_reduce(P.R + p0 * 16 + 8, 8);
    bool one_R = true;
#pragma unroll 1
    for (int li = 0; li < P.L; ++li) {
      const size_t pl = p0 + li;
      one_R = one_R && gg::words_eq(P.R + pl * 16, P.R + p0 * 16, 16);
      s = ec::sc_add(s, ec::sc_add(ec::sc_mul(m, ec::u256_load(P.k + pl * 8)), ec::sc_mul(r, ec::u256_load(P.sigma + pl * 8))));
      zero_words(P.k + pl * 8, 8); zero_words(P.sigma + pl * 8, 8);
    }
    if (!one_R || !gg::output_signature_check(s, recid, m, r, ry, y + (size_t)P.keyset[slot] * 16)) {
      code = MPE_GG20_PRESIG_VERIFY_FAILED; r = ec::u256_zero(); s = ec::u256_zero(); recid = 0;
    }
    wipe_slot(P, slot);
    settle(P.state + slot, EMPTY);
  }
  ec::u256_store(r_out + (size_t)g * 8, r);
  ec::u256_store(s_out + (size_t)g * 8, s);
  recid_out[g] = recid;
  if (status) status[g] = code;
}

// export: READY -> EMPTY, the record is then the only copy.  rec [count][REC_HEAD + REC_PARTY L]; a losing row's record is zero.
__global__ void __launch_bounds__(64) presig_export_kernel(View P, int count, const int32_t* __restrict__ d_slot, const uint32_t* __restrict__ y,
                                                           uint32_t* __restrict__ rec, int32_t* __restrict__ status) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const int slot = d_slot[g], W = REC_HEAD + REC_PARTY * P.L;
  uint32_t* o = rec + (size_t)g * W;
  int code = 0;
  if (slot < 0 || slot >= P.cap) code = MPE_GG20_PRESIG_RECORD_RANGE;
  else if (!claim(P.state + slot, READY)) code = MPE_GG20_PRESIG_EXPORT_NOT_READY;
  if (code == 0) {
    const int kk = P.keyset[slot];
    o[0] = REC_VERSION; o[1] = P.masks[P.sigset[slot]]; o[2] = (uint32_t)P.L;
    for (int j = 0; j < 8; ++j) o[3 + j] = j < P.L ? (uint32_t)P.loc[j] : 0u;
    o[11] = (uint32_t)kk;
    copy_words(o + 12, y + (size_t)kk * 16, 16);
    for (int li = 0; li < P.L; ++li) {
      const size_t pl = (size_t)slot * P.L + li;
      uint32_t* p = o + REC_HEAD + REC_PARTY * li;
      copy_words(p, P.k + pl * 8, 8); copy_words(p + 8, P.sigma + pl * 8, 8); copy_words(p + 16, P.R + pl * 16, 16);
    }
    wipe_slot(P, slot);
    settle(P.state + slot, EMPTY);
  } else {
    zero_words(o, W);
  }
  if (status) status[g] = code;
}

// import: EMPTY -> READY for a record that is this pool's (version, one of the key object's signer sets, local parties), names one of its key sets with that key
// set's y, and holds values a healthy offline stage leaves: every R on the curve, 0 < k_i < q, sigma_i < q.  The record is judged before
// the slot is claimed: a refused record leaves the slot as it was.  refused (null for clear records): the sealed import's verdict on the
// row's authentication (mpe_seal.h) — a non-zero word is the row's status, and the row goes no further.
__global__ void __launch_bounds__(64) presig_import_kernel(View P, int count, const int32_t* __restrict__ d_slot, const uint32_t* __restrict__ y,
                                                           const uint32_t* __restrict__ rec, int32_t* __restrict__ status,
                                                           const int32_t* __restrict__ refused) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const int slot = d_slot[g], W = REC_HEAD + REC_PARTY * P.L;
  const uint32_t* o = rec + (size_t)g * W;
  int code = 0, sigset = 0;
  if (slot < 0 || slot >= P.cap) code = MPE_GG20_PRESIG_RECORD_RANGE;
  else if (refused && refused[g]) code = refused[g];
  else {
    int set = -1;
    for (int k = 0; k < P.nsets; ++k) if (P.masks[k] == o[1]) set = k;
    bool ok = o[0] == REC_VERSION && set >= 0 && o[2] == (uint32_t)P.L && o[11] < (uint32_t)P.K;
    sigset = set < 0 ? 0 : set;
    for (int j = 0; j < 8; ++j) ok = ok && o[3 + j] == (j < P.L ? (uint32_t)P.loc[j] : 0u);
    if (ok) ok = gg::words_eq(o + 12, y + (size_t)o[11] * 16, 16);
#pragma unroll 1
    for (int li = 0; ok && li < P.L; ++li) {
      const uint32_t* p = o + REC_HEAD + REC_PARTY * li;
      ok = ec::sc_is_canonical_nonzero(p) && !ec::u256_ge(ec::u256_load(p + 8), ec::FQ) && ec::aff_valid(ec::aff_load(p + 16));
    }
    if (!ok) code = MPE_GG20_PRESIG_IMPORT_REFUSED;
    else if (!claim(P.state + slot, EMPTY)) code = MPE_GG20_PRESIG_IMPORT_NOT_EMPTY;
  }
  if (code == 0) {
    for (int li = 0; li < P.L; ++li) {
      const size_t pl = (size_t)slot * P.L + li;
      const uint32_t* p = o + REC_HEAD + REC_PARTY * li;
      copy_words(P.k + pl * 8, p, 8); copy_words(P.sigma + pl * 8, p + 8, 8); copy_words(P.R + pl * 16, p + 16, 16);
    }
    P.keyset[slot] = (int32_t)o[11]; P.sigset[slot] = sigset;
    settle(P.state + slot, READY);
  }
  if (status) status[g] = code;
}

// discard: READY, SIGNED or EMPTY -> EMPTY with the wipe.  One attempt per state, no loop: a slot that is BUSY belongs to a row of a call
// that is running right now on another stream, and that row settles it.
__global__ void __launch_bounds__(64) presig_discard_kernel(View P, int count, const int32_t* __restrict__ d_slot) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const int slot = d_slot[g];
  if (slot < 0 || slot >= P.cap) return;
  if (claim(P.state + slot, READY) || claim(P.state + slot, SIGNED) || claim(P.state + slot, EMPTY)) {
    wipe_slot(P, slot);
    settle(P.state + slot, EMPTY);
  }
}

// audit: out[0..3] = slots per state, out[4] = non-zero words of k_i, sigma_i in slots that are not READY
__global__ void __launch_bounds__(64) presig_audit_kernel(View P, unsigned long long* __restrict__ out) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= P.cap) return;
  const uint32_t st = __hip_atomic_load(P.state + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(out + (st < 4u ? st : (uint32_t)BUSY), 1ull);
  if (st == READY) return;
  unsigned long long stray = 0;
  const size_t pl = (size_t)slot * P.L;
  for (int j = 0; j < 8 * P.L; ++j) stray += (P.k[pl * 8 + j] != 0u) + (P.sigma[pl * 8 + j] != 0u);
  if (stray) atomicAdd(out + 4, stray);
}

}  // namespace psg
}  // namespace mpe

struct mpe_gg20_presig_pool {
  mpe_ctx* ctx = nullptr;
  const mpe_gg20_keys* K = nullptr;
  void* mem = nullptr;
  size_t mem_bytes = 0;
  mpe::psg::View v{};
};

namespace mpe {
namespace psg {

static size_t layout(View& v, char* base) {
  gg::Bump m(base);
  const size_t cap = (size_t)v.cap, pl = cap * v.L;
  v.state = m.w(cap); v.keyset = m.i(cap); v.sigset = m.i(cap);
  v.k = m.w(pl * 8); v.sigma = m.w(pl * 8); v.R = m.w(pl * 16);
  v.m = m.w(cap * 8); v.r = m.w(pl * 8); v.s_own = m.w(pl * 8);
  return m.off;
}
// the session's nonce-derived state as mpe_gg20_session_abort wipes it, with the status and bad_actors words left readable
static hipError_t wipe_session_after_deposit(mpe_gg20_session* s, hipStream_t st) {
  gg::ahead_drain(s, st);
  char* const end = (char*)s->mem + s->mem_bytes;
  hipError_t e = hipMemsetAsync(s->kq, 0, (size_t)((char*)s->bad - (char*)s->kq), st);
  if (e == hipSuccess) e = hipMemsetAsync(s->sig_r, 0, (size_t)((char*)s->status - (char*)s->sig_r), st);
  if (e == hipSuccess) e = hipMemsetAsync(s->sig_recid, 0, (size_t)(end - (char*)s->sig_recid), st);
  return e;
}
static int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mpe_set_error(what, e); return MPE_E_HIP; }
  return MPE_OK;
}
// The deposit for callers inside the library: the session's context may be another one ON THE SAME DEVICE (the pipelined engine's lanes
// run on contexts of their own; the pool reads nothing from its context).  mpe_gg20_presig_deposit asks for the pool's context first.
static int deposit_into(mpe_gg20_presig_pool* p, mpe_gg20_session* s, const int32_t* d_slot, int32_t* d_status, hipStream_t st) {
  if (!p || !s || !d_slot) return MPE_E_ARG;
  if (s->failed || s->next_round != 7) { mpe_set_error_msg("presig deposit: the session is not behind round 6"); return MPE_E_ARG; }
  // a record has no field for a tweak (MPE_GG20_PRESIG_RECORD_VERSION stays 1) and the pool signs and checks under the key object's y
  if (s->d.tw) { mpe_set_error_msg("presig deposit: a session with tweaks (mpe_gg20_session_create_tweaks) cannot be deposited"); return MPE_E_ARG; }
  bool same = s->K == p->K && s->ctx->device == p->ctx->device && s->L == p->v.L && s->d.lparty < 0;      // (the pool's local parties are ordinals)
  for (int i = 0; same && i < s->L; ++i) same = s->d.loc[i] == p->v.loc[i];
  if (!same) { mpe_set_error_msg("presig deposit: the session's keys or local parties are not the pool's"); return MPE_E_ARG; }
  hipLaunchKernelGGL(presig_deposit_kernel, dim3(blocks_for(s->B, 64)), dim3(64), 0, st, p->v, s->B, d_slot, s->kq, s->sigma_i,
                     s->R, s->status, s->d.ks, s->d.ss, d_status);
  int rc = launched("presig_deposit_kernel");
  // deposited or not, the session's copy goes, as mpe_gg20_session_abort wipes it: the only live k_i is the pool's
  const hipError_t em = wipe_session_after_deposit(s, st);
  if (em != hipSuccess && rc == MPE_OK) { mpe_set_error("presig deposit (wipe)", em); rc = MPE_E_HIP; }
  s->failed = true;
  s->next_round = 9;
  return rc;
}
// a pool over `keys` on `ctx`'s device that holds all S signers (its ordinals are then 0 .. S-1)
static bool holds_every_signer(const mpe_gg20_presig_pool* p, const mpe_gg20_keys* keys, const mpe_ctx* ctx) {
  return p && p->K == keys && p->v.L == keys->S && (!ctx || p->ctx->device == ctx->device);
}

}  // namespace psg
}  // namespace mpe

extern "C" {

int mpe_gg20_presig_pool_create(mpe_ctx* ctx, const mpe_gg20_keys* keys, int n_local, const int32_t* h_local, int capacity,
                                mpe_gg20_presig_pool** out) {
  if (!ctx || !keys || !out || !h_local || n_local < 1 || n_local > keys->S || capacity < 1 || (long long)capacity * n_local > (1ll << 28)) return MPE_E_ARG;
  for (int i = 0; i < n_local; ++i)
    if (h_local[i] < 0 || h_local[i] >= keys->S || (i && h_local[i] <= h_local[i - 1])) return MPE_E_ARG;
  mpe_gg20_presig_pool* p = new (std::nothrow) mpe_gg20_presig_pool();
  if (!p) return MPE_E_NOMEM;
  p->ctx = ctx; p->K = keys;
  mpe::psg::View& v = p->v;
  v.cap = capacity; v.L = n_local; v.S = keys->S; v.K = keys->K; v.masks = keys->d_sets + keys->nsets; v.nsets = keys->nsets;
  v.loc4 = 0;
  for (int i = 0; i < 8; ++i) { v.loc[i] = i < n_local ? h_local[i] : 0; v.loc4 |= (uint32_t)v.loc[i] << (4 * i); }
  p->mem_bytes = mpe::psg::layout(v, nullptr);
  hipError_t e = hipMalloc(&p->mem, p->mem_bytes);
  if (e != hipSuccess) { delete p; mpe_set_error("hipMalloc(presignature pool)", e); return MPE_E_NOMEM; }
  (void)mpe::psg::layout(v, (char*)p->mem);
  e = hipMemset(p->mem, 0, p->mem_bytes);                // every slot EMPTY
  if (e != hipSuccess) { (void)hipFree(p->mem); delete p; mpe_set_error("hipMemset(presignature pool)", e); return MPE_E_HIP; }
  *out = p;
  return MPE_OK;
}

int mpe_gg20_presig_pool_destroy(mpe_gg20_presig_pool* p) {
  if (!p) return MPE_E_ARG;
  (void)hipDeviceSynchronize();                          // calls on any stream may still use the slots
  (void)hipMemset(p->mem, 0, p->mem_bytes);              // the presignatures do not outlive the pool
  (void)hipDeviceSynchronize();
  (void)hipFree(p->mem);
  delete p;
  return MPE_OK;
}

int mpe_gg20_presig_pool_capacity(const mpe_gg20_presig_pool* p) { return p ? p->v.cap : MPE_E_ARG; }
int mpe_gg20_presig_record_words(const mpe_gg20_presig_pool* p) { return p ? mpe::psg::REC_HEAD + mpe::psg::REC_PARTY * p->v.L : MPE_E_ARG; }

int mpe_gg20_presig_deposit(mpe_gg20_presig_pool* p, mpe_gg20_session* s, const int32_t* d_slot, int32_t* d_status, void* stream) {
  if (!p || !s || !d_slot) return MPE_E_ARG;
  if (s->failed || s->next_round != 7) { mpe_set_error_msg("presig deposit: the session is not behind round 6"); return MPE_E_ARG; }
  if (s->ctx != p->ctx) { mpe_set_error_msg("presig deposit: the session's keys or local parties are not the pool's"); return MPE_E_ARG; }
  return mpe::psg::deposit_into(p, s, d_slot, d_status, (hipStream_t)stream);
}

int mpe_gg20_presign_sets(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const int32_t* d_sigset,
                          const mpe_gg20_nonces* nonces, mpe_gg20_presig_pool* pool, const int32_t* d_slot, int32_t* d_status, int dedup_verify,
                          int chunk, void* stream) {
  if (!ctx || !keys || !nonces || !pool || !d_slot || !d_status || batch < 0) return MPE_E_ARG;
  if (!mpe::psg::holds_every_signer(pool, keys, ctx)) { mpe_set_error_msg("mpe_gg20_presign_sets: the pool is not over these keys with every signer local"); return MPE_E_ARG; }
  const int S = keys->S;
  return mpe::gg::lockstep_pass(ctx, keys, batch, d_keyset, d_sigset, nullptr, nonces, dedup_verify, chunk, stream, [&](const mpe::gg::LockstepChunk& c, hipStream_t st) {
    // the chunk's deposit codes go to the result scratch behind the slabs ([S][Bc] words, B of them used)
    int rc = mpe::psg::deposit_into(pool, c.s, d_slot + c.b0, c.pst, st);
    if (rc == MPE_OK) {
      hipLaunchKernelGGL(mpe::psg::presign_finish_kernel, dim3(mpe::blocks_for(c.B, 64)), dim3(64), 0, st, c.B, S, c.b0, c.s->status, c.pst, d_status);
      rc = mpe::psg::launched("presign_finish_kernel");
    }
    return rc;
  });
}

int mpe_gg20_sign_online(mpe_gg20_presig_pool* p, int count, const int32_t* d_slot, const uint32_t* d_msg, uint32_t* d_r, uint32_t* d_s,
                                int32_t* d_recid, int32_t* d_status, void* stream) {
  if (!p || count < 0 || (count && (!d_slot || !d_msg || !d_r || !d_s || !d_recid))) return MPE_E_ARG;
  if (p->v.L != p->v.S) { mpe_set_error_msg("mpe_gg20_sign_online: the pool does not hold every signer"); return MPE_E_ARG; }
  if (!count) return MPE_OK;
  hipLaunchKernelGGL(mpe::psg::presig_sign_online_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, (hipStream_t)stream, p->v, count, d_slot,
                     d_msg, p->K->y, d_r, d_s, d_recid, d_status);
  return mpe::psg::launched("presig_sign_online_kernel");
}

int mpe_gg20_presig_sign(mpe_gg20_presig_pool* p, int count, const int32_t* d_slot, const uint32_t* d_msg, uint32_t* d_s_i, int32_t* d_status,
                         void* stream) {
  if (!p || count < 0 || (count && (!d_slot || !d_msg || !d_s_i))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  hipLaunchKernelGGL(mpe::psg::presig_sign_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, (hipStream_t)stream, p->v, count, d_slot, d_msg,
                     d_s_i, d_status);
  return mpe::psg::launched("presig_sign_kernel");
}

int mpe_gg20_presig_complete(mpe_gg20_presig_pool* p, int count, const int32_t* d_slot, const uint32_t* d_in, const int64_t* h_in_off,
                             uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, int32_t* d_status, void* stream) {
  if (!p || count < 0 || (count && (!d_slot || !d_in))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  mpe::gg::Slab in;
  in.p = d_in; in.W = mpe::gg::msg_words(p->v.S, p->K->n, 7);
  for (int j = 0; j < 8; ++j) in.off[j] = j < p->v.S ? (h_in_off ? (long long)h_in_off[j] : (long long)j * count) : 0;
  hipLaunchKernelGGL(mpe::psg::presig_complete_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, (hipStream_t)stream, p->v, count, d_slot, in,
                     p->K->y, d_r, d_s, d_recid, d_status);
  return mpe::psg::launched("presig_complete_kernel");
}

int mpe_gg20_presig_export(mpe_gg20_presig_pool* p, int count, const int32_t* d_slot, uint32_t* d_rec, int32_t* d_status, void* stream) {
  if (!p || count < 0 || (count && (!d_slot || !d_rec))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  hipLaunchKernelGGL(mpe::psg::presig_export_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, (hipStream_t)stream, p->v, count, d_slot,
                     p->K->y, d_rec, d_status);
  return mpe::psg::launched("presig_export_kernel");
}

int mpe_gg20_presig_import(mpe_gg20_presig_pool* p, int count, const int32_t* d_slot, const uint32_t* d_rec, int32_t* d_status, void* stream) {
  if (!p || count < 0 || (count && (!d_slot || !d_rec))) return MPE_E_ARG;
  if (!count) return MPE_OK;
  hipLaunchKernelGGL(mpe::psg::presig_import_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, (hipStream_t)stream, p->v, count, d_slot,
                     p->K->y, d_rec, d_status, (const int32_t*)nullptr);
  return mpe::psg::launched("presig_import_kernel");
}

int mpe_gg20_presig_discard(mpe_gg20_presig_pool* p, int count, const int32_t* d_slot, void* stream) {
  if (!p || count < 0 || (count && !d_slot)) return MPE_E_ARG;
  if (!count) return MPE_OK;
  hipLaunchKernelGGL(mpe::psg::presig_discard_kernel, dim3(mpe::blocks_for(count, 64)), dim3(64), 0, (hipStream_t)stream, p->v, count, d_slot);
  return mpe::psg::launched("presig_discard_kernel");
}

int mpe_gg20_presig_pool_audit(mpe_gg20_presig_pool* p, int64_t* h_out, void* stream) {
  if (!p || !h_out) return MPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, 5 * 8);
  if (e != hipSuccess) { mpe_set_error("hipMalloc(presig audit)", e); return MPE_E_NOMEM; }
  (void)hipMemsetAsync(d, 0, 5 * 8, st);
  hipLaunchKernelGGL(mpe::psg::presig_audit_kernel, dim3(mpe::blocks_for(p->v.cap, 64)), dim3(64), 0, st, p->v, d);
  unsigned long long h[5] = {0, 0, 0, 0, 0};
  e = hipMemcpyAsync(h, d, 5 * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d);
  if (e != hipSuccess) { mpe_set_error("mpe_gg20_presig_pool_audit", e); return MPE_E_HIP; }
  for (int j = 0; j < 5; ++j) h_out[j] = (int64_t)h[j];
  return MPE_OK;
}

}  // extern "C"
