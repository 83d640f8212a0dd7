// A signing SERVICE's view of the lock-step composition: batches of `batch` sessions arrive one after another (BASELINE config 4's
// literal shape is a stream of 1 024-session batches) and must not be latency-bound one by one.  The reference runs many
// `OfflineStage`s concurrently on one executor (round_based's AsyncProtocol; state_machine/sign.rs:667-691 runs its parties through
// `Simulation`, and rounds.rs:106,215,323 mark the rounds `is_expensive` so that they go to a blocking pool); the device equivalent:
//
//   * `group` consecutive batches are coalesced into ONE pass of mpe_gg20_sign (a "super-batch"): every heavy launch carries the
//     items of all of them, so the launches are large enough for the efficient lane layouts and fill whole passes of the chip
//     (the merged round-1 ladder launch of 4 x 1 024 sessions is 49 152 + 16 384 items = two full passes of 32 768 resident groups);
//   * `lanes` super-batches are in flight at once, each on ONE stream of its own (no forked streams inside a lane): the
//     latency-bound stretches of one (EC kernels, short ladders, inversions) run under the throughput-bound ladders of another.
//     lanes <= 4 streams in total, so the runtime's default 4 hardware queues never multiplex two lanes onto one queue —
//     no GPU_MAX_HW_QUEUES, no child process (round 4 needed 16 queues and 8 host threads for 13.5 k signatures/s;
//     profiles/r05/pipeline_sweep.jsonl has this design's numbers);
//   * ONE host thread feeds everything: submit() only enqueues — the caller's arrays are copied into the lane's staging arrays
//     behind the lane's running pass, or (submit_seeded) nothing is copied at all: the values of ALL batches of a group are drawn
//     by ONE launch of the device-side sampler (mpe_sample.h) right before the pass.  (Staging the inputs on a stream of their own
//     was built and measured: the sampler's small kernels starve behind the other lane's persistent ladders and the lanes wait for
//     them — 14.8 k against 15.8 k signatures/s; dropped.)
// Results are bit-identical to mpe_gg20_sign on the same inputs: a session's outputs do not depend on its neighbours in a batch.
//
// Failure contract (round 6; the reference reports per session and never loses an error: gg_2020/mod.rs:23-27, rounds.rs:696-713):
// when the pass of a group fails as a whole (MPE_E_NOMEM / MPE_E_HIP from the sampler or from mpe_gg20_sign) EVERY batch of the
// group learns it — its d_status is filled with MPE_GG20_STATUS_PASS_FAILED(rc) and its r / s / recid (/ R) zeroed on the lane's
// stream, the ticket keeps rc, and wait / query / stream_wait / latency_ms / pass_ms of that ticket return it.  The next group is
// not affected.  mpe_gg20_pipeline_inject_fault makes the next passes fail that way (tests).
//
// When does a part-filled group go?  (1) full; (2) flush / wait on one of its tickets; (3) `deadline`: its oldest batch has
// waited T microseconds of host time; (4) `eager`: the lane it would run on is idle — arrival-driven grouping: under a trickle
// every batch starts at once (lowest latency), under load the lanes are busy and the groups fill by themselves.  (3) and (4)
// are evaluated inside every submit / query / poll call — the ONE host thread that drives the pipeline; there is no hidden thread.
// A new group opens on an idle lane if there is one, otherwise on the next lane in turn.
//
// Two kinds of engine share all of the above.  A SIGNING engine's pass is mpe_gg20_sign_sets (a lane stages the batches' signer-set
// indices next to the key-set indices; a group in which no batch names its sets passes NULL and launches what mpe_gg20_sign launches).
// A PRESIG engine's pass is mpe_gg20_presign_sets: rounds 0-6, then the deposit into the ONE pool all lanes share — the slot's
// compare-and-swap (mpe_presig.h) is what makes concurrent deposits of several lanes, and other calls on the pool beside them, safe;
// which slots to name stays the caller's policy.  Its batches have no message and one result array, d_status.  A failed pass fills it with
// PASS_FAILED(rc); the deposit is the last step of a pass, so a pass that failed before it left every slot of the group EMPTY.  The engine
// holds the pool's pointer: it is destroyed before its pool.
// Included by mpe_lib.hip after mpe_presig.h and mpe_sample.h.
#pragma once
#include <chrono>

#include "mpe_sample.h"

struct mpe_gg20_pipeline {
  static constexpr int MAX_LANES = 4, MAX_GROUP = 64, RING = 4096;
  mpe_ctx* parent = nullptr;
  const mpe_gg20_keys* K = nullptr;
  mpe_gg20_presig_pool* pool = nullptr;       // a PRESIG engine: its passes end in the deposit into this pool (mpe_gg20_presign_sets)
  bool every_set = false;                     // the key object holds the secrets of every member of every signer set
  int batch = 0, group = 0, lanes = 0, dedup = 0;
  int64_t deadline_us = -1;                   // < 0: no deadline
  int eager = 0;                              // launch a part-filled group as soon as its lane is idle
  int fail_next = 0, fail_rc = MPE_E_NOMEM;   // fault injection: that many next passes fail with fail_rc
  using Clock = std::chrono::steady_clock;
  struct Out { uint32_t *r, *s, *R; int32_t *recid, *status; };
  struct Lane {
    mpe_ctx* ctx = nullptr;
    hipStream_t st = nullptr;
    mpe_gg20_nonce_buf* stage = nullptr;      // [group * batch] sessions, every signer local
    int32_t *keyset = nullptr, *sigset = nullptr, *slot = nullptr;      // slot: a presig engine's pool slots
    void* blob = nullptr;                     // keyset | sigset | slot | r | s | R | recid | status | fail staging
    size_t blob_bytes = 0;
    Out res{};
    int32_t* fail = nullptr;
    int filled = 0, seeded = 0;               // seeded: slots of the open group whose values the sampler draws (all or none)
    bool any_keyset = false, any_sigset = false;
    bool with_sigset[MAX_GROUP];
    uint8_t seeds[32 * mpe::smp::MAX_SLOTS];
    uint64_t counters[mpe::smp::MAX_SLOTS];
    Out dst[MAX_GROUP];
    uint64_t ticket[MAX_GROUP];
    uint64_t last_ticket = 0;                 // the last batch of the last pass queued on this lane (idle test)
    Clock::time_point oldest;                 // host time of the open group's first submission
  } lane[MAX_LANES];
  struct Ticket { uint64_t id = 0, begin_of = 0; hipEvent_t submitted = nullptr, begin = nullptr, done = nullptr; int lane = -1, rc = MPE_OK; bool launched = false, used = false; };
  Ticket ring[RING];
  int cur = 0;
  uint64_t next_ticket = 1;
  uint64_t launched_groups = 0, launched_by_deadline = 0, launched_by_idle = 0, failed_groups = 0;
};

namespace mpe {
namespace pipe {

static mpe_gg20_pipeline::Ticket* ticket_of(mpe_gg20_pipeline* p, uint64_t id) {
  if (id == 0 || id >= p->next_ticket) return nullptr;
  mpe_gg20_pipeline::Ticket* t = &p->ring[id % mpe_gg20_pipeline::RING];
  return (t->used && t->id == id) ? t : nullptr;
}

// every ticket of a failed pass reports it: status = MPE_GG20_STATUS_PASS_FAILED(rc) for every session, no signature
__global__ void fill_i32_kernel(int32_t* __restrict__ p, int n, int32_t v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
static void wipe_bytes(void* p, size_t n) {                   // not elidable
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < n; ++i) v[i] = 0;
}
static bool lane_idle(mpe_gg20_pipeline* p, int li) {
  mpe_gg20_pipeline::Lane& L = p->lane[li];
  if (!L.last_ticket) return true;
  mpe_gg20_pipeline::Ticket* t = ticket_of(p, L.last_ticket);
  return !t || !t->launched || hipEventQuery(t->done) == hipSuccess;      // (a recycled ring slot: that pass ended long ago)
}

// the open group of lane `li` goes to the device: one pass over filled * batch sessions, then every batch's results to its owner
static int launch_group(mpe_gg20_pipeline* p, int li) {
  mpe_gg20_pipeline::Lane& L = p->lane[li];
  if (L.filled == 0) return MPE_OK;
  const int B = L.filled * p->batch;
  mpe_gg20_nonces Z;
  (void)mpe_gg20_nonces_view(L.stage, &Z);
  const int32_t* ks = (p->K->K > 1 || L.any_keyset) ? L.keyset : nullptr;
  const int32_t* ss = L.any_sigset ? L.sigset : nullptr;      // no batch of the group named its sets: the launches of mpe_gg20_sign
  for (int g = 0; ss && g < L.filled; ++g)                    // a group may mix batches with and without sets: without = set 0
    if (!L.with_sigset[g]) (void)hipMemsetAsync(L.sigset + (size_t)g * p->batch, 0, (size_t)p->batch * 4, L.st);
  if (mpe_gg20_pipeline::Ticket* t0 = ticket_of(p, L.ticket[0])) (void)hipEventRecord(t0->begin, L.st);
  int rc = MPE_OK;
  if (L.seeded) {                               // every value of every batch of the group: one launch of the sampler
    int32_t local[8];
    for (int i = 0; i < p->K->S; ++i) local[i] = i;
    rc = mpe::smp::sample_gg20(L.ctx, p->K, p->batch, L.filled, p->K->S, local, ks, L.seeds, L.counters, &Z, L.fail, L.st, ss);
    // the seeds derive every nonce of their batches: as sensitive as the key share, gone from host memory once the sampler is queued
    // (the kernel arguments were copied at launch)
    wipe_bytes(L.seeds, sizeof L.seeds);
    wipe_bytes(L.counters, sizeof L.counters);
  }
  if (rc == MPE_OK && p->fail_next > 0) {       // fault injection (tests): the pass fails as a whole, after its inputs were staged
    --p->fail_next;
    rc = p->fail_rc;
    mpe_set_error_msg("gg20 pipeline: injected pass failure");
  }
  if (rc == MPE_OK)
    rc = p->pool ? mpe_gg20_presign_sets(L.ctx, p->K, B, ks, ss, &Z, p->pool, L.slot, L.res.status, p->dedup, 0, L.st)
                 : mpe_gg20_sign_sets(L.ctx, p->K, B, ks, ss, &Z, L.res.r, L.res.s, L.res.recid, L.res.R, L.res.status, p->dedup, 0, L.st);
  if (rc == MPE_OK) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { mpe_set_error("gg20 pipeline launch", e); rc = MPE_E_HIP; }
  } else {
    (void)hipGetLastError();
  }
  for (int g = 0; g < L.filled; ++g) {
    const size_t o = (size_t)g * p->batch, nb = (size_t)p->batch;
    const mpe_gg20_pipeline::Out& d = L.dst[g];
    if (p->pool) {                              // a presig engine's one result array
      if (rc == MPE_OK) (void)hipMemcpyAsync(d.status, L.res.status + o, nb * 4, hipMemcpyDeviceToDevice, L.st);
      else hipLaunchKernelGGL(fill_i32_kernel, dim3(mpe::blocks_for((int)nb, 256)), dim3(256), 0, L.st, d.status, (int)nb, (int32_t)MPE_GG20_STATUS_PASS_FAILED(rc));
    } else if (rc == MPE_OK) {
      (void)hipMemcpyAsync(d.r, L.res.r + o * 8, nb * 32, hipMemcpyDeviceToDevice, L.st);
      (void)hipMemcpyAsync(d.s, L.res.s + o * 8, nb * 32, hipMemcpyDeviceToDevice, L.st);
      (void)hipMemcpyAsync(d.recid, L.res.recid + o, nb * 4, hipMemcpyDeviceToDevice, L.st);
      (void)hipMemcpyAsync(d.status, L.res.status + o, nb * 4, hipMemcpyDeviceToDevice, L.st);
      if (d.R) (void)hipMemcpyAsync(d.R, L.res.R + o * 16, nb * 64, hipMemcpyDeviceToDevice, L.st);
    } else {                                    // the owner of EVERY batch of the group reads the failure in its own arrays
      hipLaunchKernelGGL(fill_i32_kernel, dim3(mpe::blocks_for((int)nb, 256)), dim3(256), 0, L.st, d.status, (int)nb, (int32_t)MPE_GG20_STATUS_PASS_FAILED(rc));
      (void)hipMemsetAsync(d.r, 0, nb * 32, L.st);
      (void)hipMemsetAsync(d.s, 0, nb * 32, L.st);
      (void)hipMemsetAsync(d.recid, 0, nb * 4, L.st);
      if (d.R) (void)hipMemsetAsync(d.R, 0, nb * 64, L.st);
    }
  }
  // the staged sampled values (k_i, gamma_i, Paillier randomness) of this group do not wait for the next one to overwrite them,
  // nor do the lane's copies of the signatures (the owners have theirs)
  (void)hipMemsetAsync(L.stage->blob, 0, L.stage->bytes, L.st);
  if (!p->pool) {
    (void)hipMemsetAsync(L.res.r, 0, (size_t)B * 8 * 4, L.st);
    (void)hipMemsetAsync(L.res.s, 0, (size_t)B * 8 * 4, L.st);
  }
  mpe_gg20_pipeline::Ticket* t0 = ticket_of(p, L.ticket[0]);
  for (int g = 0; g < L.filled; ++g) {
    mpe_gg20_pipeline::Ticket* t = ticket_of(p, L.ticket[g]);
    if (!t) continue;
    (void)hipEventRecord(t->done, L.st);
    if (g && t0) t->begin_of = t0->id;
    t->rc = rc;
    t->launched = true;
  }
  L.last_ticket = L.ticket[L.filled - 1];
  L.filled = 0;
  L.seeded = 0;
  L.any_keyset = false;
  L.any_sigset = false;
  p->launched_groups++;
  if (rc != MPE_OK) p->failed_groups++;
  // the next group opens on an idle lane if there is one, otherwise on the next lane in turn
  int next = (li + 1) % p->lanes;
  for (int k = 0; k < p->lanes; ++k) {
    const int c = (li + 1 + k) % p->lanes;
    if (lane_idle(p, c)) { next = c; break; }
  }
  p->cur = next;
  return rc;
}

// rules (3) and (4) of the header comment for the open group; *launched += 1 when it went
static int poll_open_group(mpe_gg20_pipeline* p, int* launched) {
  mpe_gg20_pipeline::Lane& L = p->lane[p->cur];
  if (L.filled == 0) return MPE_OK;
  bool go = false;
  if (p->eager && lane_idle(p, p->cur)) { go = true; p->launched_by_idle++; }
  if (!go && p->deadline_us >= 0 &&
      std::chrono::duration_cast<std::chrono::microseconds>(mpe_gg20_pipeline::Clock::now() - L.oldest).count() >= p->deadline_us) { go = true; p->launched_by_deadline++; }
  if (!go) return MPE_OK;
  if (launched) ++*launched;
  return launch_group(p, p->cur);
}

// common part of the submit forms: reserves slot g of the current lane, records the ticket (a presig engine's batch has d_status alone)
static int open_slot(mpe_gg20_pipeline* p, uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, int32_t* d_status, hipStream_t caller,
                     int* lane_out, int* slot_out, uint64_t* ticket_out) {
  if (!p || !d_status || !ticket_out || (!p->pool && (!d_r || !d_s || !d_recid))) return MPE_E_ARG;
  const uint64_t id = p->next_ticket;
  mpe_gg20_pipeline::Ticket* t = &p->ring[id % mpe_gg20_pipeline::RING];
  if (t->used && (!t->launched || hipEventQuery(t->done) != hipSuccess)) {
    mpe_set_error_msg("gg20 pipeline: more than 4096 batches in flight");
    return MPE_E_ARG;
  }
  for (hipEvent_t* ev : {&t->submitted, &t->begin, &t->done})        // created once per ring slot (a failed creation is retried by the next use)
    if (!*ev && hipEventCreate(ev) != hipSuccess) { *ev = nullptr; mpe_set_error_msg("gg20 pipeline: hipEventCreate"); return MPE_E_HIP; }
  const int li = p->cur;
  mpe_gg20_pipeline::Lane& L = p->lane[li];
  const int g = L.filled;
  t->id = id; t->begin_of = id; t->lane = li; t->rc = MPE_OK; t->launched = false; t->used = true;
  if (g == 0) L.oldest = mpe_gg20_pipeline::Clock::now();
  // the lane reads the caller's arrays only after the caller's stream has produced them
  (void)hipEventRecord(t->submitted, caller);
  (void)hipStreamWaitEvent(L.st, t->submitted, 0);
  L.dst[g] = mpe_gg20_pipeline::Out{d_r, d_s, d_R, d_recid, d_status};
  L.ticket[g] = id;
  p->next_ticket++;
  *lane_out = li; *slot_out = g; *ticket_out = id;
  return MPE_OK;
}
// d_sigset: the batch's signer sets, staged next to the key sets (a batch without them: zeros = set 0); d_slot: a presig engine's pool slots
static int close_slot(mpe_gg20_pipeline* p, int li, const int32_t* d_keyset, const int32_t* d_sigset, const int32_t* d_slot) {
  mpe_gg20_pipeline::Lane& L = p->lane[li];
  const size_t o = (size_t)L.filled * p->batch;
  if (d_keyset) { (void)hipMemcpyAsync(L.keyset + o, d_keyset, (size_t)p->batch * 4, hipMemcpyDeviceToDevice, L.st); L.any_keyset = true; }
  else (void)hipMemsetAsync(L.keyset + o, 0, (size_t)p->batch * 4, L.st);
  if (d_sigset) { (void)hipMemcpyAsync(L.sigset + o, d_sigset, (size_t)p->batch * 4, hipMemcpyDeviceToDevice, L.st); L.any_sigset = true; }
  L.with_sigset[L.filled] = d_sigset != nullptr;      // (launch_group zeroes the rows of the others when the group names sets at all)
  if (d_slot) (void)hipMemcpyAsync(L.slot + o, d_slot, (size_t)p->batch * 4, hipMemcpyDeviceToDevice, L.st);
  L.filled++;
  // a pass that fails is reported through the tickets of its batches (each owner learns it from wait / query and from its
  // status array), not through whichever submit happened to close the group: the submission itself succeeded
  if (L.filled == p->group) (void)launch_group(p, li);
  else (void)poll_open_group(p, nullptr);
  return MPE_OK;
}

}  // namespace pipe
}  // namespace mpe

extern "C" {

int mpe_gg20_pipeline_destroy(mpe_gg20_pipeline* p);

}  // extern "C"

namespace mpe {
namespace pipe {

// pool: NULL for a signing engine, the pool a presig engine deposits into
static int create(mpe_ctx* ctx, const mpe_gg20_keys* keys, mpe_gg20_presig_pool* pool, int batch, int group, int lanes, int dedup_verify, mpe_gg20_pipeline** out) {
  if (!ctx || !keys || !out || batch <= 0 || group < 1 || group > mpe_gg20_pipeline::MAX_GROUP || lanes < 1 || lanes > mpe_gg20_pipeline::MAX_LANES)
    return MPE_E_ARG;
  for (int i = 0; i < keys->S; ++i) if (keys->own_slot[keys->signers[i]] < 0) { mpe_set_error_msg("gg20 pipeline: the key object must hold every signer's secrets"); return MPE_E_ARG; }
  bool every_set = true;                      // the rule of mpe_gg20_sign_sets, asked once here and not pass by pass
  for (int k = 0; k < keys->nsets; ++k)
    for (int i = 0; i < keys->S; ++i) every_set = every_set && keys->own_slot[(keys->sets4[k] >> (4 * i)) & 15u] >= 0;
  if (pool && !every_set) { mpe_set_error_msg("gg20 pipeline: the key object must hold the secrets of every member of every signer set"); return MPE_E_ARG; }
  mpe_gg20_pipeline* p = new (std::nothrow) mpe_gg20_pipeline();
  if (!p) return MPE_E_NOMEM;
  p->parent = ctx; p->K = keys; p->pool = pool; p->every_set = every_set; p->batch = batch; p->group = group; p->lanes = lanes; p->dedup = dedup_verify ? 1 : 0;
  const size_t GB = (size_t)group * batch;
  int rc = MPE_OK;
  for (int li = 0; li < lanes && rc == MPE_OK; ++li) {
    mpe_gg20_pipeline::Lane& L = p->lane[li];
    rc = mpe_ctx_create(&L.ctx, ctx->device);
    if (rc != MPE_OK) break;
    // a lane is the parent context with a workspace of its own and NO forked streams (one stream per lane: <= 4 in total)
    mpe_ctx* c = L.ctx;
    mpe::ctx_copy_options(c, ctx);            // every option of the parent (mpe_ctx_set_option), then:
    c->enc = ctx->enc;
    c->allow_par = false;
    c->use_prio = 0;                          // the lanes' ladders compete with each other, not with side work of their own pass
    if (hipStreamCreateWithFlags(&L.st, hipStreamNonBlocking) != hipSuccess) { mpe_set_error_msg("gg20 pipeline: hipStreamCreate"); rc = MPE_E_HIP; break; }
    rc = mpe_gg20_nonces_alloc(c, keys, (int)GB, keys->S, &L.stage);
    if (rc != MPE_OK) break;
    const size_t words = GB * (3 + 8 + 8 + 16 + 1 + 1) + 64;
    L.blob_bytes = words * 4;
    if (hipMalloc(&L.blob, L.blob_bytes) != hipSuccess) { mpe_set_error_msg("gg20 pipeline: hipMalloc(staging)"); rc = MPE_E_NOMEM; break; }
    (void)hipMemset(L.blob, 0, L.blob_bytes);
    uint32_t* w = (uint32_t*)L.blob;
    L.keyset = (int32_t*)w; w += GB; L.sigset = (int32_t*)w; w += GB; L.slot = (int32_t*)w; w += GB;
    L.res.r = w; w += GB * 8; L.res.s = w; w += GB * 8; L.res.R = w; w += GB * 16;
    L.res.recid = (int32_t*)w; w += GB; L.res.status = (int32_t*)w; w += GB;
    L.fail = (int32_t*)w;
  }
  if (rc != MPE_OK) { mpe_gg20_pipeline_destroy(p); return rc; }
  *out = p;
  return MPE_OK;
}
// the refusals every submit form shares, BEFORE a slot or a ticket is taken: the engine's kind, the key sets, the signer sets
static int submit_refused(const mpe_gg20_pipeline* p, bool presig, const int32_t* d_keyset, const int32_t* d_sigset) {
  if ((p->pool != nullptr) != presig) { mpe_set_error_msg("gg20 pipeline: a signing engine takes submit / submit_seeded, a presig engine submit_presig / submit_presig_seeded"); return MPE_E_ARG; }
  if (p->K->K > 1 && !d_keyset) return MPE_E_ARG;
  if (d_sigset && !p->every_set) { mpe_set_error_msg("gg20 pipeline: signer sets need the secrets of every member of every set in the key object"); return MPE_E_ARG; }
  return MPE_OK;
}
// the caller-sampled forms: the first `fields` arrays of the batch go to slot g of the lane's staging (msg is the last field)
static int stage_nonces(mpe_gg20_pipeline* p, int li, int g, const mpe_gg20_nonces* src, int fields) {
  mpe_gg20_pipeline::Lane& L = p->lane[li];
  const mpe_gg20_nonce_buf* sb = L.stage;
  for (int f = 0; f < fields; ++f) {
    const gg::NonceField& F = gg::NONCE_FIELDS[f];
    const size_t w = gg::nonce_words(F, sb->S, sb->n, sb->L, p->batch);
    (void)hipMemcpyAsync(const_cast<uint32_t*>(sb->view.*F.ptr) + (size_t)g * w, src->*F.ptr, w * 4, hipMemcpyDeviceToDevice, L.st);
  }
  return MPE_OK;
}
static const char* const MIXED_FORMS = "gg20 pipeline: a group holds seeded or caller-sampled batches, not both (flush between the two forms)";

}  // namespace pipe
}  // namespace mpe

extern "C" {

int mpe_gg20_pipeline_create(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, int group, int lanes, int dedup_verify, mpe_gg20_pipeline** out) {
  return mpe::pipe::create(ctx, keys, nullptr, batch, group, lanes, dedup_verify, out);
}
int mpe_gg20_pipeline_create_presig(mpe_ctx* ctx, const mpe_gg20_keys* keys, mpe_gg20_presig_pool* pool, int batch, int group, int lanes,
                                    int dedup_verify, mpe_gg20_pipeline** out) {
  if (!ctx || !keys || !pool) return MPE_E_ARG;
  if (!mpe::psg::holds_every_signer(pool, keys, ctx)) { mpe_set_error_msg("gg20 pipeline: the pool is not over these keys with every signer local"); return MPE_E_ARG; }
  return mpe::pipe::create(ctx, keys, pool, batch, group, lanes, dedup_verify, out);
}

int mpe_gg20_pipeline_destroy(mpe_gg20_pipeline* p) {
  if (!p) return MPE_E_ARG;
  for (int li = 0; li < p->lanes; ++li) {
    mpe_gg20_pipeline::Lane& L = p->lane[li];
    if (L.st) (void)hipStreamSynchronize(L.st);
    if (L.stage) (void)mpe_gg20_nonces_free(L.stage);
    if (L.blob) { (void)hipMemset(L.blob, 0, L.blob_bytes); (void)hipFree(L.blob); }
    if (L.ctx) (void)mpe_ctx_destroy(L.ctx);
    if (L.st) (void)hipStreamDestroy(L.st);
    mpe::pipe::wipe_bytes(L.seeds, sizeof L.seeds);
    mpe::pipe::wipe_bytes(L.counters, sizeof L.counters);
  }
  for (auto& t : p->ring) { if (t.submitted) (void)hipEventDestroy(t.submitted); if (t.begin) (void)hipEventDestroy(t.begin); if (t.done) (void)hipEventDestroy(t.done); }
  delete p;
  return MPE_OK;
}

int mpe_gg20_pipeline_submit(mpe_gg20_pipeline* p, const int32_t* d_keyset, const mpe_gg20_nonces* nonces, uint32_t* d_r, uint32_t* d_s, int32_t* d_recid,
                             uint32_t* d_R, int32_t* d_status, void* stream, uint64_t* ticket) {
  return mpe_gg20_pipeline_submit_sets(p, d_keyset, nullptr, nonces, d_r, d_s, d_recid, d_R, d_status, stream, ticket);
}
int mpe_gg20_pipeline_submit_sets(mpe_gg20_pipeline* p, const int32_t* d_keyset, const int32_t* d_sigset, const mpe_gg20_nonces* nonces, uint32_t* d_r,
                                  uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, int32_t* d_status, void* stream, uint64_t* ticket) {
  if (!p || !nonces) return MPE_E_ARG;
  // every refusal comes BEFORE a slot and a ticket are taken: a refused call leaves the pipeline as it was
  MPE_TRY(mpe::pipe::submit_refused(p, false, d_keyset, d_sigset));
  if (mpe::gg::nonces_missing(*nonces, mpe::gg::NF)) { mpe_set_error_msg("gg20 pipeline: a nonce array is NULL"); return MPE_E_ARG; }
  (void)mpe::pipe::poll_open_group(p, nullptr);
  if (p->lane[p->cur].seeded) { mpe_set_error_msg(mpe::pipe::MIXED_FORMS); return MPE_E_ARG; }
  int li = 0, g = 0;
  MPE_TRY(mpe::pipe::open_slot(p, d_r, d_s, d_recid, d_R, d_status, (hipStream_t)stream, &li, &g, ticket));
  (void)mpe::pipe::stage_nonces(p, li, g, nonces, mpe::gg::NF);
  return mpe::pipe::close_slot(p, li, d_keyset, d_sigset, nullptr);
}

int mpe_gg20_pipeline_submit_seeded(mpe_gg20_pipeline* p, const int32_t* d_keyset, const uint8_t* h_seed32, uint64_t batch_counter, const uint32_t* d_msg,
                                    uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, int32_t* d_status, void* stream, uint64_t* ticket) {
  return mpe_gg20_pipeline_submit_seeded_sets(p, d_keyset, nullptr, h_seed32, batch_counter, d_msg, d_r, d_s, d_recid, d_R, d_status, stream, ticket);
}
int mpe_gg20_pipeline_submit_seeded_sets(mpe_gg20_pipeline* p, const int32_t* d_keyset, const int32_t* d_sigset, const uint8_t* h_seed32, uint64_t batch_counter,
                                         const uint32_t* d_msg, uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, int32_t* d_status, void* stream,
                                         uint64_t* ticket) {
  if (!p || !h_seed32 || !d_msg || (batch_counter >> 56) != 0) return MPE_E_ARG;
  MPE_TRY(mpe::pipe::submit_refused(p, false, d_keyset, d_sigset));
  if (p->group > mpe::smp::MAX_SLOTS) { mpe_set_error_msg("gg20 pipeline: seeded submission needs group <= 16 (one sampler launch per group)"); return MPE_E_ARG; }
  (void)mpe::pipe::poll_open_group(p, nullptr);
  if (p->lane[p->cur].filled != p->lane[p->cur].seeded) { mpe_set_error_msg(mpe::pipe::MIXED_FORMS); return MPE_E_ARG; }
  int li = 0, g = 0;
  MPE_TRY(mpe::pipe::open_slot(p, d_r, d_s, d_recid, d_R, d_status, (hipStream_t)stream, &li, &g, ticket));
  mpe_gg20_pipeline::Lane& L = p->lane[li];
  (void)hipMemcpyAsync(const_cast<uint32_t*>(L.stage->view.msg) + (size_t)g * p->batch * 8, d_msg, (size_t)p->batch * 32, hipMemcpyDeviceToDevice, L.st);
  memcpy(L.seeds + 32 * g, h_seed32, 32);
  L.counters[g] = batch_counter;
  L.seeded++;
  return mpe::pipe::close_slot(p, li, d_keyset, d_sigset, nullptr);
}

// The presig engine's two forms: no message, d_slot [batch] staged like d_keyset, d_status the one result array.
int mpe_gg20_pipeline_submit_presig(mpe_gg20_pipeline* p, const int32_t* d_keyset, const int32_t* d_sigset, const mpe_gg20_nonces* nonces, const int32_t* d_slot,
                                    int32_t* d_status, void* stream, uint64_t* ticket) {
  if (!p || !nonces || !d_slot) return MPE_E_ARG;
  MPE_TRY(mpe::pipe::submit_refused(p, true, d_keyset, d_sigset));
  const int fields = mpe::gg::NF - 1;                  // (msg, the last field, is not read)
  if (mpe::gg::nonces_missing(*nonces, fields)) { mpe_set_error_msg("gg20 pipeline: a nonce array is NULL"); return MPE_E_ARG; }
  (void)mpe::pipe::poll_open_group(p, nullptr);
  if (p->lane[p->cur].seeded) { mpe_set_error_msg(mpe::pipe::MIXED_FORMS); return MPE_E_ARG; }
  int li = 0, g = 0;
  MPE_TRY(mpe::pipe::open_slot(p, nullptr, nullptr, nullptr, nullptr, d_status, (hipStream_t)stream, &li, &g, ticket));
  (void)mpe::pipe::stage_nonces(p, li, g, nonces, fields);
  return mpe::pipe::close_slot(p, li, d_keyset, d_sigset, d_slot);
}
int mpe_gg20_pipeline_submit_presig_seeded(mpe_gg20_pipeline* p, const int32_t* d_keyset, const int32_t* d_sigset, const uint8_t* h_seed32, uint64_t batch_counter,
                                           const int32_t* d_slot, int32_t* d_status, void* stream, uint64_t* ticket) {
  if (!p || !h_seed32 || !d_slot || (batch_counter >> 56) != 0) return MPE_E_ARG;
  MPE_TRY(mpe::pipe::submit_refused(p, true, d_keyset, d_sigset));
  if (p->group > mpe::smp::MAX_SLOTS) { mpe_set_error_msg("gg20 pipeline: seeded submission needs group <= 16 (one sampler launch per group)"); return MPE_E_ARG; }
  (void)mpe::pipe::poll_open_group(p, nullptr);
  if (p->lane[p->cur].filled != p->lane[p->cur].seeded) { mpe_set_error_msg(mpe::pipe::MIXED_FORMS); return MPE_E_ARG; }
  int li = 0, g = 0;
  MPE_TRY(mpe::pipe::open_slot(p, nullptr, nullptr, nullptr, nullptr, d_status, (hipStream_t)stream, &li, &g, ticket));
  mpe_gg20_pipeline::Lane& L = p->lane[li];
  memcpy(L.seeds + 32 * g, h_seed32, 32);
  L.counters[g] = batch_counter;
  L.seeded++;
  return mpe::pipe::close_slot(p, li, d_keyset, d_sigset, d_slot);
}

int mpe_gg20_pipeline_flush(mpe_gg20_pipeline* p) {
  if (!p) return MPE_E_ARG;
  int rc = MPE_OK;
  for (int k = 0; k < p->lanes; ++k) {
    const int li = (p->cur + k) % p->lanes;
    if (p->lane[li].filled) { const int r = mpe::pipe::launch_group(p, li); if (rc == MPE_OK) rc = r; }
  }
  return rc;
}

int mpe_gg20_pipeline_query(mpe_gg20_pipeline* p, uint64_t ticket, int* done) {
  if (!p || !done) return MPE_E_ARG;
  mpe_gg20_pipeline::Ticket* t = mpe::pipe::ticket_of(p, ticket);
  if (!t) return MPE_E_ARG;
  if (!t->launched) (void)mpe::pipe::poll_open_group(p, nullptr);
  *done = (t->launched && hipEventQuery(t->done) == hipSuccess) ? 1 : 0;
  return (*done && t->rc != MPE_OK) ? t->rc : MPE_OK;           // a completed batch whose pass failed says so
}

int mpe_gg20_pipeline_wait(mpe_gg20_pipeline* p, uint64_t ticket) {
  if (!p) return MPE_E_ARG;
  mpe_gg20_pipeline::Ticket* t = mpe::pipe::ticket_of(p, ticket);
  if (!t) return MPE_E_ARG;
  if (!t->launched) (void)mpe::pipe::launch_group(p, t->lane);          // its group is still open: it goes now, partly filled
  const hipError_t e = hipEventSynchronize(t->done);
  if (e != hipSuccess) { mpe_set_error("gg20 pipeline wait", e); return MPE_E_HIP; }
  if (t->rc != MPE_OK) mpe_set_error_msg("gg20 pipeline: the pass that carried this batch failed (status arrays hold MPE_GG20_STATUS_PASS_FAILED)");
  return t->rc;
}

int mpe_gg20_pipeline_stream_wait(mpe_gg20_pipeline* p, uint64_t ticket, void* stream) {
  if (!p) return MPE_E_ARG;
  mpe_gg20_pipeline::Ticket* t = mpe::pipe::ticket_of(p, ticket);
  if (!t) return MPE_E_ARG;
  if (!t->launched) (void)mpe::pipe::launch_group(p, t->lane);
  const hipError_t e = hipStreamWaitEvent((hipStream_t)stream, t->done, 0);
  if (e != hipSuccess) { mpe_set_error("gg20 pipeline stream wait", e); return MPE_E_HIP; }
  return t->rc;                                                          // known at launch time: the failure is not asynchronous
}

int mpe_gg20_pipeline_latency_ms(mpe_gg20_pipeline* p, uint64_t ticket, float* ms) {
  if (!p || !ms) return MPE_E_ARG;
  mpe_gg20_pipeline::Ticket* t = mpe::pipe::ticket_of(p, ticket);
  if (!t || !t->launched) return MPE_E_ARG;
  hipError_t e = hipEventSynchronize(t->done);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, t->submitted, t->done);
  if (e != hipSuccess) { mpe_set_error("gg20 pipeline latency", e); return MPE_E_HIP; }
  return t->rc;
}

int mpe_gg20_pipeline_pass_ms(mpe_gg20_pipeline* p, uint64_t ticket, float* ms) {
  if (!p || !ms) return MPE_E_ARG;
  mpe_gg20_pipeline::Ticket* t = mpe::pipe::ticket_of(p, ticket);
  if (!t || !t->launched) return MPE_E_ARG;
  mpe_gg20_pipeline::Ticket* t0 = mpe::pipe::ticket_of(p, t->begin_of);
  if (!t0) return MPE_E_ARG;
  hipError_t e = hipEventSynchronize(t->done);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, t0->begin, t->done);
  if (e != hipSuccess) { mpe_set_error("gg20 pipeline pass time", e); return MPE_E_HIP; }
  return t->rc;
}

int mpe_gg20_pipeline_ticket_rc(mpe_gg20_pipeline* p, uint64_t ticket, int* launched, int* rc) {
  if (!p || !rc) return MPE_E_ARG;
  mpe_gg20_pipeline::Ticket* t = mpe::pipe::ticket_of(p, ticket);
  if (!t) return MPE_E_ARG;
  if (launched) *launched = t->launched ? 1 : 0;
  *rc = t->launched ? t->rc : MPE_OK;
  return MPE_OK;
}

int mpe_gg20_pipeline_set_deadline_us(mpe_gg20_pipeline* p, int64_t us) {
  if (!p) return MPE_E_ARG;
  p->deadline_us = us < 0 ? -1 : us;
  return MPE_OK;
}
int mpe_gg20_pipeline_set_eager(mpe_gg20_pipeline* p, int on) {
  if (!p) return MPE_E_ARG;
  p->eager = on ? 1 : 0;
  return MPE_OK;
}
int mpe_gg20_pipeline_poll(mpe_gg20_pipeline* p, int* launched) {
  if (!p) return MPE_E_ARG;
  if (launched) *launched = 0;
  (void)mpe::pipe::poll_open_group(p, launched);                // a failed pass is its tickets' news
  return MPE_OK;
}
int mpe_gg20_pipeline_inject_fault(mpe_gg20_pipeline* p, int passes, int rc) {
  if (!p || passes < 0 || (rc != MPE_E_NOMEM && rc != MPE_E_HIP)) return MPE_E_ARG;
  p->fail_next = passes;
  p->fail_rc = rc;
  return MPE_OK;
}
int mpe_gg20_pipeline_counters(const mpe_gg20_pipeline* p, uint64_t* groups, uint64_t* by_deadline, uint64_t* by_idle, uint64_t* failed) {
  if (!p) return MPE_E_ARG;
  if (groups) *groups = p->launched_groups;
  if (by_deadline) *by_deadline = p->launched_by_deadline;
  if (by_idle) *by_idle = p->launched_by_idle;
  if (failed) *failed = p->failed_groups;
  return MPE_OK;
}

int mpe_gg20_pipeline_sampler_failures(mpe_gg20_pipeline* p, int32_t* h_out) {
  if (!p || !h_out) return MPE_E_ARG;
  int32_t tot = 0;
  for (int li = 0; li < p->lanes; ++li) {
    int32_t v = 0;
    (void)hipStreamSynchronize(p->lane[li].st);
    if (hipMemcpy(&v, p->lane[li].fail, 4, hipMemcpyDeviceToHost) != hipSuccess) return MPE_E_HIP;
    tot += v;
  }
  *h_out = tot;
  return MPE_OK;
}

}  // extern "C"
