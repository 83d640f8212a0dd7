/* mpecdsa_hip.h — C-ABI of the MI355X (gfx950) batched crypto core for GG20 threshold signing.
 *
 * Drop-in boundary: the reference (ZenGo-X/multi-party-ecdsa v0.8.1) has no FFI of
 * its own on this path; its arithmetic leaves the crate through curv-kzen / kzen-paillier method
 * calls.  Every entry point below is the batched equivalent of one such call and cites the call
 * site(s) it replaces.  A Rust shim crate that re-exports the curv/paillier names would bind these
 * with `extern "C"`.
 *
 * Conventions
 *  - Big integers cross the boundary as fixed-width little-endian arrays of uint32_t words
 *    ("interface words"): 64 words = 2048 bit, 128 words = 4096 bit.  A batch is item-major:
 *    item i occupies words [i*K32, (i+1)*K32).
 *  - All data pointers are DEVICE pointers (HBM-resident); the library never allocates or frees
 *    caller memory.  `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *    are asynchronous with respect to the host unless stated otherwise.
 *  - Return value: 0 = ok, negative = MPE_E_* (argument/launch errors).  Verifiers additionally
 *    write a per-item uint8_t ok[] (1 = accept) — the batched form of the reference's
 *    bool / Result<(), Error> returns; one bad item never aborts the batch.
 *  - No mutable global state: distinct mpe_ctx may be used from distinct host threads / streams at the same time
 *    (tests/test_threads_gpu.py).  The environment is read only inside mpe_ctx_create; mpe_last_error() is per thread.
 *
 * Two caveats a binder must know
 *  - RECALLED conventions.  curv-kzen 0.9, kzen-paillier 0.4.2 and zk-paillier 0.4.3 are not vendored with the reference
 *    (Cargo.toml:36-47), so these byte-level details are believed, not read: DigestExt::chain_point hashing the 65-byte
 *    uncompressed point; BigInt::to_bytes(0) = one 0x00 byte; the order of the points in the challenges of DLogProof,
 *    PedersenProof, HomoELGamalProof, ECDDHProof; zk-paillier's SALT_STRING, mask_generation block order and
 *    CompositeDLogProof field order; the serde forms of BigInt / Point / Scalar (host side only: multi_party_ecdsa_amd/wire.py).
 *    Each is a run-time field of `mpe_encoding` (mpe_ctx_set_encoding below), exercised in every alternative by the tests;
 *    tools/diagnose_encodings.py finds the profile of the real crates from one dump of vectors (tools/rust_vectors/run.sh).
 *  - Side channels.  No secret-dependent control flow (fixed window schedules, masked selects; the one exponent whose bits
 *    steer the operation sequence is the PUBLIC key N), but window tables in HBM are indexed by secret exponent windows:
 *    the kernels are NOT constant-time against a co-tenant observing memory-access patterns on the same GPU.  Deploy on a
 *    GPU dedicated to the signing service.  (The reference's mpz_powm makes no constant-time claim either.)
 */
#ifndef MPECDSA_HIP_H
#define MPECDSA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPE_OK 0
#define MPE_E_ARG (-1)     /* bad argument (NULL pointer, unsupported width, ...) */
#define MPE_E_HIP (-2)     /* HIP runtime error; see mpe_last_error() */
#define MPE_E_NOMEM (-3)

typedef struct mpe_ctx mpe_ctx;         /* per-thread/stream context: owns scratch (window tables) */
typedef struct mpe_modset mpe_modset;   /* a set of moduli with their Montgomery constants in HBM */

/* Library / device info.  mpe_version() never touches the GPU. */
const char* mpe_version(void);
const char* mpe_last_error(void);

int mpe_ctx_create(mpe_ctx** out, int device);
int mpe_ctx_destroy(mpe_ctx* ctx);
/* Zeroes the scratch the context owns (window tables of secret bases, nonce-derived intermediates of composite calls);
 * the reference zeroizes its round-1 secrets (src/utilities/mta/range_proofs.rs:26-36,197-212).  Also done by destroy. */
int mpe_ctx_wipe(mpe_ctx* ctx, void* stream);
/* Audit of the wiping: the number of non-zero 32-bit words in every scratch region the context owns (window tables,
 * composite workspace, cached GG20 session arena and message slabs) and their total size.  Synchronises the stream. */
int mpe_ctx_scratch_audit(mpe_ctx* ctx, uint64_t* nonzero_words, uint64_t* total_bytes, void* stream);
/* A hint for callers that run SEVERAL contexts on one device at the same time (one host thread and stream each).  A single small
 * batch is latency-bound, so by default a context spreads each big integer of a small launch over 2x / 4x the lanes (less efficient,
 * shorter); with `contexts` > 1 the small-batch heuristics compare a launch with 1/contexts of the chip and keep the efficient
 * layouts.  MEASURED (profiles/r04/stream_sweep*.log): the hint LOSES 7-20 % at every depth from 2 to 24 contexts — concurrent small
 * batches are bound by how many kernels run side by side, and the wide layouts fill the chip with fewer of them.  It is kept for
 * experiments only (results are identical whatever the value; default 1).  The supported way to serve a stream of small batches is
 * mpe_gg20_pipeline_* below: one handle, one host thread, batches coalesced per pass. */
int mpe_ctx_set_device_share(mpe_ctx* ctx, int contexts);
/* Run-time options: the A/B switches every "x vs y" figure of DESIGN.md was measured with.  The library reads NO environment
 * variable; a context starts with the shipped defaults and changes only through this call (before the objects that depend on the
 * option are created: e.g. fb_window_bits before mpe_statements_create / mpe_gg20_keys_create).  None changes a result.
 *   0/1 switches   no_fixed_base no_crt no_multiexp no_pair no_pown no_sliding no_par no_wide no_ec_lane_groups
 *                  no_adaptive_lanes (= no_wide + no_ec_lane_groups) no_merge_xn no_merge_r1 gg20_trace
 *                  no_r1_inversion_ahead no_r1_dlog_first (mpe_gg20_sign on small batches: round 0 no longer inverts the ciphertexts
 *                  round 1 needs / MessageB's DLog proofs go behind the ladders again)  no_pdl_ahead (round 4 computes the PDL
 *                  proofs' beta^N itself instead of finding it done)  no_prio (no s_setprio in the ladder kernels)
 *                  no_crt_n (the provers' r^e mod N on the 2048-bit ladder instead of through p | q)
 *                  no_r5_self_crt (a verifier checks the PDL proofs made under its OWN key on the public key, like everybody else's,
 *                  instead of through p^2 | q^2: GG20 round 5, mpe_pdl_verify with a private key object)
 *   integers       fb_window_bits 4..16 | window_bits 0 (auto), 2..6 | wide_div 1..64 | xwide_div 0 (off).. | waves_per_cu 1..8
 *                  fb_budget_mb | fb_split 0 (auto)..64 | sampler_max_attempts 1.. (default 128)
 *                  safe_pass_log 16..26 (default 24: mpe_sample_safe_prime fills a pass with about 2^24 candidates)
 *   names          grid = equal | full | hybrid
 * MPE_E_ARG (and mpe_last_error) for an unknown key or a value out of range.  mpe_ctx_get_option returns the integer form;
 * mpe_ctx_option_count / _name enumerate the integer-valued keys. */
int mpe_ctx_set_option(mpe_ctx* ctx, const char* key, const char* value);
int mpe_ctx_get_option(const mpe_ctx* ctx, const char* key, long* value);
int mpe_ctx_option_count(void);
const char* mpe_ctx_option_name(int i);
/* Blocks the host until everything queued on `stream` has finished (hipStreamSynchronize). */
int mpe_sync(mpe_ctx* ctx, void* stream);

/* ---- byte-level conventions of the un-vendored crates -------------------------------------------------------------------
 * The reference pulls curv-kzen 0.9, kzen-paillier 0.4.2 and zk-paillier 0.4.3 from crates.io (Cargo.toml:36-47); none is
 * vendored under /root/reference, so the byte strings their Fiat-Shamir transcripts hash are RECALLED, not read.  Every such
 * convention is a run-time property of a context — never a build-time constant — so that the day a vector dumped from the
 * real crates (tools/rust_vectors/run.sh -> tests/golden/ref_vectors.json) disagrees with a default below, the fix is one
 * mpe_ctx_set_encoding call, not a kernel edit.  tools/diagnose_encodings.py reads such a dump and prints the profile the
 * crates actually use.  The defaults are what this repository believes curv 0.9 does.
 *
 * What is NOT here because the reference's own source fixes it: AliceProof / BobProof / PDLwSlackProof transcripts
 * (range_proofs.rs:143-150,175-182,375-405; zk_pdl_with_slack/mod.rs:102-110: chain_bigint of every field, points as
 * BigInt::from_bytes(to_bytes(true))) and the message of the HashCommitment (party_i.rs:577-580: the compressed point as a
 * BigInt).  They depend on the crates only through `zero_bytes`. */
typedef struct mpe_encoding {
  uint8_t chain_point;      /* curv `DigestExt::chain_point(P)` (DLogProof mta/mod.rs:147-148,170-171; PedersenProof party_i.rs:620-634;
                             * HomoELGamalProof :778-833; ECDDHProof blame.rs:258-320):
                             * 0 = P.to_bytes(false), 65 bytes 04|x|y (default);  1 = P.to_bytes(true), 33 bytes 02/03|x */
  uint8_t zero_bytes;       /* `BigInt::to_bytes()` of the value 0, as hashed by chain_bigint / zk-paillier's compute_digest:
                             * 0 = one 0x00 byte (rust-gmp exports sizeinbase(0) = 1 digit; default);  1 = the empty string */
  uint8_t ck_mask_order;    /* zk-paillier `mask_generation` of NiCorrectKeyProof (party_i.rs:283-301): the 256-bit blocks
                             * H(seed, j), j = 0.. are combined as  0 = sum_j H(seed, j) << (256 j) (default);
                             * 1 = H(seed, 0) || H(seed, 1) || ... (block 0 most significant) */
  uint8_t reserved;         /* must be 0 */
  uint32_t ck_salt;         /* NiCorrectKeyProof's salt as an integer: SALT_STRING = b"KZen" = 0x4B5A656E (default) */
  /* order of the points inside the challenge hash of each curv sigma proof: ord[i] = index (into the canonical list named
   * here) of the point hashed i-th; the default is the identity.  Unused tail entries are ignored. */
  uint8_t ord_dlog[4];      /* DLogProof        (R = pk_t_rand_commitment, G, pk) */
  uint8_t ord_pedersen[8];  /* PedersenProof    (g, h, com, a1, a2) */
  uint8_t ord_heg[8];       /* HomoELGamalProof (T, A3, G, H, Y, D, E) */
  uint8_t ord_ecddh[8];     /* ECDDHProof       (g1, h1, g2, h2, a1, a2) */
  uint8_t ord_cdlog[4];     /* zk-paillier CompositeDLogProof challenge, BigInts (x, g, N, ni)  (party_i.rs:219-258) */
} mpe_encoding;
/* Fills *out with the defaults above.  Never touches the GPU. */
void mpe_encoding_default(mpe_encoding* out);
/* Installs / reads the profile of a context.  set returns MPE_E_ARG unless every flag is 0/1 and every ord_* prefix is a
 * permutation.  Takes effect for every later call on the context (objects created earlier hold no encoded state). */
int mpe_ctx_set_encoding(mpe_ctx* ctx, const mpe_encoding* enc);
int mpe_ctx_get_encoding(const mpe_ctx* ctx, mpe_encoding* out);

/* ---- moduli ------------------------------------------------------------------------------ */
/* Precomputes, ON THE GPU, the Montgomery constants of `count` odd moduli of `bits` (2048|4096)
 * bits: n in the kernel's internal radix, -n^-1, R mod n, R^2 mod n.  In the reference these are
 * rebuilt inside every mpz_powm call; per-key reuse is output-identical.
 * d_moduli: [count][bits/32] interface words.  Moduli must be odd and >= 3. */
int mpe_modset_create(mpe_ctx* ctx, int bits, int count, const uint32_t* d_moduli,
                      mpe_modset** out, void* stream);
int mpe_modset_destroy(mpe_modset* ms);
int mpe_modset_count(const mpe_modset* ms);
int mpe_modset_bits(const mpe_modset* ms);

/* ---- BigInt::mod_pow --------------------------------------------------------------------- */
/* out[i] = base[i] ^ exp[i] mod modulus[idx(i)]           (curv `BigInt::mod_pow` == mpz_powm;
 * reference call sites: src/utilities/mta/range_proofs.rs:52-57,86,122-141,238-249,291,339-372;
 * src/utilities/zk_pdl_with_slack/mod.rs:189-195).
 *  d_mod_idx : per-item index into `ms`, or NULL meaning idx(i) = (count==1 ? 0 : i).
 *  d_base    : [batch][bits/32], any value < 2^bits (need not be reduced).
 *  d_exp     : [batch][exp_words] little-endian words, exponent >= 0.
 *  d_out     : [batch][bits/32], canonical residue in [0, n).
 * Fixed windows (4/5/6 bits by exponent length), constant sequence of operations for a given exp_words
 * (exponents on this path are secret nonces). */
int mpe_modexp(mpe_ctx* ctx, const mpe_modset* ms, int batch, const int32_t* d_mod_idx,
               const uint32_t* d_base, const uint32_t* d_exp, int exp_words, uint32_t* d_out,
               void* stream);
/* out[i] = base[i]^exp[i] * base2[i]^exp2[i] mod modulus[idx(i)]: the `mod_pow(..) * mod_pow(..) % n` pattern of
 * the verifiers (range_proofs.rs:134-141, zk_pdl_with_slack/mod.rs:144-157) on ONE ladder — the squarings are
 * shared, the residue is the same.  exp2 must be the short one: 32*exp2_words < 32*exp_words - 6. */
int mpe_modexp2(mpe_ctx* ctx, const mpe_modset* ms, int batch, const int32_t* d_mod_idx,
                const uint32_t* d_base, const uint32_t* d_exp, int exp_words,
                const uint32_t* d_base2, const uint32_t* d_exp2, int exp2_words, uint32_t* d_out, void* stream);

/* out[i] = a[i] * b[i] mod modulus[idx(i)]   (curv `BigInt::mod_mul`,
 * src/utilities/zk_pdl_with_slack/mod.rs:198; also Paillier::add = mulmod N^2, mta/mod.rs:145) */
int mpe_modmul(mpe_ctx* ctx, const mpe_modset* ms, int batch, const int32_t* d_mod_idx,
               const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, void* stream);

/* ---- kzen-paillier ------------------------------------------------------------------------ */
/* A set of Paillier-2048 keys resident in HBM.  Public sets hold N, N^2 and their Montgomery
 * constants; private sets are built from (p, q) and additionally hold p^2, q^2, h_p, h_q and the CRT
 * constants — all computed ON THE GPU at creation (the reference recomputes them in every
 * Paillier::decrypt call; reuse is output-identical).
 *  d_N: [nkeys][64]   d_p, d_q: [nkeys][32]  (1024-bit primes)
 * key_idx arguments: per-item key index, or NULL meaning (nkeys==1 ? 0 : i). */
typedef struct mpe_paillier mpe_paillier;
int mpe_paillier_create_public(mpe_ctx* ctx, int nkeys, const uint32_t* d_N, mpe_paillier** out, void* stream);
int mpe_paillier_create_private(mpe_ctx* ctx, int nkeys, const uint32_t* d_p, const uint32_t* d_q,
                                mpe_paillier** out, void* stream);
int mpe_paillier_destroy(mpe_paillier* pk);
int mpe_paillier_nkeys(const mpe_paillier* pk);
/* device pointer to the [nkeys][64] table of moduli N (valid for the life of the key set) */
const uint32_t* mpe_paillier_n(const mpe_paillier* pk);

/* c = (1 + m*N) * r^N mod N^2     `Paillier::encrypt_with_chosen_randomness(ek, m, r)`
 * (src/utilities/mta/mod.rs:68-75,133-137).  m, r: [batch][64] (m < N);  c: [batch][128]. */
int mpe_paillier_encrypt(mpe_ctx* ctx, const mpe_paillier* pk, int batch, const int32_t* d_key_idx,
                         const uint32_t* d_m, const uint32_t* d_r, uint32_t* d_c, void* stream);
/* m = Dec(c), CRT form            `Paillier::decrypt(dk, c)` (src/utilities/mta/mod.rs:165,
 * src/protocols/multi_party_ecdsa/gg_2020/party_i.rs:455-457).  c: [batch][128] -> m: [batch][64].
 * Requires a private key set.  Ciphertexts must be units mod N (as the reference assumes). */
int mpe_paillier_decrypt(mpe_ctx* ctx, const mpe_paillier* sk, int batch, const int32_t* d_key_idx,
                         const uint32_t* d_c, uint32_t* d_m, void* stream);
/* c1*c2 mod N^2                   `Paillier::add` (src/utilities/mta/mod.rs:145) */
/* kzen-paillier `Open::open(dk, c)` (blame.rs:252-256, `extract_paillier_randomness`): m = Dec(c) and the r with
 * c = (1 + m N) r^N mod N^2, i.e. r = (c mod N)^(N^-1 mod phi(N)) mod N.  d_m, d_r [batch][64]. */
int mpe_paillier_open(mpe_ctx* ctx, const mpe_paillier* sk, int batch, const int32_t* d_key_idx, const uint32_t* d_c,
                      uint32_t* d_m, uint32_t* d_r, void* stream);
int mpe_paillier_add(mpe_ctx* ctx, const mpe_paillier* pk, int batch, const int32_t* d_key_idx,
                     const uint32_t* d_c1, const uint32_t* d_c2, uint32_t* d_out, void* stream);
/* c^k mod N^2                     `Paillier::mul` (src/utilities/mta/mod.rs:140-144); k: [batch][k_words] */
int mpe_paillier_mul(mpe_ctx* ctx, const mpe_paillier* pk, int batch, const int32_t* d_key_idx,
                     const uint32_t* d_c, const uint32_t* d_k, int k_words, uint32_t* d_out, void* stream);

/* ---- BigInt::mod_inv ------------------------------------------------------------------------ */
/* out[i] = a[i]^-1 mod modulus[idx(i)], ok[i] = 0 when gcd != 1 (curv `BigInt::mod_inv` -> Option;
 * src/utilities/mta/range_proofs.rs:122,135,339,351,363; zk_pdl_with_slack/mod.rs:192).
 * a must be reduced (a < modulus). */
int mpe_modinv(mpe_ctx* ctx, const mpe_modset* ms, int batch, const int32_t* d_mod_idx, const uint32_t* d_a,
               uint32_t* d_out, uint8_t* d_ok, void* stream);

/* ---- secp256k1 (curv Point<Secp256k1> / Scalar<Secp256k1>) -------------------------------------- */
/* Points: 16 words, affine x[8] | y[8], all-zero = point at infinity.  Scalars: k_words little-endian
 * words, reduced mod q on entry exactly like `Scalar::from(&BigInt)` (k_words <= 89).
 * out = k*G (`Point::generator() * k`), out = k*P (`P * k`), out = P + Q. */
int mpe_ec_mul_base(mpe_ctx* ctx, int batch, const uint32_t* d_k, int k_words, uint32_t* d_out, void* stream);
int mpe_ec_mul(mpe_ctx* ctx, int batch, const uint32_t* d_k, int k_words, const uint32_t* d_P, uint32_t* d_out,
               void* stream);
int mpe_ec_add(mpe_ctx* ctx, int batch, const uint32_t* d_P, const uint32_t* d_Q, uint32_t* d_out, void* stream);

/* curv `DLogProof::prove(sk)` with the nonce as input / `DLogProof::verify`
 * (src/utilities/mta/mod.rs:147-148,170-171).  pk, R: points; z: 8 words. */
int mpe_dlog_prove(mpe_ctx* ctx, int batch, const uint32_t* d_sk, const uint32_t* d_nonce, uint32_t* d_pk,
                   uint32_t* d_R, uint32_t* d_z, void* stream);
int mpe_dlog_verify(mpe_ctx* ctx, int batch, const uint32_t* d_pk, const uint32_t* d_R, const uint32_t* d_z,
                    uint8_t* d_ok, void* stream);

/* ---- DLogStatement tables and the range / PDL proofs -------------------------------------------- */
/* `zk_paillier::DLogStatement{N, g, ni}` as GG20 stores (N~, h1, h2)
 * (src/protocols/multi_party_ecdsa/gg_2020/party_i.rs:225-229).  d_Nt, d_h1, d_h2: [count][64]. */
typedef struct mpe_statements mpe_statements;
int mpe_statements_create(mpe_ctx* ctx, int count, const uint32_t* d_Nt, const uint32_t* d_h1,
                          const uint32_t* d_h2, mpe_statements** out, void* stream);
/* the same with an explicit window width (bits, 2..16) of the fixed-base tables of h1, h2: 2 * count tables of
 * ceil(2848 / wb) * 2^wb rows of 288 bytes (mpe_statements_create uses 13: 0.5 GB per base); wb = 0: no tables
 * (statements used once, e.g. the fresh (N~, h1, h2) of a Lindell'17 key generation) */
int mpe_statements_create_wb(mpe_ctx* ctx, int count, const uint32_t* d_Nt, const uint32_t* d_h1, const uint32_t* d_h2,
                             int wb, mpe_statements** out, void* stream);
int mpe_statements_destroy(mpe_statements* s);

/* Field widths (words): z,s 64 | e 8 | s1 25 (< 2^769) | s2,s3 89 (< 2^2817) | u2 128 | points 16.
 * Nonces (the reference samples them inside the call; here they are inputs):
 * alpha 24 (< q^3) | beta 64 | gamma 88 (< q^3 N~) | rho 72 (< q N~). */
typedef struct { uint32_t *z, *e, *s, *s1, *s2; } mpe_alice_proof;
typedef struct { const uint32_t *alpha, *beta, *gamma, *rho; } mpe_alice_nonces;
/* `AliceProof::generate(a, cipher, alice_ek, dlog_statement, r)`  (src/utilities/mta/range_proofs.rs:160-193)
 * a: [batch][8], cipher: [batch][128], r: [batch][64] (the Paillier randomness of cipher). */
int mpe_alice_generate(mpe_ctx* ctx, const mpe_paillier* pk, const mpe_statements* stm, int batch,
                       const int32_t* d_key_idx, const int32_t* d_st_idx, const uint32_t* d_a,
                       const uint32_t* d_cipher, const uint32_t* d_r, const mpe_alice_nonces* nonces,
                       const mpe_alice_proof* out, void* stream);
/* `AliceProof::verify(cipher, alice_ek, dlog_statement) -> bool`  (range_proofs.rs:105-156) */
int mpe_alice_verify(mpe_ctx* ctx, const mpe_paillier* pk, const mpe_statements* stm, int batch,
                     const int32_t* d_key_idx, const int32_t* d_st_idx, const uint32_t* d_cipher,
                     const mpe_alice_proof* proof, uint8_t* d_ok, void* stream);

typedef struct { uint32_t *z, *u1, *u2, *u3, *s1, *s2, *s3; } mpe_pdl_proof;
typedef struct { const uint32_t *alpha, *beta, *rho, *gamma; } mpe_pdl_nonces;
/* `PDLwSlackProof::prove(witness{x, r}, statement{ciphertext, ek, Q, G, h1, h2, N_tilde})`
 * (src/utilities/zk_pdl_with_slack/mod.rs:68-125).  Q, G: points; x: [batch][8]; r: [batch][64]. */
int mpe_pdl_prove(mpe_ctx* ctx, const mpe_paillier* pk, const mpe_statements* stm, int batch,
                  const int32_t* d_key_idx, const int32_t* d_st_idx, const uint32_t* d_cipher,
                  const uint32_t* d_Q, const uint32_t* d_G, const uint32_t* d_x, const uint32_t* d_r,
                  const mpe_pdl_nonces* nonces, const mpe_pdl_proof* out, void* stream);
/* `PDLwSlackProof::verify(statement) -> Result<(), ZkPdlWithSlackError>`  (mod.rs:127-179); ok[i]=1 accepts.
 * (Where the reference would panic on a non-invertible c or z, the item is rejected instead.) */
int mpe_pdl_verify(mpe_ctx* ctx, const mpe_paillier* pk, const mpe_statements* stm, int batch,
                   const int32_t* d_key_idx, const int32_t* d_st_idx, const uint32_t* d_cipher,
                   const uint32_t* d_Q, const uint32_t* d_G, const mpe_pdl_proof* proof, uint8_t* d_ok,
                   void* stream);

/* ---- MtA share conversion (src/utilities/mta/mod.rs) ---------------------------------------------------- */
/* `dlog_statements` = all statements of `stm` (rounds.rs:87,154 pass the whole h1_h2_n_tilde_vec); per-exchange
 * arrays of range proofs / nonces are item-major [batch][count_statements]. */
typedef struct { uint32_t *pk, *R, *z; } mpe_dlog_proof;     /* DLogProof{pk, pk_t_rand_commitment, challenge_response} */
/* `MessageA::a_with_predefined_randomness(a, alice_ek, randomness, dlog_statements)`  (:62-87)
 * a [batch][8], r [batch][64] -> c [batch][128] + one AliceProof per statement. */
int mpe_mta_message_a(mpe_ctx* ctx, const mpe_paillier* pk, const mpe_statements* stm, int batch,
                      const int32_t* d_key_idx, const uint32_t* d_a, const uint32_t* d_r,
                      const mpe_alice_nonces* nonces, uint32_t* d_c, const mpe_alice_proof* proofs, void* stream);
/* `MessageB::b_with_predefined_randomness(b, alice_ek, m_a, randomness, beta_tag, dlog_statements)`  (:111-158)
 * key_idx selects ALICE's key.  ok[i] = 0 is the reference's Err(InvalidKey) (a range proof failed); the
 * outputs of such an item are still written.  beta = -beta_tag mod q [batch][8]. */
int mpe_mta_message_b(mpe_ctx* ctx, const mpe_paillier* pk, const mpe_statements* stm, int batch,
                      const int32_t* d_key_idx, const uint32_t* d_b, const uint32_t* d_ca,
                      const mpe_alice_proof* range_proofs, const uint32_t* d_r, const uint32_t* d_beta_tag,
                      const uint32_t* d_nonce_b, const uint32_t* d_nonce_bt, uint32_t* d_cb, uint32_t* d_beta,
                      const mpe_dlog_proof* b_proof, const mpe_dlog_proof* beta_tag_proof, uint8_t* d_ok, void* stream);
/* `MessageB::verify_proofs_get_alpha(dk, a)`  (:160-179): alpha [batch][8] = Dec(c_b) mod q, alice_share [batch][64]
 * the full plaintext; ok[i] = 0 is Err(InvalidKey). */
int mpe_mta_verify_get_alpha(mpe_ctx* ctx, const mpe_paillier* sk, int batch, const int32_t* d_key_idx,
                             const uint32_t* d_cb, const mpe_dlog_proof* b_proof, const mpe_dlog_proof* beta_tag_proof,
                             const uint32_t* d_a, uint32_t* d_alpha, uint32_t* d_alice_share, uint8_t* d_ok, void* stream);

/* Bob's MtA(wc) range proof: `BobProof::generate` / `BobProof::verify` / `BobProofExt::verify`
 * (src/utilities/mta/range_proofs.rs:218-534).  Widths (words): t,z,s 64 | e 8 | s1 25 | s2,t2 89 | t1 81 (< 2^2561).
 * Nonces: alpha 24 (< q^3) | beta 64 | gamma 80 (< q^2 N) | rho, sigma 72 (< q N~) | rho_prim, tau 88 (< q^3 N~).
 * generate: a_enc, mta_enc [batch][128]; b [batch][8]; beta_prim, r [batch][64]; check != 0 also writes
 * u = alpha*G to d_u [batch][16] and hashes X = b*G, u (the `check` flag of :414-424).
 * verify: d_X, d_u both NULL -> BobProof::verify(.., None); both set -> BobProofExt::verify. */
typedef struct { uint32_t *t, *z, *e, *s, *s1, *s2, *t1, *t2; } mpe_bob_proof;
typedef struct { const uint32_t *alpha, *beta, *gamma, *rho, *rho_prim, *sigma, *tau; } mpe_bob_nonces;
int mpe_bob_generate(mpe_ctx* ctx, const mpe_paillier* pk, const mpe_statements* stm, int batch,
                     const int32_t* d_key_idx, const int32_t* d_st_idx, const uint32_t* d_a_enc,
                     const uint32_t* d_mta_enc, const uint32_t* d_b, const uint32_t* d_beta_prim, const uint32_t* d_r,
                     const mpe_bob_nonces* nonces, int check, const mpe_bob_proof* out, uint32_t* d_u, void* stream);
int mpe_bob_verify(mpe_ctx* ctx, const mpe_paillier* pk, const mpe_statements* stm, int batch,
                   const int32_t* d_key_idx, const int32_t* d_st_idx, const uint32_t* d_a_enc,
                   const uint32_t* d_mta_enc, const mpe_bob_proof* proof, const uint32_t* d_X, const uint32_t* d_u,
                   uint8_t* d_ok, void* stream);

/* ---- curv sigma proofs of GG20 phases 3 / 6 and the phase-1 hash commitment (curv-kzen 0.9, un-vendored) ------ */
/* `PedersenProof::prove(m, r)` with the nonces s1, s2 as inputs (src/protocols/multi_party_ecdsa/gg_2020/party_i.rs:620-634):
 * com = m G + r H (H = `Point::base_point2()`), a1 = s1 G, a2 = s2 H, e = H(G, H, com, a1, a2), z1 = s1 + e m, z2 = s2 + e r.
 * Points 16 words, scalars 8.  `PedersenProof::verify` (state_machine/sign/rounds.rs:371-378) recomputes e. */
typedef struct { uint32_t *com, *e, *a1, *a2, *z1, *z2; } mpe_pedersen_proof;
int mpe_pedersen_prove(mpe_ctx* ctx, int batch, const uint32_t* d_m, const uint32_t* d_r, const uint32_t* d_s1,
                       const uint32_t* d_s2, const mpe_pedersen_proof* out, void* stream);
int mpe_pedersen_verify(mpe_ctx* ctx, int batch, const mpe_pedersen_proof* proof, uint8_t* d_ok, void* stream);
/* `HomoELGamalProof::prove(witness{x, r}, statement{G, H, Y, D, E})` / `verify` (party_i.rs:778-833): T = s1 H + s2 Y,
 * A3 = s2 G, e = H(T, A3, G, H, Y, D, E), z1 = s1 + e x (s1 when x = 0), z2 = s2 + e r;
 * verify: z1 H + z2 Y == T + e D and z2 G == A3 + e E.  Every point per item, [batch][16]. */
typedef struct { const uint32_t *G, *H, *Y, *D, *E; } mpe_heg_statement;
typedef struct { uint32_t *T, *A3, *z1, *z2; } mpe_heg_proof;
int mpe_heg_prove(mpe_ctx* ctx, int batch, const uint32_t* d_x, const uint32_t* d_r, const uint32_t* d_s1, const uint32_t* d_s2,
                  const mpe_heg_statement* statement, const mpe_heg_proof* out, void* stream);
int mpe_heg_verify(mpe_ctx* ctx, int batch, const mpe_heg_statement* statement, const mpe_heg_proof* proof, uint8_t* d_ok,
                   void* stream);
/* `HashCommitment::create_commitment_with_user_defined_randomness(BigInt::from_bytes(P.to_bytes(true)), blind)`
 * (party_i.rs:577-580,654-659): com [batch][8] = SHA-256(33 bytes of P || minimal bytes of blind). */
int mpe_hash_commit_point(mpe_ctx* ctx, int batch, const uint32_t* d_P, const uint32_t* d_blind, uint32_t* d_com, void* stream);

/* ---- GG20 signing ------------------------------------------------------------------------------------------------ */
/* Key material as the reference's keygen leaves it in `LocalKey` (state_machine/keygen/rounds.rs:311-322), for
 * `nkeysets` wallets of the same (t, n) shape (a batch may mix wallets: every session names its key set).
 * PUBLIC part, all n parties:  d_N [K][n][64] `paillier_key_vec`, d_Nt/d_h1/d_h2 [K][n][64] `h1_h2_n_tilde_vec`,
 * d_y [K][16] `y_sum_s`, d_X [K][n][16] `pk_vec`.
 * SECRET part, only of the n_own parties h_own[] (ascending party indices) this process acts for:
 * d_x [K][n_own][8] `keys_linear.x_i`, d_p / d_q [K][n_own][32] `paillier_dk`.  One party per process is the
 * reference's deployment; all of them in one object is its `Simulation` test harness (state_machine/sign.rs:667-763).
 * h_signers (HOST array): n_signers ascending party indices (`s_l` minus one, sign.rs:78), t < n_signers <= n.
 * The window width of the fixed-base tables of h1, h2 is chosen from the table memory 2 K n bases need
 * (13 bits = 0.5 GB per base when that fits a quarter of the free HBM, narrower for many wallets). */
typedef struct mpe_gg20_keys mpe_gg20_keys;
int mpe_gg20_keys_create(mpe_ctx* ctx, int t, int n, int n_signers, const int32_t* h_signers, int nkeysets, int n_own,
                         const int32_t* h_own, const uint32_t* d_x, const uint32_t* d_p, const uint32_t* d_q,
                         const uint32_t* d_N, const uint32_t* d_Nt, const uint32_t* d_h1, const uint32_t* d_h2,
                         const uint32_t* d_y, const uint32_t* d_X, mpe_gg20_keys** out, void* stream);
/* The same with SEVERAL signer sets, so that one key object (one set of fixed-base tables, Paillier objects and sampling bounds) signs
 * for any quorum of the wallet: h_sets [n_sets][n_signers] (HOST), every row ascending distinct party indices < n, 1 <= n_sets <= 256,
 * two equal rows are MPE_E_ARG.  Every session of a batch then names its set through d_sigset (the *_sets calls below); set 0 is what
 * h_signers is above: mpe_gg20_keys_create is the n_sets == 1 case, and every entry point that takes no per-session set means set 0.
 * n_signers is one value per key object. */
int mpe_gg20_keys_create_sets(mpe_ctx* ctx, int t, int n, int n_signers, int n_sets, const int32_t* h_sets, int nkeysets, int n_own,
                              const int32_t* h_own, const uint32_t* d_x, const uint32_t* d_p, const uint32_t* d_q,
                              const uint32_t* d_N, const uint32_t* d_Nt, const uint32_t* d_h1, const uint32_t* d_h2,
                              const uint32_t* d_y, const uint32_t* d_X, mpe_gg20_keys** out, void* stream);
int mpe_gg20_keys_destroy(mpe_gg20_keys* keys);
int mpe_gg20_keys_fb_window_bits(const mpe_gg20_keys* keys);

/* Everything the reference samples while signing, as inputs.  L = the local parties of a session object (their
 * nonces only), S = signers.  Leading dimensions [B][L]; then statement st (n); peer slot jj (S-1; the peer's signer
 * ordinal is ind = jj < i ? jj : jj+1, the `ind` of rounds.rs:149); MessageB variant v (0: gamma_i, 1: w_i).
 *   k, gamma, blind, l, ped_s1, ped_s2, heg_s1, heg_s2 : [B][L][8]      r_a : [B][L][64]
 *   al_alpha [B][L][n][24]  al_beta [..][64]  al_gamma [..][88]  al_rho [..][72]       (AliceProof nonces)
 *   mb_beta_tag, mb_r : [B][L][S-1][2][64]   mb_nonce_b, mb_nonce_bt : [B][L][S-1][2][8] (MessageB::b)
 *   pdl_alpha [B][L][S-1][24]  pdl_beta [..][64]  pdl_rho [..][72]  pdl_gamma [..][88]   (PDLwSlackProof::prove)
 *   msg : [B][8]  the message as BigInt (reduced mod q like `Scalar::from(message)`, party_i.rs:857); read by
 *         mpe_gg20_sign only (the round view takes the message in round 7). */
typedef struct {
  const uint32_t *k, *gamma, *blind, *r_a;
  const uint32_t *al_alpha, *al_beta, *al_gamma, *al_rho;
  const uint32_t *mb_beta_tag, *mb_r, *mb_nonce_b, *mb_nonce_bt;
  const uint32_t *l, *ped_s1, *ped_s2;
  const uint32_t *pdl_alpha, *pdl_beta, *pdl_rho, *pdl_gamma;
  const uint32_t *heg_s1, *heg_s2;
  const uint32_t *msg;
} mpe_gg20_nonces;

/* ---- the SAMPLING side of the trait surface ------------------------------------------------------------------------
 * curv `Samplable::{sample, sample_below, sample_range}`, the reference's `SampleFromMultiplicativeGroup::from_modulo`
 * (src/utilities/mta/range_proofs.rs:538-557) and `Scalar::<Secp256k1>::random()`, drawn ON THE DEVICE from a 32-byte seed.
 * Item g of stream `stream_id` reads the ChaCha20 keystream (RFC 8439 block function) with key = seed, state[12] = block
 * counter from 0, state[13] = g, state[14] | state[15] << 32 = stream_id, taking its bytes in order; the byte -> integer
 * rules are curv's (recalled): sample(bits) = from_bytes_be(ceil(bits/8) bytes) >> (8 ceil(bits/8) - bits);
 * sample_below(u) = repeat sample(bit_length(u)) until < u (every attempt takes fresh bytes).
 * A (seed, stream_id) pair must never be used twice.  h_seed32: HOST pointer to 32 bytes.
 * (The sealed records below have the same kind of contract: a (wrapping key, nonce_hi) pair must never be used twice.)
 *   mpe_sample_bits    d_out [batch][out_words] = BigInt::sample(bits)
 *   mpe_sample_below   d_out = sample_below(bound row d_bound_idx[i] of d_bound [nbounds][bound_words]; NULL index: row 0 when
 *                      nbounds == 1, else row i); flags: MPE_SAMPLE_NONZERO rejects 0, MPE_SAMPLE_PLUS_ONE returns 1 + the draw
 *                      (sample_range(1, bound + 1)), MPE_SAMPLE_COPRIME = from_modulo: also repeat until gcd(x, bound) == 1
 *                      (odd bounds of at most 2048 bits; an even bound counts as a failure)
 *   mpe_sample_scalar  d_out [batch][8] = Scalar::random(): 32 bytes as a big-endian integer until 0 < x < q
 * d_fail (may be NULL): incremented for every item that exhausted 128 attempts (probability < 2^-128; its row is zero). */
#define MPE_SAMPLE_NONZERO 1
#define MPE_SAMPLE_PLUS_ONE 2
#define MPE_SAMPLE_COPRIME 4
int mpe_sample_bits(mpe_ctx* ctx, int batch, const uint8_t* h_seed32, uint64_t stream_id, int bits, int out_words, uint32_t* d_out,
                    void* stream);
int mpe_sample_below(mpe_ctx* ctx, int batch, const uint8_t* h_seed32, uint64_t stream_id, const uint32_t* d_bound, int bound_words,
                     int nbounds, const int32_t* d_bound_idx, int flags, int out_words, uint32_t* d_out, int32_t* d_fail, void* stream);
int mpe_sample_scalar(mpe_ctx* ctx, int batch, const uint8_t* h_seed32, uint64_t stream_id, uint32_t* d_out, int32_t* d_fail,
                      void* stream);
/* Everything a batch of signing sessions draws from OsRng, with the reference's distributions, into the arrays of `out`
 * (all fields but msg; the layout of mpe_gg20_nonces for `n_local` local parties h_local[]):
 *   k, gamma, l, ped_s*, heg_s*, mb_nonce_*: Scalar::random() (party_i.rs:561-563,628; curv's sigma proofs; mta/mod.rs:147-148)
 *   blind: BigInt::sample(256) (party_i.rs:574)     r_a: sample_below(N_i) (mta/mod.rs:57)
 *   al_alpha < q^3, al_beta = from_modulo(N_i), al_gamma < q^3 N~_st, al_rho < q N~_st   (range_proofs.rs:48-51)
 *   mb_beta_tag, mb_r < N_peer (mta/mod.rs:97-98)
 *   pdl_alpha < q^3, pdl_beta = sample_range(1, N_i - 1), pdl_rho < q N~_peer, pdl_gamma < q^3 N~_peer (zk_pdl_with_slack/mod.rs:73-77)
 * field f (its position in mpe_gg20_nonces, k = 0) of batch `batch_counter` (< 2^56) uses stream_id = batch_counter | f << 56 and
 * item index = the field's row index.  from_modulo's gcd runs as ONE batched verdict (Montgomery's trick) and only failing
 * items are redrawn lane by lane — the values equal those of the literal loop.  A (seed, batch_counter) pair signs ONE batch.
 * mpe_gg20_nonces_alloc / _view / _free: one device allocation holding every field for (batch, n_local), zeroed when freed. */
typedef struct mpe_gg20_nonce_buf mpe_gg20_nonce_buf;
int mpe_gg20_nonces_alloc(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, int n_local, mpe_gg20_nonce_buf** out);
int mpe_gg20_nonces_view(const mpe_gg20_nonce_buf* buf, mpe_gg20_nonces* out);
int mpe_gg20_nonces_free(mpe_gg20_nonce_buf* buf);
int mpe_gg20_sample_nonces(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, int n_local, const int32_t* h_local,
                           const int32_t* d_keyset, const uint8_t* h_seed32, uint64_t batch_counter, const mpe_gg20_nonces* out,
                           int32_t* d_fail, void* stream);
/* ... for sessions that name their signer set (d_sigset [batch], device; local_by_party as for mpe_gg20_session_create_sets).  Stream
 * ids and item indices are those of mpe_gg20_sample_nonces; only the bound row an item reads follows the session's set: row b equals
 * row b of the uniform call on a key object whose signer set is that session's, under the same (seed, batch_counter). */
int mpe_gg20_sample_nonces_sets(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, int n_local, const int32_t* h_local,
                                const int32_t* d_keyset, const int32_t* d_sigset, int local_by_party, const uint8_t* h_seed32,
                                uint64_t batch_counter, const mpe_gg20_nonces* out, int32_t* d_fail, void* stream);

/* GG20 round messages.  One fixed-size record of 32-bit words per (sender, session); a slab holds, for every sender,
 * a [B][W] block of records.  P2P messages travel like broadcast ones and are filtered by the receiver, exactly as the
 * reference's relay does (examples/gg20_sm_client.rs:35-40).  Points: x[8] | y[8]; all other fields little-endian words.
 *   round 0  (MessageA, SignBroadcastPhase1)       W = 256 (n+1): sub-record st < n = AliceProof for statement st
 *                                                   {z 0, e 64, s 72, s1 136, s2 161}; sub-record n = {c 0, com 128}
 *   round 1  (GammaI, WI) to every peer            W = 208 * 2 (S-1): sub-record 2 jj + v = MessageB for peer slot jj
 *                                                   {c 0, b_proof {pk 128, R 144, z 160}, beta_tag_proof {pk 168, R 184, z 200}}
 *   round 2  (DeltaI, TI, TIProof)                 W = 96: {delta 0, T 8, proof {e 24, a1 32, a2 48, com 64, z1 80, z2 88}}
 *   round 3  SignDecommitPhase1                    W = 24: {blind_factor 0, g_gamma_i 8}
 *   round 4  (RDash, Vec<PDLwSlackProof>)          W = 450 S: sub-record jj < S-1 = the proof for peer slot jj
 *                                                   {z 0, u1 64, u2 80, u3 208, s1 272, s2 297, s3 361}; sub-record S-1 = {R_dash 0}
 *   round 5  (SI, HEGProof)                        W = 64: {S_i 0, T 16, A3 32, z1 48, z2 56}
 *   round 7  PartialSignature                      W = 8:  {s_i}
 * mpe_gg20_msg_words returns W (0 for rounds that emit nothing). */
int mpe_gg20_msg_words(int n_signers, int n, int round);

/* The per-party ROUND VIEW: `RoundN::proceed` (state_machine/sign/rounds.rs:68,122,234,347,431,525,612,672) batched over
 * `batch` sessions and over the n_local parties h_local[] (ascending signer ORDINALS, positions in s_l) this object acts
 * for; their secrets must be in `keys`.  d_keyset [batch]: key set of every session (NULL when nkeysets == 1).
 * `nonces`: the local parties' sampled values (layout above); the arrays must stay valid until round 5 is queued.
 * dedup_verify = 0: faithful work (each range proof verified for both MessageB::b calls, every local party verifies
 * every PDL proof, rounds.rs:151-175,546-558); 1: identical checks are evaluated once (same results).
 *
 * mpe_gg20_roundN(sess, d_in, h_in_off, d_out): d_in = the previous round's records of ALL S senders ("including me"):
 * sender ordinal j's [batch][W] block starts at record h_in_off[j] of d_in (HOST array; NULL = j*batch); d_out = this
 * object's outgoing records [n_local][batch][W].  Round 6 emits nothing; round 7 takes the messages to sign
 * (d_msg [batch][8]) and emits the partial signatures; mpe_gg20_complete = `SignManual::complete` (sign.rs:625-646).
 * Rounds must be called in order.  A failing check never aborts the batch: the party's status in that session becomes
 * 100*round + detail of its FIRST failed check, in the order the reference evaluates them, and sticks:
 *   101 MessageB::b -> InvalidKey (Error::Round1) | 201 verify_proofs_get_alpha | 202 b_proof.pk != g_w_vec[ind] (rounds.rs:281)
 *   303 T_i != proof.com (rounds.rs:366) | 301 delta not invertible | 302 PedersenProof::verify
 *   401 phase4 "bad gamma_i decommit" | 501 "Bad PDLwSlack proof" | 502 phase5_check_R_dash_sum
 *   601 phase6_verify_proof | 602 phase6_check_S_i_sum | 701 output_signature: verify failed
 *   91 (MPE_GG20_STATUS_BAD_NONCE, round 0) k_i or gamma_i is not a value `Scalar::random()` returns (0 < x < q): the device sampler
 *      marks the party of a session one of whose rejection loops gave up this way (mpe_gg20_sample_nonces: after
 *      sampler_max_attempts candidates, default 128 — probability < 2^-128 per draw; curv's loops are unbounded, a deliberate
 *      divergence) so that a session NEVER signs on zeroed values; a caller's own out-of-range k_i / gamma_i is refused alike
 *   92 (MPE_GG20_STATUS_BAD_SET, round 0) the session names no quorum this party signs in: d_sigset[b] is outside [0, n_sets), or the
 *      local party given by index is not a member of the session's set.  Checked on the device (the host never reads d_sigset); the
 *      party emits zero records and never signs
 *   93 (MPE_GG20_STATUS_BAD_TWEAK, round 0) the session's tweak (mpe_gg20_session_create_tweaks) is not canonical (t >= q — the all-ones
 *      tweak of a failed mpe_bip32_derive row is), or the child key y + t G is the point at infinity; the party emits zero records and
 *      never signs, the other sessions of the batch are unaffected
 * with `bad_actors` (a bit mask over signer ordinals, the reference's `ErrorType::bad_actors`, gg_2020/mod.rs:23-27) set
 * for 401 (the peers whose decommitment is bad), 501 (the first failing prover) and 601 (every failing prover).
 * mpe_gg20_session_result: d_status, d_bad_actors, d_recid [n_local][batch]; d_r, d_s [n_local][batch][8] (after
 * mpe_gg20_complete; zero unless status == 0); d_R [n_local][batch][16] (after round 4).  Any pointer may be NULL.
 * Destroying a session zeroes its state (k_i, gamma_i, w_i, sigma_i, ...). */
#define MPE_GG20_STATUS_BAD_NONCE 91
#define MPE_GG20_STATUS_BAD_SET 92
#define MPE_GG20_STATUS_BAD_TWEAK ((int)93)
typedef struct mpe_gg20_session mpe_gg20_session;
int mpe_gg20_session_create(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, int n_local, const int32_t* h_local,
                            const int32_t* d_keyset, const mpe_gg20_nonces* nonces, int dedup_verify, mpe_gg20_session** out,
                            void* stream);
/* Sessions that name their signer set: d_sigset [batch] (device int32) = the set of `keys` (mpe_gg20_keys_create_sets) session b signs
 * with; NULL = set 0 for all, which computes exactly what mpe_gg20_session_create computes.  Signer ORDINALS — senders of a slab, peer
 * slots, bad_actors bits, fault-injection masks — are positions in the session's OWN set.  The local parties come in two forms:
 *   local_by_party = 0  h_local[] are ordinals, as above: local slot l is the party at position h_local[l] of each session's set, so
 *                       `keys` must hold the secrets of every party that can stand there in ANY of its sets (checked here, MPE_E_ARG);
 *   local_by_party = 1  n_local = 1 and h_local[0] is a PARTY INDEX whose secrets `keys` holds (one party per process, the reference's
 *                       deployment): its ordinal in session b is its rank in set d_sigset[b].  The incoming slabs stay
 *                       [sender ordinal][batch][W], ordinals taken in each session's own set; routing records is the relay's job.
 * A session whose d_sigset[b] is out of range, or whose by-index party is not in its set, gets MPE_GG20_STATUS_BAD_SET.
 * d_sigset, like d_keyset, must stay valid until the batch is completed, deposited or given up (the rounds read it). */
int mpe_gg20_session_create_sets(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, int n_local, const int32_t* h_local,
                                 const int32_t* d_keyset, const int32_t* d_sigset, int local_by_party, const mpe_gg20_nonces* nonces,
                                 int dedup_verify, mpe_gg20_session** out, void* stream);
/* Sessions that sign for CHILD KEYS of their key set (non-hardened BIP32 derivation, mpe_bip32_derive): d_tweak [batch][8] (device,
 * little-endian words, PUBLIC) = the tweak t_b of session b; the session signs for x + t_b, public key y + t_b G.  Adding t to every
 * Shamir share moves the polynomial's constant term by t and nothing else, so x_i' = x_i + t, X_i' = X_i + t G, and of a signing
 * session only w_i = lambda_i (x_i + t), g_w_vec[j] = g_w[j] + (lambda_j t) G and y change: Paillier keys, N~ statements, sampler bounds
 * and every ladder stay.  The session copies the tweaks and owns two tables, y_b [batch][16] and g_w_b [batch][S][16], filled by one
 * kernel here and at every re-arm ((S + 1) comb multiplications per session); d_tweak need not outlive the call.  NULL = no tweak:
 * exactly mpe_gg20_session_create_sets, no table, the same launches.  A tweak that is not canonical, or whose child key is the point
 * at infinity, stops the session's parties at round 0 with MPE_GG20_STATUS_BAD_TWEAK.  The tweak is bound at round 0 (sigma_i contains
 * w_i'): a presignature made here belongs to its child key.
 * NOT supported for a session with tweaks, each MPE_E_ARG with a mpe_last_error text: mpe_gg20_presig_deposit (the record keeps its
 * layout; MPE_GG20_PRESIG_RECORD_VERSION stays 1) and mpe_gg20_session_blame6_state (the blame entry points take a key object and know
 * no tweak).  The pipelined engines, mpe_gg20_presign_sets and the sharded exchange have no form that takes tweaks. */
int mpe_gg20_session_create_tweaks(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, int n_local, const int32_t* h_local,
                                   const int32_t* d_keyset, const int32_t* d_sigset, int local_by_party, const uint32_t* d_tweak,
                                   const mpe_gg20_nonces* nonces, int dedup_verify, mpe_gg20_session** out, void* stream);
/* d_y [batch][16]: the public key every session of the running batch signs for — its child key (zero where the tweak was refused), or
 * its key set's y in a batch without tweaks. */
int mpe_gg20_session_child_keys(const mpe_gg20_session* sess, uint32_t* d_y, void* stream);
int mpe_gg20_session_destroy(mpe_gg20_session* sess, void* stream);
/* The next batch of the same shape on the same object (a party process signs batch after batch: `SignManual::new` again
 * with fresh `SignKeys`, sign.rs:540-569): new sampled values (and key-set choice), state of the previous batch zeroed, rounds
 * start again at 0.  Results are identical to those of a freshly created session.
 * `nonces` MUST hold freshly sampled values (the same buffers refilled are fine): signing two batches with the same k_i,
 * gamma_i or Paillier randomness leaks the key share, and the library cannot detect it.  MPE_E_ARG when the previous batch is
 * half-way through the protocol and healthy (finish it with mpe_gg20_complete, or give it up with mpe_gg20_session_abort);
 * MPE_E_HIP when the wipe fails. */
int mpe_gg20_session_rearm(mpe_gg20_session* sess, const int32_t* d_keyset, const mpe_gg20_nonces* nonces, void* stream);
/* ... with the next batch's signer sets, for a session made by mpe_gg20_session_create_sets with a d_sigset (MPE_E_ARG otherwise: the
 * local parties' secrets were then checked against set 0 alone).  NULL = set 0 for all; mpe_gg20_session_rearm is that case. */
int mpe_gg20_session_rearm_sets(mpe_gg20_session* sess, const int32_t* d_keyset, const int32_t* d_sigset, const mpe_gg20_nonces* nonces,
                                void* stream);
/* ... with the next batch's tweaks, for a session made by mpe_gg20_session_create_tweaks with a d_tweak (MPE_E_ARG otherwise: the
 * session owns no tables).  NULL = no tweak for the next batch; mpe_gg20_session_rearm_sets is that case. */
int mpe_gg20_session_rearm_tweaks(mpe_gg20_session* sess, const int32_t* d_keyset, const int32_t* d_sigset, const uint32_t* d_tweak,
                                  const mpe_gg20_nonces* nonces, void* stream);
/* Gives the running batch up (a peer vanished, a round call returned an error): the
 * nonce-derived state is wiped at once, every round entry point refuses, and mpe_gg20_session_rearm starts the next batch.  (A caller
 * that stops after the offline stage to sign later does not abort: mpe_gg20_presig_deposit moves the presignatures into a pool.)  A
 * session whose round call FAILED (MPE_E_NOMEM, MPE_E_HIP) may also be re-armed directly: a long-lived party process is never
 * left with an object it can only destroy. */
int mpe_gg20_session_abort(mpe_gg20_session* sess, void* stream);
int mpe_gg20_round0(mpe_gg20_session* sess, uint32_t* d_out, void* stream);
int mpe_gg20_round1(mpe_gg20_session* sess, const uint32_t* d_in, const int64_t* h_in_off, uint32_t* d_out, void* stream);
int mpe_gg20_round2(mpe_gg20_session* sess, const uint32_t* d_in, const int64_t* h_in_off, uint32_t* d_out, void* stream);
int mpe_gg20_round3(mpe_gg20_session* sess, const uint32_t* d_in, const int64_t* h_in_off, uint32_t* d_out, void* stream);
int mpe_gg20_round4(mpe_gg20_session* sess, const uint32_t* d_in, const int64_t* h_in_off, uint32_t* d_out, void* stream);
int mpe_gg20_round5(mpe_gg20_session* sess, const uint32_t* d_in, const int64_t* h_in_off, uint32_t* d_out, void* stream);
int mpe_gg20_round6(mpe_gg20_session* sess, const uint32_t* d_in, const int64_t* h_in_off, void* stream);
int mpe_gg20_round7(mpe_gg20_session* sess, const uint32_t* d_msg, uint32_t* d_out, void* stream);
int mpe_gg20_complete(mpe_gg20_session* sess, const uint32_t* d_in, const int64_t* h_in_off, void* stream);
int mpe_gg20_session_result(const mpe_gg20_session* sess, int32_t* d_status, uint32_t* d_bad_actors, uint32_t* d_r,
                            uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, void* stream);

/* Fault injection of the reference's own tests (gg_2020/test.rs:282-289,458-465,679-686): the local parties whose signer
 * ordinal is in party_mask double their delta_i (step 5), sigma_i (step 6) or s_i (step 7).  step 0 switches it off. */
int mpe_gg20_session_fault_inject(mpe_gg20_session* sess, int step, uint32_t party_mask);

/* ---- the presignature pool: offline stages kept, signed online later ----------------------------------------------------
 * GG20's rounds 0-6 need no message.  `CompletedOfflineStage` (state_machine/sign/rounds.rs:647-661) is a value in the reference: it
 * leaves `OfflineStage::pick_output` and enters `SignManual::new` when the message arrives.  A pool keeps that value on the device, in
 * single-use SLOTS, for the n_local parties h_local[] (signer ordinals, as for mpe_gg20_session_create) of `keys`; one slot = one
 * session: per party k_i [8], sigma_i [8], R [16], per slot the key-set index and a state word.  The pool's memory is its own
 * allocation; _destroy zeroes it first (and waits for the device: calls on any stream may still use the slots).
 *
 *   EMPTY --deposit / import--> READY --sign--> SIGNED --complete--> EMPTY        READY --export--> EMPTY       any --discard--> EMPTY
 *
 * Every transition is ONE device-scope compare-and-swap on the slot's state word, taken before any secret of the slot is read; a row
 * that loses it touches nothing and reports a status.  However calls, streams and duplicate slot indices interleave, at most one
 * partial signature is ever computed from one k_i.  (A slot is BUSY only while the winning row of a running call works on it.)
 * Which slots are free is the caller's policy: every call takes the slot indices d_slot [count] it is to use.  Row statuses (0 = done):
 *   801 deposit: slot out of range | 802 deposit: slot not EMPTY | 803 deposit: the session had failed in that row (a local party's
 *       status is non-zero; it stays readable through mpe_gg20_session_result)
 *   811 sign: slot out of range | 812 sign: slot not READY (empty, already signed, or claimed by another row or another call)
 *   821 complete: slot out of range | 822 complete: slot not SIGNED | 701 output_signature: verify failed (party_i.rs:873-936, as
 *       mpe_gg20_complete reports it)
 *   831 export / import: slot out of range | 832 import: record refused | 833 export: slot not READY | 834 import: slot not EMPTY
 * Every d_status may be NULL.
 *
 * mpe_gg20_presig_deposit   sess must be behind round 6 (the next call would be mpe_gg20_round7) with the pool's keys and local
 *     parties, else MPE_E_ARG and nothing is touched.  Row b of the session goes to slot d_slot[b] ([batch]) when every local party's
 *     status in it is 0 and the slot is EMPTY.  In EVERY case the session's nonce-derived state is then wiped as
 *     mpe_gg20_session_abort wipes it and the rounds refuse until mpe_gg20_session_rearm: the only live copy of k_i is the pool's.
 * mpe_gg20_presig_sign      `Round7::new` / phase7_local_sig (party_i.rs:850-871) for READY slots: d_msg [count][8] as
 *     mpe_gg20_round7 takes it, d_s_i [n_local][count][8] = m k_i + r sigma_i (zero rows unless status 0).  The slot keeps m, r and its
 *     own s_i for the completion; k_i and sigma_i are zeroed by the same kernel.  Among duplicate indices exactly one row wins.
 * mpe_gg20_presig_complete  `SignManual::complete` (sign.rs:625-646; output_signature + verify) for SIGNED slots: d_in = the partial
 *     signatures of all S senders including the own, sender j's [count][8] block at record h_in_off[j] (HOST array; NULL = j * count);
 *     d_r, d_s [n_local][count][8], d_recid, d_status [n_local][count]: low-s normalised with the recid flip, zero unless status 0.
 *     The slot returns to EMPTY whatever the verdict.
 * mpe_gg20_presig_export    moves READY slots out (READY -> EMPTY, secrets zeroed in the pool): the record is then the only copy.
 * mpe_gg20_presig_import    EMPTY -> READY.  Refused (832): a version, number of local parties or ordinals that are not the pool's; a
 *     signer-set mask that is none of the key object's sets (the slot remembers which one); a key-set index out of range or a y that is not that key set's; an R that is no valid curve point; a k_i outside
 *     (0, q) or a sigma_i outside [0, q).
 *     The RECORD, mpe_gg20_presig_record_words(pool) = 28 + 32 n_local little-endian 32-bit words:
 *       [0] MPE_GG20_PRESIG_RECORD_VERSION | [1] signer-set mask (bit = party index) | [2] n_local | [3..10] local ordinals (unused: 0)
 *       | [11] key-set index | [12..27] y (x[8] | y[8]) | then per local party k_i [8] | sigma_i [8] | R [16]
 *     This layout is this library's own: the reference derives no `Serialize` for `CompletedOfflineStage`, there is no byte parity to
 *     claim.  A record holds k_i in the clear: importing one record twice, or into two pools, is the nonce reuse the slots prevent.
 *     Sealing a record (mpe_gg20_sealed_presig_export / _import below) closes DISCLOSURE and FORGERY: k_i leaves the device
 *     encrypted, and an edited record, or one sealed under another wallet's wrapping key, is refused.  It does not close REPLAY: a
 *     sealed record imports as often as it is presented, and keeping it from being presented twice stays the caller's duty.
 * mpe_gg20_presig_discard   READY, SIGNED or EMPTY -> EMPTY with the wipe (a slot that a running call on another stream holds BUSY is
 *     left to that call).
 * A slot remembers the signer set its session signed with (mpe_gg20_session_create_sets; set 0 otherwise) beside the key set: export
 * writes that set's party mask into word [1].  sign and complete need no set.  Sessions whose local party was given by index are not
 * deposited (MPE_E_ARG): the pool's local parties are ordinals.
 * mpe_gg20_presig_pool_audit  h_out[0..3] = slots that are EMPTY, READY, SIGNED, BUSY; h_out[4] = non-zero words of k_i, sigma_i in
 *     slots that are not READY (must be 0).  Synchronises the stream. */
#define MPE_GG20_PRESIG_RECORD_VERSION 1
#define MPE_GG20_PRESIG_DEPOSIT_RANGE 801
#define MPE_GG20_PRESIG_DEPOSIT_NOT_EMPTY 802
#define MPE_GG20_PRESIG_SESSION_FAILED 803
#define MPE_GG20_PRESIG_SIGN_RANGE 811
#define MPE_GG20_PRESIG_SIGN_NOT_READY 812
#define MPE_GG20_PRESIG_COMPLETE_RANGE 821
#define MPE_GG20_PRESIG_COMPLETE_NOT_SIGNED 822
#define MPE_GG20_PRESIG_VERIFY_FAILED 701
#define MPE_GG20_PRESIG_RECORD_RANGE 831
#define MPE_GG20_PRESIG_IMPORT_REFUSED 832
#define MPE_GG20_PRESIG_EXPORT_NOT_READY 833
#define MPE_GG20_PRESIG_IMPORT_NOT_EMPTY 834
typedef struct mpe_gg20_presig_pool mpe_gg20_presig_pool;
int mpe_gg20_presig_pool_create(mpe_ctx* ctx, const mpe_gg20_keys* keys, int n_local, const int32_t* h_local, int capacity,
                                mpe_gg20_presig_pool** out);
int mpe_gg20_presig_pool_destroy(mpe_gg20_presig_pool* pool);
int mpe_gg20_presig_pool_capacity(const mpe_gg20_presig_pool* pool);
int mpe_gg20_presig_record_words(const mpe_gg20_presig_pool* pool);
int mpe_gg20_presig_deposit(mpe_gg20_presig_pool* pool, mpe_gg20_session* sess, const int32_t* d_slot, int32_t* d_status, void* stream);
int mpe_gg20_presig_sign(mpe_gg20_presig_pool* pool, int count, const int32_t* d_slot, const uint32_t* d_msg, uint32_t* d_s_i,
                         int32_t* d_status, void* stream);
int mpe_gg20_presig_complete(mpe_gg20_presig_pool* pool, int count, const int32_t* d_slot, const uint32_t* d_in, const int64_t* h_in_off,
                             uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, int32_t* d_status, void* stream);
int mpe_gg20_presig_export(mpe_gg20_presig_pool* pool, int count, const int32_t* d_slot, uint32_t* d_rec, int32_t* d_status, void* stream);
int mpe_gg20_presig_import(mpe_gg20_presig_pool* pool, int count, const int32_t* d_slot, const uint32_t* d_rec, int32_t* d_status,
                           void* stream);
int mpe_gg20_presig_discard(mpe_gg20_presig_pool* pool, int count, const int32_t* d_slot, void* stream);
int mpe_gg20_presig_pool_audit(mpe_gg20_presig_pool* pool, int64_t* h_out, void* stream);
/* The online step in ONE launch, for a pool that holds all S signers (n_local == S; MPE_E_ARG otherwise): sign + complete of the rows'
 * slots without the SIGNED state in between.  A row claims its READY slot with the same single compare-and-swap, computes every
 * s_i = m k_i + r sigma_i (k_i and sigma_i zeroed at once), sums them, normalises to low s with the recid flip, runs output_signature's
 * verify ONCE and returns the slot to EMPTY with the wipe.  One verify is exact: with every signer in the pool the S parties of
 * sign + complete verify the same (r, s) under the same y — the argument of dedup_verify.  (A slot whose parties do not hold one and
 * the same R, which no offline stage leaves and only an import can make, is 701.)  d_r, d_s [count][8], d_recid, d_status [count]:
 * what mpe_gg20_sign reports per session; 811 / 812 from the claim (among duplicate indices exactly one row wins), 701 when the
 * verify fails; zero outputs unless status 0.  d_status may be NULL. */
int mpe_gg20_sign_online(mpe_gg20_presig_pool* pool, int count, const int32_t* d_slot, const uint32_t* d_msg, uint32_t* d_r,
                                uint32_t* d_s, int32_t* d_recid, int32_t* d_status, void* stream);

/* ---- sealed records: presignatures and key shares leave the device encrypted ------------------------------------------------
 * ChaCha20-Poly1305 exactly as RFC 8439 §2.8 defines it, on the device, under a WRAPPING KEY: 32 bytes from the operator's KMS or
 * HSM — the one secret the host handles.  mpe_wrap_key_create copies them (h_key32: HOST pointer) into device memory the object owns;
 * _destroy zeroes that memory before it frees it (and waits for the device: calls on any stream may still read the key).
 *     The SEALED ROW (this library's own layout, little-endian 32-bit words taken as their byte image): words + 10 words for a
 *     payload of `words` words, 1 <= words <= MPE_SEAL_MAX_WORDS:
 *       [0] MPE_SEAL_MAGIC (bytes "MPS1") | [1] kind | [2] words | [3..5] nonce = (row index within the call, low 32 bits of nonce_hi,
 *       high 32 bits) — ChaCha20's state[13..15] | [6 .. 6+words) ciphertext | [6+words .. 10+words) Poly1305 tag
 *     AAD = words [0..2] as 12 bytes, so kind and length are authenticated; the one-time Poly1305 key is the first 32 bytes of block 0,
 *     the payload is XORed with blocks 1, 2, ...  Kinds: MPE_SEAL_KIND_PRESIG (1) a presignature record, MPE_SEAL_KIND_KEYSHARE (2) a
 *     GG20 key share, >= MPE_SEAL_KIND_USER (16) the caller's own rows.
 * nonce_hi: a (wrapping key, nonce_hi) pair must NEVER be used twice — the caller's contract, like the sampler's (seed, stream_id):
 *     two calls that seal under the same pair encrypt their rows with the same keystream and MAC them with the same one-time keys.
 *     64 random bits per call, or a counter kept with the key, both do.
 * mpe_seal      d_plain [count][words] -> d_sealed [count][words + 10].
 * mpe_unseal    d_sealed -> d_plain [count][words], d_status [count] (may be NULL): 0, or MPE_SEAL_REFUSED (841) for a row whose magic,
 *     kind, length or tag does not match.  A row is authenticated before it is decrypted; the tag is compared without an early exit; a
 *     refused row's plaintext row is all zero — unauthenticated plaintext is never written.
 *     The generic pair takes kinds >= MPE_SEAL_KIND_USER only: kinds 1 and 2 are MPE_E_ARG, so that a sealed presignature or key share
 *     is not turned back into clear words through it.
 * mpe_poly1305  the one-time-key MAC on its own: d_key [count][8] (r [4] | s [4]), d_msg [count][msg_bytes] bytes, d_tag [count][4].
 * mpe_gg20_sealed_presig_export / _import: mpe_gg20_presig_export / _import with the record (kind 1) sealed, rows of
 *     mpe_gg20_sealed_presig_words(pool) = record words + 10; the same state transitions and row statuses.  A row that exports nothing
 *     (831, 833) gets an all-zero sealed row.  Import AUTHENTICATES BEFORE IT CLAIMS: a row that fails authentication reports 841 and
 *     its slot stays EMPTY and untouched; an authenticated record is then judged by import's own rules (832, 834).  The clear records
 *     exist only in a stage inside the pool's context's workspace (counted by mpe_ctx_scratch_audit), which the same call zeroes in
 *     stream order: after the call no device buffer outside the pool holds a clear record.  What sealing closes and what it does not:
 *     see mpe_gg20_presig_import above.
 * mpe_gg20_keyshare_seal: rows x [8] | p [32] | q [32] = MPE_GG20_KEYSHARE_WORDS (72) payload words, kind 2, gathered from d_x
 *     [count][8], d_p, d_q [count][32] -> d_sealed [count][82]: key generation seals its shares before anything is copied out.
 * mpe_gg20_keys_create_sealed: mpe_gg20_keys_create_sets with d_x, d_p, d_q replaced by the wrapping key and d_sealed_shares
 *     [nkeysets][n_own][82]: unseals into device memory of its own, builds the object through the existing path and zeroes the clear
 *     rows.  Any refused row fails the call (MPE_E_ARG) and creates no object.  Synchronises the stream. */
#define MPE_SEAL_MAGIC ((uint32_t)0x3153504du)
#define MPE_SEAL_REFUSED ((int)841)
#define MPE_SEAL_MAX_WORDS ((int)4096)
#define MPE_SEAL_KIND_PRESIG ((uint32_t)1)
#define MPE_SEAL_KIND_KEYSHARE ((uint32_t)2)
#define MPE_SEAL_KIND_USER ((uint32_t)16)
#define MPE_GG20_KEYSHARE_WORDS ((int)72)
typedef struct mpe_wrap_key mpe_wrap_key;
int mpe_wrap_key_create(mpe_ctx* ctx, const uint8_t* h_key32, mpe_wrap_key** out);
int mpe_wrap_key_destroy(mpe_wrap_key* key);
int mpe_seal(mpe_ctx* ctx, const mpe_wrap_key* key, uint32_t kind, int count, int words, const uint32_t* d_plain, uint64_t nonce_hi,
             uint32_t* d_sealed, void* stream);
int mpe_unseal(mpe_ctx* ctx, const mpe_wrap_key* key, uint32_t kind, int count, int words, const uint32_t* d_sealed, uint32_t* d_plain,
               int32_t* d_status, void* stream);
int mpe_poly1305(mpe_ctx* ctx, int count, const uint32_t* d_key, const uint8_t* d_msg, size_t msg_bytes, uint32_t* d_tag, void* stream);
int mpe_gg20_sealed_presig_words(const mpe_gg20_presig_pool* pool);
int mpe_gg20_sealed_presig_export(mpe_gg20_presig_pool* pool, const mpe_wrap_key* key, int count, const int32_t* d_slot, uint64_t nonce_hi,
                                  uint32_t* d_sealed, int32_t* d_status, void* stream);
int mpe_gg20_sealed_presig_import(mpe_gg20_presig_pool* pool, const mpe_wrap_key* key, int count, const int32_t* d_slot,
                                  const uint32_t* d_sealed, int32_t* d_status, void* stream);
int mpe_gg20_keyshare_seal(mpe_ctx* ctx, const mpe_wrap_key* key, int count, const uint32_t* d_x, const uint32_t* d_p, const uint32_t* d_q,
                           uint64_t nonce_hi, uint32_t* d_sealed, void* stream);
int mpe_gg20_keys_create_sealed(mpe_ctx* ctx, int t, int n, int n_signers, int n_sets, const int32_t* h_sets, int nkeysets, int n_own,
                                const int32_t* h_own, const mpe_wrap_key* key, const uint32_t* d_sealed_shares, const uint32_t* d_N,
                                const uint32_t* d_Nt, const uint32_t* d_h1, const uint32_t* d_h2, const uint32_t* d_y, const uint32_t* d_X,
                                mpe_gg20_keys** out, void* stream);

/* ---- identifiable abort: src/protocols/multi_party_ecdsa/gg_2020/blame.rs ---------------------------------------- */
/* Every signer has opened the values the failing phase used; the functions re-derive the public ciphertexts from the
 * openings under the signers' PUBLIC Paillier keys and name the parties whose openings do not match or whose broadcast
 * value is inconsistent.  Layout: leading dimensions [batch][S] (signer ordinal), then the peer slot j (S-1; the peer's
 * ordinal is ind = j < i ? j : j+1).  d_bad_actors [batch]: bit mask over signer ordinals = the reference's sorted,
 * de-duplicated `ErrorType::bad_actors`.
 * `GlobalStatePhase5::phase5_blame` (blame.rs:116-224), called when phase5_check_R_dash_sum failed (status 502):
 *   k, gamma [B][S][8]; k_rand [B][S][64] (the MessageA randomness); beta_tag, beta_rand [B][S][S-1][64] (for Alice i, slot j:
 *   what Bob `ind` used in his gamma MessageB to i); delta [B][S][8]; g_gamma [B][S][16]; c_a [B][S][128] (m_a_vec[i].c);
 *   c_b [B][S][S-1][128] (m_b_mat[i][j].c, the gamma MessageB ciphertexts Alice i received). */
typedef struct { const uint32_t *k, *k_rand, *gamma, *beta_tag, *beta_rand, *delta, *g_gamma, *c_a, *c_b; } mpe_gg20_blame5_in;
int mpe_gg20_blame5(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const mpe_gg20_blame5_in* in,
                    uint32_t* d_bad_actors, void* stream);
/* `GlobalStatePhase6::phase6_blame` (blame.rs:322-421), called when phase6_check_S_i_sum failed (status 602):
 *   k, k_rand as above; miu, miu_rand [B][S][S-1][64] (plaintext before reduction and Paillier randomness of the w_i MessageB
 *   ciphertexts Alice i received, `Paillier::open`); a1, a2 [B][S][16], z [B][S][8] (each signer's ECDDHProof that
 *   S_i = sigma_i R); S [B][S][16]; c_a [B][S][128]; c_b [B][S][S-1][128] (the w_i MessageB ciphertexts); R [B][16]. */
typedef struct { const uint32_t *k, *k_rand, *miu, *miu_rand, *a1, *a2, *z, *S, *c_a, *c_b, *R; } mpe_gg20_blame6_in;
int mpe_gg20_blame6(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const mpe_gg20_blame6_in* in,
                    uint32_t* d_bad_actors, void* stream);
/* The two for sessions that name their signer set (d_sigset [batch], NULL = set 0; an index out of range reads as set 0): the [S]
 * dimension and the bad_actors bits are ordinals of each session's own set.  blame7 needs no set. */
int mpe_gg20_blame5_sets(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const int32_t* d_sigset,
                         const mpe_gg20_blame5_in* in, uint32_t* d_bad_actors, void* stream);
int mpe_gg20_blame6_sets(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const int32_t* d_sigset,
                         const mpe_gg20_blame6_in* in, uint32_t* d_bad_actors, void* stream);
/* `GlobalStatePhase7::phase7_blame` (blame.rs:434-454), called when the signature did not verify (status 701):
 *   s [B][S][8] (partial signatures); r, m [B][8]; R_dash, S [B][S][16]; R [B][16]:  R s_i == m R_dash_i + r S_i. */
typedef struct { const uint32_t *s, *r, *R_dash, *m, *R, *S; } mpe_gg20_blame7_in;
int mpe_gg20_blame7(mpe_ctx* ctx, int n_signers, int batch, const mpe_gg20_blame7_in* in, uint32_t* d_bad_actors, void* stream);
/* What a local party publishes for the phase-6 blame beyond the inputs it was given (LocalStatePhase6, blame.rs:227-234):
 * d_miu [n_local][batch][S-1][64] and the ECDDH proof d_a1, d_a2 [n_local][batch][16], d_z [n_local][batch][8] that
 * S_i = sigma_i R (`GlobalStatePhase6::ecddh_proof`, blame.rs:258-272; d_nonce [batch][n_local][8] is its sampled value).
 * Valid after round 5.  (The Paillier randomness of the incoming ciphertexts: mpe_paillier_open.) */
int mpe_gg20_session_blame6_state(const mpe_gg20_session* sess, const uint32_t* d_nonce, uint32_t* d_miu, uint32_t* d_a1,
                                  uint32_t* d_a2, uint32_t* d_z, void* stream);
/* curv `ECDDHProof::{prove, verify}` for the statement {g1, h1 = x g1, g2, h2 = x g2}: a1 = s g1, a2 = s g2,
 * e = H(g1, h1, g2, h2, a1, a2), z = s + e x; verify: z g1 == a1 + e h1 and z g2 == a2 + e h2.  Points [batch][16]. */
typedef struct { const uint32_t *g1, *h1, *g2, *h2; } mpe_ecddh_statement;
typedef struct { uint32_t *a1, *a2, *z; } mpe_ecddh_proof;
int mpe_ecddh_prove(mpe_ctx* ctx, int batch, const uint32_t* d_x, const uint32_t* d_s, const mpe_ecddh_statement* statement,
                    const mpe_ecddh_proof* out, void* stream);
int mpe_ecddh_verify(mpe_ctx* ctx, int batch, const mpe_ecddh_statement* statement, const mpe_ecddh_proof* proof, uint8_t* d_ok,
                     void* stream);

/* ---- SHA-512, HMAC-SHA512 and BIP32 public derivation -----------------------------------------------------------------------------
 * One item per lane.  Byte arrays are device uint8_t rows of a length fixed per call.
 * mpe_sha512       d_msg [batch][msg_bytes] -> d_out [batch][64], 0 <= msg_bytes <= MPE_SHA512_MAX_MSG_BYTES (65 536).
 * mpe_hmac_sha512  d_key [batch][key_bytes], 0 <= key_bytes <= 128 (a longer key is MPE_E_ARG: RFC 2104's hash-the-key branch is not
 *                  built), d_msg as above -> d_out [batch][64].
 * mpe_bip32_derive CKDpub along a path of non-hardened indices, one row per lane.  Parents: d_parent_pub [n_parents][16] (x [8] | y [8]
 *                  little-endian words, as every point here), d_parent_cc [n_parents][32] bytes; row b starts from parent
 *                  d_parent_idx[b] (NULL = parent 0) and walks d_path[b][0 .. d_depth[b]) (d_path [batch][max_depth], 1 <= max_depth <=
 *                  MPE_BIP32_MAX_DEPTH).  Per level I = HMAC-SHA512(cc, serP(K) | ser32(i)); tweak += I_L mod q; K += I_L G; cc = I_R.
 *                  Outputs: d_tweak [batch][8] (the sum of the I_L: child private key = parent private key + tweak mod q — what
 *                  mpe_gg20_session_create_tweaks takes), d_child_pub [batch][16], d_child_cc [batch][32], d_status [batch]:
 *                    0 ok (depth 0: tweak 0, the parent's key and chain code)
 *                    MPE_BIP32_STATUS_HARDENED  an index >= 2^31 on the path (hardened derivation needs the private key)
 *                    MPE_BIP32_STATUS_INVALID   I_L >= q or a child at infinity at some level (BIP32: take the next index — the
 *                                               caller's choice), or a parent that is not a valid point
 *                    MPE_BIP32_STATUS_DEPTH     d_depth[b] outside [0, max_depth] or d_parent_idx[b] outside [0, n_parents)
 *                  A FAILED ROW NEVER READS AS "TWEAK 0" (which would sign for the parent): its tweak is 0xFFFFFFFF x 8 (>= q: a session
 *                  refuses it with MPE_GG20_STATUS_BAD_TWEAK), its child key and chain code are zero. */
#define MPE_SHA512_MAX_MSG_BYTES ((int)65536)
#define MPE_BIP32_MAX_DEPTH ((int)16)
#define MPE_BIP32_STATUS_HARDENED ((int)1)
#define MPE_BIP32_STATUS_INVALID ((int)2)
#define MPE_BIP32_STATUS_DEPTH ((int)3)
int mpe_sha512(mpe_ctx* ctx, int batch, const uint8_t* d_msg, int msg_bytes, uint8_t* d_out, void* stream);
int mpe_hmac_sha512(mpe_ctx* ctx, int batch, const uint8_t* d_key, int key_bytes, const uint8_t* d_msg, int msg_bytes, uint8_t* d_out,
                    void* stream);
int mpe_bip32_derive(mpe_ctx* ctx, int batch, int n_parents, const uint32_t* d_parent_pub, const uint8_t* d_parent_cc,
                     const int32_t* d_parent_idx, const uint32_t* d_path, const int32_t* d_depth, int max_depth, uint32_t* d_tweak,
                     uint32_t* d_child_pub, uint8_t* d_child_cc, int32_t* d_status, void* stream);
/* The lock-step composition of the rounds above with every signer local (needs every signer's secrets in `keys`):
 * OfflineStage Round0..Round6 and SignManual for `batch` sessions on this GPU — what `round_based::dev::Simulation`
 * does for one session (state_machine/sign.rs:667-763).  nonces: [batch][S] layout.  Outputs per session: d_r, d_s
 * [batch][8] and d_recid [batch] = `SignatureRecid{r,s,recid}` (party_i.rs:131-135, low-s normalised, 873-910; zero
 * unless status == 0), optionally d_R [batch][16], and d_status [batch] = the smallest non-zero party status (0 = every
 * party produced and verified the signature).  chunk: sessions per internal pass (0 = 65536, fewer for wide shapes so
 * that a pass stays under ~64 GB).  Scratch that held nonce-derived values is zeroed before the call returns. */
int mpe_gg20_sign(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const mpe_gg20_nonces* nonces,
                  uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, int32_t* d_status, int dedup_verify, int chunk,
                  void* stream);
/* ... with a signer set per session (d_sigset [batch], device; NULL = mpe_gg20_sign): `keys` must hold the secrets of every member of
 * every one of its sets.  A session whose index is out of range ends with status MPE_GG20_STATUS_BAD_SET and zero outputs. */
int mpe_gg20_sign_sets(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const int32_t* d_sigset,
                       const mpe_gg20_nonces* nonces, uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, int32_t* d_status,
                       int dedup_verify, int chunk, void* stream);
/* ... with a tweak per session (d_tweak [batch][8], device; NULL = mpe_gg20_sign_sets): session b signs for the child key y + t_b G
 * (mpe_gg20_session_create_tweaks).  A session whose tweak is refused ends with status MPE_GG20_STATUS_BAD_TWEAK and zero outputs. */
int mpe_gg20_sign_tweaks(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const int32_t* d_sigset,
                         const uint32_t* d_tweak, const mpe_gg20_nonces* nonces, uint32_t* d_r, uint32_t* d_s, int32_t* d_recid,
                         uint32_t* d_R, int32_t* d_status, int dedup_verify, int chunk, void* stream);
/* The offline stage alone, as one call: chunks and runs rounds 0-6 exactly as mpe_gg20_sign_sets does and, where that function signs,
 * deposits every chunk into `pool`; the same scratch is zeroed before the call returns.  nonces->msg is not read and may be NULL.
 * `pool` must be over `keys`, on this context's device, with all S ordinals local, else MPE_E_ARG and nothing is touched.  Row b goes to
 * slot d_slot[b] ([batch], device).  d_status [batch]: the session's smallest non-zero party status if the session failed — what
 * mpe_gg20_sign would report, MPE_GG20_STATUS_BAD_SET for a set index out of range included, not the pool's blanket 803 — otherwise
 * the deposit's 801 / 802, otherwise 0.  A row with a non-zero status leaves its slot untouched. */
int mpe_gg20_presign_sets(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, const int32_t* d_keyset, const int32_t* d_sigset,
                          const mpe_gg20_nonces* nonces, mpe_gg20_presig_pool* pool, const int32_t* d_slot, int32_t* d_status,
                          int dedup_verify, int chunk, void* stream);

/* ---- a stream of batches: the pipelined engine ------------------------------------------------------------------------
 * A signing service receives batch after batch of `batch` sessions (BASELINE config 4: 1 024) and one such batch alone is
 * latency-bound (chains of ~2 048 dependent squarings at a fraction of the chip).  The reference runs many `OfflineStage`s
 * concurrently on one executor (state_machine/sign.rs:667-691; rounds.rs:106,215,323 `is_expensive`).  Here:
 * `group` consecutive batches are coalesced into ONE lock-step pass (every heavy launch carries the items of all of them) and
 * `lanes` (1..4) such passes are in flight at once, each on one stream of its own with its own workspace — at most 4 streams,
 * the runtime's default hardware queues, ONE host thread: submit only enqueues.  Results are bit-identical to mpe_gg20_sign.
 *   submit         the caller's sampled values of ONE batch (layout of mpe_gg20_nonces with every signer local, as for
 *                  mpe_gg20_sign) and where its results go: d_r, d_s [batch][8], d_recid, d_status [batch], d_R [batch][16] or NULL.
 *                  `stream`: the stream that produced the inputs (the pipeline waits for it).  Inputs are copied and results
 *                  written ASYNCHRONOUSLY: both sets of arrays must stay valid until the ticket completes.
 *   submit_seeded  the same, but every sampled value is drawn on the device from (h_seed32, batch_counter) exactly as
 *                  mpe_gg20_sample_nonces does (one sampler launch per group, right before its pass; group <= 16); d_msg [batch][8]
 *                  are the messages.  A (seed, batch_counter) pair signs ONE batch.  A group holds batches of one form only.
 *   flush          sends the partly filled group to the device (a service calls it when its queue runs dry)
 *   wait           blocks the host until the batch of `ticket` is complete (flushing its group if it is still open);
 *   stream_wait    makes `stream` wait for it instead;  query: *done = 0 / 1 without blocking
 *   latency_ms     device time from the submit call to the completion of that batch's results (includes the time the batch waited
 *                  for its group to fill and for a lane);  pass_ms: from the start of the pass that carried it to its completion
 * One pipeline object is driven by one host thread at a time.  Destroying it waits for the work in flight and wipes its staging. */
typedef struct mpe_gg20_pipeline mpe_gg20_pipeline;
int mpe_gg20_pipeline_create(mpe_ctx* ctx, const mpe_gg20_keys* keys, int batch, int group, int lanes, int dedup_verify,
                             mpe_gg20_pipeline** out);
int mpe_gg20_pipeline_destroy(mpe_gg20_pipeline* p);
int mpe_gg20_pipeline_submit(mpe_gg20_pipeline* p, const int32_t* d_keyset, const mpe_gg20_nonces* nonces, uint32_t* d_r, uint32_t* d_s,
                             int32_t* d_recid, uint32_t* d_R, int32_t* d_status, void* stream, uint64_t* ticket);
int mpe_gg20_pipeline_submit_seeded(mpe_gg20_pipeline* p, const int32_t* d_keyset, const uint8_t* h_seed32, uint64_t batch_counter,
                                    const uint32_t* d_msg, uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, int32_t* d_status,
                                    void* stream, uint64_t* ticket);
/* ... with a signer set per session (d_sigset [batch], device, staged next to d_keyset; NULL = the two calls above): `keys` must hold the
 * secrets of every member of every one of its sets, else MPE_E_ARG.  A group may mix batches with and without sets (without: set 0);
 * a group in which no batch names its sets launches what mpe_gg20_sign launches.  An index out of range is that session's
 * MPE_GG20_STATUS_BAD_SET.  The seeded form draws every value as mpe_gg20_sample_nonces_sets does. */
int mpe_gg20_pipeline_submit_sets(mpe_gg20_pipeline* p, const int32_t* d_keyset, const int32_t* d_sigset, const mpe_gg20_nonces* nonces,
                                  uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, uint32_t* d_R, int32_t* d_status, void* stream,
                                  uint64_t* ticket);
int mpe_gg20_pipeline_submit_seeded_sets(mpe_gg20_pipeline* p, const int32_t* d_keyset, const int32_t* d_sigset, const uint8_t* h_seed32,
                                         uint64_t batch_counter, const uint32_t* d_msg, uint32_t* d_r, uint32_t* d_s, int32_t* d_recid,
                                         uint32_t* d_R, int32_t* d_status, void* stream, uint64_t* ticket);
/* A PRESIG engine: the same object — tickets, grouping, flush / wait / query / poll, deadline, eager, latency, counters, inject_fault —
 * whose passes end in the deposit of mpe_gg20_presign_sets into `pool` (over `keys`, same device, all S ordinals local; `keys` must hold
 * the secrets of every member of every one of its sets) instead of rounds 7-8.
 *   submit_presig         the caller's sampled values of ONE batch (nonces->msg is not read and may be NULL), d_keyset / d_sigset as
 *                         above (NULL = key set 0 / set 0), d_slot [batch] the pool slots of its rows, staged like d_keyset;
 *                         d_status [batch] is the one result array, with the statuses of mpe_gg20_presign_sets
 *   submit_presig_seeded  the seeded form; there is no message
 * Which slots are free stays the caller's policy.  All lanes deposit into the one pool concurrently, and other calls on the pool may
 * run beside them: the slot's compare-and-swap makes that safe, a row that loses it reads 802 and touches nothing.
 * Submitting the wrong kind (submit / submit_seeded to a presig engine, submit_presig* to a signing engine) is MPE_E_ARG before a
 * slot or a ticket is taken.  Failure contract: a failed pass fills every batch's d_status with MPE_GG20_STATUS_PASS_FAILED(rc); the
 * deposit is the last step of a pass, so no slot of that group has left EMPTY (a group of more than 65 536 sessions runs in several
 * chunks: rows of chunks that were deposited before a later chunk failed read PASS_FAILED too and their slots are the caller's to
 * discard).  The next group deposits.  The engine is destroyed BEFORE its pool. */
int mpe_gg20_pipeline_create_presig(mpe_ctx* ctx, const mpe_gg20_keys* keys, mpe_gg20_presig_pool* pool, int batch, int group, int lanes,
                                    int dedup_verify, mpe_gg20_pipeline** out);
int mpe_gg20_pipeline_submit_presig(mpe_gg20_pipeline* p, const int32_t* d_keyset, const int32_t* d_sigset, const mpe_gg20_nonces* nonces,
                                    const int32_t* d_slot, int32_t* d_status, void* stream, uint64_t* ticket);
int mpe_gg20_pipeline_submit_presig_seeded(mpe_gg20_pipeline* p, const int32_t* d_keyset, const int32_t* d_sigset, const uint8_t* h_seed32,
                                           uint64_t batch_counter, const int32_t* d_slot, int32_t* d_status, void* stream, uint64_t* ticket);
int mpe_gg20_pipeline_flush(mpe_gg20_pipeline* p);
int mpe_gg20_pipeline_query(mpe_gg20_pipeline* p, uint64_t ticket, int* done);
int mpe_gg20_pipeline_wait(mpe_gg20_pipeline* p, uint64_t ticket);
int mpe_gg20_pipeline_stream_wait(mpe_gg20_pipeline* p, uint64_t ticket, void* stream);
int mpe_gg20_pipeline_latency_ms(mpe_gg20_pipeline* p, uint64_t ticket, float* ms);
int mpe_gg20_pipeline_pass_ms(mpe_gg20_pipeline* p, uint64_t ticket, float* ms);
/* Failure contract.  A failing CHECK of a session is that session's status (above), never an error.  When the PASS that carries a
 * group fails as a whole (MPE_E_NOMEM / MPE_E_HIP from the sampler or the lock-step composition), every batch of that group is
 * told: its d_status array is filled with MPE_GG20_STATUS_PASS_FAILED(rc), its d_r / d_s / d_recid (/ d_R) are zeroed (on the
 * lane's stream, ordered before the ticket completes), and wait / stream_wait / latency_ms / pass_ms — and query once the ticket
 * is done — return that rc for EACH of its tickets.  submit itself returns MPE_OK when the batch was accepted: an error belongs
 * to the batches of the failed pass, not to the caller whose submission happened to close the group.  Later groups are unaffected.
 * (The reference reports per session and never drops an error: gg_2020/mod.rs:23-27, state_machine/sign/rounds.rs:696-713.)
 *   ticket_rc      *launched = 0 while the batch's group is still open; otherwise *rc = the pass's return code
 *   inject_fault   test hook: the next `passes` passes fail with rc (MPE_E_NOMEM or MPE_E_HIP) after their inputs were staged */
#define MPE_GG20_STATUS_PASS_FAILED(rc) (9000 - (rc))        /* 9001 MPE_E_ARG, 9002 MPE_E_HIP, 9003 MPE_E_NOMEM */
int mpe_gg20_pipeline_ticket_rc(mpe_gg20_pipeline* p, uint64_t ticket, int* launched, int* rc);
int mpe_gg20_pipeline_inject_fault(mpe_gg20_pipeline* p, int passes, int rc);
/* When a part-filled group goes to the device: when it is full, on flush / wait, and — evaluated inside every submit / query /
 * poll call of the ONE host thread that drives the pipeline, there is no hidden thread —
 *   set_deadline_us   when its oldest batch has waited `us` microseconds of host time (us < 0: never, the default);
 *   set_eager         as soon as the lane it would run on is idle: arrival-driven grouping — a trickle of batches starts at once,
 *                     under load the lanes are busy and the groups fill by themselves (off by default);
 *   poll              applies both rules now (a service calls it from its loop); *launched = 1 if a group went.
 * counters: groups launched in total / by the deadline / by an idle lane / failed passes. */
int mpe_gg20_pipeline_set_deadline_us(mpe_gg20_pipeline* p, int64_t us);
int mpe_gg20_pipeline_set_eager(mpe_gg20_pipeline* p, int on);
int mpe_gg20_pipeline_poll(mpe_gg20_pipeline* p, int* launched);
int mpe_gg20_pipeline_counters(const mpe_gg20_pipeline* p, uint64_t* groups, uint64_t* by_deadline, uint64_t* by_idle, uint64_t* failed);
/* items of the seeded submissions whose rejection loops gave up (see mpe_sample_below); waits for the lanes */
int mpe_gg20_pipeline_sampler_failures(mpe_gg20_pipeline* p, int32_t* h_out);


/* ---- multi-GPU: the per-round message fan-out behind the C-ABI (RCCL over xGMI; SURVEY.md 8e B, BASELINE config 5) ------------
 * Party-sharded signing: the parties of a session live on DIFFERENT GPUs (one process per GPU) and every round's messages travel
 * through ONE all-gather, after which each party reads what is addressed to it — the reference's relay broadcasts every message,
 * P2P ones included, to the room and the client filters (examples/gg20_sm_client.rs:35-40; state_machine/sign.rs:252-438).
 *   mpe_comm_unique_id   ncclGetUniqueId: ONE rank calls it, the host carries the MPE_COMM_ID_BYTES bytes to the others (any channel)
 *   mpe_comm_create      ncclCommInitRank on the context's device; blocks until all `world` ranks have called it
 *   mpe_comm_all_gather  d_buf = [world][bytes_per_rank]; this rank's block already sits at rank * bytes_per_rank; one ncclAllGather
 *                        queued on `stream` fills the others (in place; from a copy of the block when the self-test chose that form)
 *   mpe_comm_layout_self_test  one all-gather of known row patterns on the REAL communicator before any signing work: in place
 *                        first, then the copy form; all ranks agree (ncclAllReduce) on the first form that puts every row of every rank
 *                        where h_in_off will look for it.  *h_mode = 0 in place / 1 copy, *h_ok = 1; an error when neither is right.
 * Placement of party p (signer ordinal) of session block s:
 *   MPE_PLACE_PARTY    rank p % world, slot p / world (world divides S; one block);
 *   MPE_PLACE_ROTATED  world blocks; rank (s + p) % world, slot p — every rank hosts S (block, party) pairs for any world size, and
 *                      with world >= S no two parties of a session share a GPU.
 * The gather buffer is [world * per_rank] rows of [batch][W(round)] records; rank r owns rows [r * per_rank, (r + 1) * per_rank), row
 * r * per_rank + slot = that pair's outgoing records (mpe_gg20_roundN's d_out points there).  mpe_gg20_shard_in_off gives, for a
 * block, the record offset of every sender's row: the h_in_off argument of the next mpe_gg20_roundN, which reads the gathered
 * buffer in place.  mpe_gg20_round_exchange = the all-gather of round `round`'s records (per_rank * batch * W words per rank). */
#define MPE_COMM_ID_BYTES 128
#define MPE_PLACE_PARTY 0
#define MPE_PLACE_ROTATED 1
typedef struct mpe_comm mpe_comm;
int mpe_comm_unique_id(uint8_t* h_id);
int mpe_comm_create(mpe_ctx* ctx, const uint8_t* h_id, int rank, int world, mpe_comm** out);
int mpe_comm_destroy(mpe_comm* comm);
/* RCCL is bound at run time (dlopen) by the first communicator call — libmpecdsa_hip.so itself does not link it, so single-GPU
 * users need no librccl.  A copy the process ALREADY holds (PyTorch loads its own librccl.so.1) is adopted, so a process never
 * runs two RCCL instances; otherwise librccl.so.1 is searched on the loader path, then under $ROCM_PATH/lib (/opt/rocm/lib).
 * mpe_comm_library: the bound file (path_buf, NUL-terminated, may be NULL), *adopted = 1 if it was already loaded, *version =
 * ncclGetVersion.  MPE_E_HIP (and mpe_last_error) when no RCCL can be found. */
int mpe_comm_library(char* path_buf, size_t path_cap, int* adopted, int* version);
int mpe_comm_rank(const mpe_comm* comm);
int mpe_comm_world(const mpe_comm* comm);
int mpe_comm_gather_mode(const mpe_comm* comm);
int mpe_comm_all_gather(mpe_comm* comm, void* d_buf, size_t bytes_per_rank, void* stream);
int mpe_comm_layout_self_test(mpe_comm* comm, int rows_per_rank, int* h_mode, int* h_ok, void* stream);
int mpe_gg20_shard_where(int placement, int n_signers, int world, int block, int party, int* rank, int* slot);
int mpe_gg20_shard_blocks(int placement, int n_signers, int world);
int mpe_gg20_shard_per_rank(int placement, int n_signers, int world);
int mpe_gg20_shard_in_off(int placement, int n_signers, int world, int batch, int block, int64_t* h_in_off);
int mpe_gg20_round_exchange(mpe_comm* comm, int n_signers, int n, int round, int per_rank, int batch, uint32_t* d_slab, void* stream);

/* ---- keygen VERIFICATION math (src/protocols/multi_party_ecdsa/gg_2020/party_i.rs:260-438) ----------------------- */
/* What every party checks about every other party's first keygen messages and shares, batched over (verifier, prover)
 * pairs / wallets.  Every key is its own modulus: the moduli set is built per call.  The two zk-paillier 0.4.3 proofs are
 * un-vendored; their definitions are recalled.
 * `NiCorrectKeyProof::verify(ek, SALT_STRING)` (party_i.rs:286-289): d_N [batch][64], d_sigma [batch][11][64]:
 *   sigma_i^N == rho_i (mod N) for the 11 hash-derived rho_i and no prime below 6370 divides N. */
int mpe_correct_key_verify(mpe_ctx* ctx, int batch, const uint32_t* d_N, const uint32_t* d_sigma, uint8_t* d_ok, void* stream);
/* `CompositeDLogProof{x, y}::verify(DLogStatement{N, g, ni})` (party_i.rs:294-301; called twice per prover, bases h1 and h2):
 *   N >= 2^128 and odd, gcd(g, N) = gcd(ni, N) = 1, e = H(x, g, N, ni), x == g^y ni^e mod N.  d_y [batch][73]. */
int mpe_composite_dlog_verify(mpe_ctx* ctx, int batch, const uint32_t* d_N, const uint32_t* d_g, const uint32_t* d_ni,
                              const uint32_t* d_x, const uint32_t* d_y, uint8_t* d_ok, void* stream);
/* The PROVE side of the same two proofs (what a party sends in keygen round 1, party_i.rs:219-258); key generation itself
 * (the prime search) is further down: mpe_paillier_keygen / mpe_ntilde_generate.
 * `NiCorrectKeyProof::proof(dk, SALT_STRING)` for EVERY key of a private key set: d_sigma [nkeys][11][64],
 *   sigma_i = rho_i^(N^-1 mod phi(N)) mod N. */
int mpe_correct_key_prove(mpe_ctx* ctx, const mpe_paillier* sk, uint32_t* d_sigma, void* stream);
/* `CompositeDLogProof::prove(DLogStatement{N, g, ni}, secret)` with the sampled r (< 2^512, d_r [batch][16]) as input:
 *   x = g^r mod N, e = H(x, g, N, ni), y = r + e secret.  d_secret [batch][64]; outputs d_x [batch][64], d_y [batch][73]. */
int mpe_composite_dlog_prove(mpe_ctx* ctx, int batch, const uint32_t* d_N, const uint32_t* d_g, const uint32_t* d_ni,
                             const uint32_t* d_secret, const uint32_t* d_r, uint32_t* d_x, uint32_t* d_y, void* stream);
/* Feldman VSS (curv `VerifiableSS`): d_commits [batch][t1][16] (t1 = t + 1 coefficient commitments), d_index [batch]
 * (1-based party index).  validate_share (party_i.rs:337-340): share G == sum_k index^k C_k;
 * get_point_commitment (party_i.rs:383-385): that sum. */
int mpe_vss_validate_share(mpe_ctx* ctx, int batch, int t1, const uint32_t* d_commits, const uint32_t* d_share, const int32_t* d_index,
                           uint8_t* d_ok, void* stream);
int mpe_vss_point_commitment(mpe_ctx* ctx, int batch, int t1, const uint32_t* d_commits, const int32_t* d_index, uint32_t* d_out,
                             void* stream);
/* The two keygen verdicts AS THE REFERENCE COMPOSES THEM, batched over items = (keygen session, prover i): `n_parties` consecutive
 * items form one session, d_ok [batch], d_bad_actors [batch / n_parties] = the reference's `ErrorType::bad_actors` as a bit mask
 * over the provers of the session (may be NULL).
 * mpe_keygen_verify_round1 = `phase1_verify_com_phase3_verify_correct_key_verify_dlog_phase2_distribute` (party_i.rs:260-320):
 *   HashCommitment(y_i, blind_factor) == com  &&  NiCorrectKeyProof::verify(e)  &&  2047 <= e.n.bit_length() <= 2048  &&
 *   2047 <= dlog_statement.N.bit_length() <= 2048 (PAILLIER_MIN/MAX_BIT_LENGTH, party_i.rs:49-50; a wider modulus does not fit the
 *   64-word rows)  &&  composite_dlog_proof_base_h1.verify({N~, h1, h2})  &&  composite_dlog_proof_base_h2.verify({N~, h2, h1}).
 *   Rows: y [16], blind [8], com [8], N [64], sigma [11][64], Nt / h1 / h2 [64], x_h1 / x_h2 [64], y_h1 / y_h2 [73].
 * mpe_keygen_verify_round2 = the verdict of `phase2_verify_vss_construct_keypair_phase3_pok_dlog` (party_i.rs:322-367):
 *   vss_scheme_vec[i].validate_share(share_i, index)  &&  vss_scheme_vec[i].commitments[0] == y_vec[i].
 *   d_commits [batch][t1][16], d_share [batch][8], d_index [batch] (the VERIFIER's 1-based index), d_y [batch][16]. */
typedef struct {
  const uint32_t *y, *blind, *com, *N, *sigma, *Nt, *h1, *h2, *x_h1, *y_h1, *x_h2, *y_h2;
} mpe_keygen_round1;
int mpe_keygen_verify_round1(mpe_ctx* ctx, int batch, int n_parties, const mpe_keygen_round1* in, uint8_t* d_ok, uint32_t* d_bad_actors,
                             void* stream);
int mpe_keygen_verify_round2(mpe_ctx* ctx, int batch, int n_parties, int t1, const uint32_t* d_commits, const uint32_t* d_share,
                             const int32_t* d_index, const uint32_t* d_y, uint8_t* d_ok, uint32_t* d_bad_actors, void* stream);
/* The rest of keygen: dealing, the key pair, and the verdict of round 3.  Sampled values are inputs; all three run on the caller's
 * stream without synchronising it.
 * mpe_vss_share = `VerifiableSS::share(t, n, &u_i)` (the dealing of party_i.rs:260-320), item = one dealer of one session:
 *   d_coef [batch][t1][8]: coef[0] = the secret u_i, coef[1..t] the sampled coefficients, each reduced mod q as read;
 *   d_commits [batch][t1][16] = coef[k] G (comb tables of the generator);  d_shares [batch][n][8], shares[j] = f(j + 1) mod q.
 *   A coefficient that is 0 mod q gives the neutral (all-zero) commitment row: mpe_vss_validate_share refuses every share of such
 *   a sharing, and mpe_keygen_verify_round3 its session (the reference samples non-zero coefficients).
 * mpe_keygen_construct_keypair = the OK branch of `phase2_verify_vss_construct_keypair_phase3_pok_dlog` (party_i.rs:355-363), item =
 *   (session, receiving party): d_shares [batch][n][8] = the n shares that party received, in dealer order, d_y [batch][n][16] = y_vec,
 *   d_nonce [batch][8];  d_x = x_i = sum of the shares mod q, d_ysum = y = sum of y_vec (exact for equal and opposite summands; the
 *   neutral element is the all-zero row), (d_pk, d_R, d_z) = `DLogProof::prove(&x_i)` — the words mpe_dlog_prove gives for (x_i, nonce)
 *   under the context's encoding.  No verdict here: that is mpe_keygen_verify_round2.
 * mpe_keygen_verify_round3 = `Keys::verify_dlog_proofs_check_against_vss` (party_i.rs:405-438), item (s, i) = dealer i's commitments
 *   d_commits [batch][t1][16] and party i's proof (d_pk, d_R [batch][16], d_z [batch][8]); `n_parties` consecutive items form a session:
 *   ok = DLogProof::verify(proof_i) (as mpe_dlog_verify)  &&  xi_commit[s][i] == pk_i,  xi_commit[s][i] = sum_k (i + 1)^k sum_j C[s][j][k]
 *   (`get_commitments_to_xi`, :369-388; the inner sums are formed once per session).  d_bad_actors [batch / n_parties] (may be NULL) as
 *   in rounds 1 and 2; d_xi_commit [batch][16] (may be NULL) receives the commitments.  `y_vec` is only length-checked by the reference
 *   and is no argument.  n_parties <= 32.
 *   DELIBERATE DIVERGENCE: the reference cannot hold a point that is off the curve (curv refuses it when it deserialises).  Here a
 *   commitment row that is no valid point (off the curve, not canonical, or neutral) refuses EVERY item of its session — all n bits of
 *   the mask — and that session's d_xi_commit rows are neutral; an invalid pk or R refuses its own item only. */
int mpe_vss_share(mpe_ctx* ctx, int batch, int t1, int n, const uint32_t* d_coef, uint32_t* d_commits, uint32_t* d_shares, void* stream);
int mpe_keygen_construct_keypair(mpe_ctx* ctx, int batch, int n, const uint32_t* d_shares, const uint32_t* d_y, const uint32_t* d_nonce,
                                 uint32_t* d_x, uint32_t* d_ysum, uint32_t* d_pk, uint32_t* d_R, uint32_t* d_z, void* stream);
int mpe_keygen_verify_round3(mpe_ctx* ctx, int batch, int n_parties, int t1, const uint32_t* d_commits, const uint32_t* d_pk,
                             const uint32_t* d_R, const uint32_t* d_z, uint8_t* d_ok, uint32_t* d_bad_actors, uint32_t* d_xi_commit,
                             void* stream);

/* ---- key MATERIAL: `Keys::create` (party_i.rs:159-177) = `Paillier::keypair()` + `generate_h1_h2_N_tilde()` (:137-156) ----------- */
/* Batched primality verdict for any value in [0, 2^1024): d_n [batch][32], d_ok [batch].  0 for n < 2 and even n > 2; trial division
 * by every odd prime below 6370 (a table prime itself is prime, anything below 6370^2 is decided by the table alone); otherwise
 * `rounds` (1..16) strong-probable-prime (Miller-Rabin) tests.  The bases are FIXED — 2, 3, 5, 7, ... (the first `rounds` primes) —
 * so this serves self-generated candidates and fixtures, NOT adversarially chosen numbers. */
int mpe_is_probable_prime(mpe_ctx* ctx, int batch, const uint32_t* d_n, int rounds, uint8_t* d_ok, void* stream);
/* kzen-paillier `sample_prime` [RECALLED]: attempt a = 0, 1, ... of item g is BigInt::sample(1024) taken from bytes [128 a, 128 a + 128)
 * of the item's ChaCha20 stream (the sampler's stream definition above), with bit 0 and bit 1023 set — fresh draws, no incremental
 * search.  d_out [batch][32] = the candidate of the LOWEST attempt < max_attempts (0 = 16384) that passes mpe_is_probable_prime with
 * 8 rounds, d_attempt [batch] (may be NULL) = that attempt.  DELIBERATE DIVERGENCE from the reference's unbounded loop: an item
 * without such an attempt gets a zero row, attempt -1, and adds 1 to *d_fail (may be NULL).  An item's result depends on neither
 * `batch` nor the other items.  bits must be 1024.  Synchronises the stream (once per pass over the unfinished items). */
int mpe_sample_prime(mpe_ctx* ctx, int batch, const uint8_t* h_seed32, uint64_t stream_id, int bits, int max_attempts, uint32_t* d_out,
                     int32_t* d_attempt, int32_t* d_fail, void* stream);
/* kzen-paillier `sample_safe_prime` [RECALLED]: loop { q = sample_prime(bits); if is_prime((q - 1) / 2) return q } — the key generation
 * the reference recommends "if the code is used in production" (`Keys::create_safe_prime`, party_i.rs:179-199).  Every call of
 * sample_prime goes on with fresh draws, so on the statement above: d_out [batch][32] = the candidate c of the LOWEST attempt
 * < max_attempts (0 = 2^24, the largest value) for which c AND (c - 1) / 2 pass mpe_is_probable_prime with 8 rounds; d_attempt, d_fail,
 * the give-up (zero row, -1, a count; probability ~e^-44 at the default) and the independence of `batch` as for mpe_sample_prime.
 * A result costs ~380 000 attempts (mpe_sample_prime: ~355).  bits must be 1024.  Synchronises the stream once per pass (about
 * 2^safe_pass_log candidates whatever the batch, at most 2^20 attempts of an item; the option changes no result).  Workspace: three
 * survivor lists of min(2^safe_pass_log, batch * 2^20) entries, 192 MB at the default from batch 16 on (12 MB at batch 1);
 * mpe_ntilde_generate_safe_primes reserves it twice. */
int mpe_sample_safe_prime(mpe_ctx* ctx, int batch, const uint8_t* h_seed32, uint64_t stream_id, int bits, int max_attempts, uint32_t* d_out,
                          int32_t* d_attempt, int32_t* d_fail, void* stream);
/* UNSTABLE measurement aid (tools/exp_safe_primes.py reads it; it may change or go without a version step; a context serves one thread
 * at a time, the counters are not synchronised): what the searches of this context have counted so far (the list lengths of their
 * passes); reset != 0 clears them.
 * h_out9 = plain search: attempts sieved, survivors of the sieve, of round 1; safe search: attempts sieved, survivors of the sieve's
 * head, of the whole sieve, of round 1 on c, of round 1 on (c - 1) / 2, of rounds 2..8 on c. */
int mpe_prime_search_counts(mpe_ctx* ctx, int64_t* h_out9, int reset);
/* Field f of these two calls draws stream `counter | f << 56` (counter < 2^56; the convention of mpe_gg20_sample_nonces), item = row:
 * f = 0 p, 1 q, 2 p~, 3 q~, 4 h1, 5 xi.  A failed prime or draw zeroes EVERY output row of that item and adds 1 to *d_fail.
 * `Paillier::keypair()`: d_p, d_q [nkeys][32], d_N [nkeys][64] = p q (as in the reference: no retry for a 2047-bit product or p == q). */
int mpe_paillier_keygen(mpe_ctx* ctx, int nkeys, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_p, uint32_t* d_q,
                        uint32_t* d_N, int32_t* d_fail, void* stream);
/* `Paillier::keypair_safe_primes()`: the same arguments and stream fields 0, 1 as mpe_paillier_keygen, p and q through
 * mpe_sample_safe_prime — the safe key of a (seed, counter) holds the first safe prime of each sequence the plain call walks.  A
 * (seed, counter) pair therefore mints ONE key: use it for the plain call or for this one, never for both (the two keys would be
 * drawn from the same keystream). */
int mpe_paillier_keygen_safe_primes(mpe_ctx* ctx, int nkeys, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_p,
                                    uint32_t* d_q, uint32_t* d_N, int32_t* d_fail, void* stream);
/* `generate_h1_h2_N_tilde()`: N~ = p~ q~, phi = (p~ - 1)(q~ - 1), h1 = sample_below(N~), xi = sample_below(phi) redrawn with fresh
 * bytes (bounded by option sampler_max_attempts) until gcd(xi, phi) = 1, h2 = h1^xi mod N~; outputs xhi = phi - xi and
 * xhi_inv = phi - xi^-1 mod phi (the secrets of the two CompositeDLogProofs).  All rows [count][64]. */
int mpe_ntilde_generate(mpe_ctx* ctx, int count, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_Nt, uint32_t* d_h1,
                        uint32_t* d_h2, uint32_t* d_xhi, uint32_t* d_xhi_inv, int32_t* d_fail, void* stream);
/* `generate_h1_h2_N_tilde()` with the line the reference comments "note, should be safe primes" (party_i.rs:138-139) taken at its
 * word: p~, q~ (fields 2, 3) through mpe_sample_safe_prime; everything behind them is mpe_ntilde_generate's own body. */
int mpe_ntilde_generate_safe_primes(mpe_ctx* ctx, int count, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_Nt,
                                    uint32_t* d_h1, uint32_t* d_h2, uint32_t* d_xhi, uint32_t* d_xhi_inv, int32_t* d_fail, void* stream);

/* ---- Lindell'17 two-party ECDSA, signing ---------------------------------------------- */
/* Party two, `PartialSig::compute(ek, encrypted_secret_share, local_share, ephemeral_local_share,
 * ephemeral_other_public_share, message)` (src/protocols/two_party_ecdsa/lindell_2017/party_two.rs:390-423).
 * pk = party ONE's Paillier key (public part is enough); c_key [batch][128] = Enc(x1); x2, k2, msg [batch][8];
 * R1 [batch][16] = party one's ephemeral public share; rho [batch][16] (< q^2, `BigInt::sample_below(&q.pow(2))`)
 * and r [batch][64] (the randomness `Paillier::encrypt` draws) are inputs.  c3 [batch][128]. */
int mpe_lindell_partial_sig(mpe_ctx* ctx, const mpe_paillier* pk, int batch, const int32_t* d_key_idx,
                            const uint32_t* d_c_key, const uint32_t* d_x2, const uint32_t* d_k2, const uint32_t* d_R1,
                            const uint32_t* d_msg, const uint32_t* d_rho, const uint32_t* d_r, uint32_t* d_c3, void* stream);
/* Party one, `Signature::compute_with_recid(party_one_private, partial_sig_c3, ephemeral_local_share,
 * ephemeral_other_public_share)` (lindell_2017/party_one.rs:519-565).  sk holds p, q; k1 [batch][8]; R2 [batch][16];
 * outputs r, s [batch][8] (s low: min(s, q - s)) and recid [batch]. */
int mpe_lindell_sign(mpe_ctx* ctx, const mpe_paillier* sk, int batch, const int32_t* d_key_idx, const uint32_t* d_c3,
                     const uint32_t* d_k1, const uint32_t* d_R2, uint32_t* d_r, uint32_t* d_s, int32_t* d_recid,
                     void* stream);

/* Key generation, the PDL exchange.  Party one, `pdl_proof(party1_private, paillier_key_pair)` (party_one.rs:366-401):
 * statement {ciphertext = c_key, ek, Q = x1 G, G = generator, h1, h2, N~}, witness {x1, c_key_randomness};
 * sk = party one's key set (private part), stm = its (N~, h1, h2) (create with mpe_statements_create); d_Q [batch][16] out.
 * (`CompositeDLogProof::prove` for (N~, h1, h2) is a host-side muladd + one mpe_modexp.) */
int mpe_lindell_pdl_proof(mpe_ctx* ctx, const mpe_paillier* sk, const mpe_statements* stm, int batch, const int32_t* d_key_idx,
                          const int32_t* d_st_idx, const uint32_t* d_c_key, const uint32_t* d_x1, const uint32_t* d_r,
                          const mpe_pdl_nonces* nonces, uint32_t* d_Q, const mpe_pdl_proof* out, void* stream);
/* Party two, `PaillierPublic::pdl_verify(composite_dlog_proof, statement, proof, paillier_public, q1)` (party_two.rs:275-300):
 * ok = statement.{ek, ciphertext, Q} == (pk[key], c_key, q1)  &&  CompositeDLogProof{x, y}.verify(DLogStatement{N~, h1, h2})
 *      &&  PDLwSlackProof::verify.  Every item brings its own statement: d_Nt, d_h1, d_h2, d_dlog_x [batch][64], d_dlog_y
 * [batch][73], d_stmt_N [batch][64], d_stmt_c / d_c_key [batch][128], d_stmt_Q / d_q1 [batch][16]. */
int mpe_lindell_pdl_verify(mpe_ctx* ctx, const mpe_paillier* pk, int batch, const int32_t* d_key_idx, const uint32_t* d_Nt,
                           const uint32_t* d_h1, const uint32_t* d_h2, const uint32_t* d_dlog_x, const uint32_t* d_dlog_y,
                           const uint32_t* d_stmt_N, const uint32_t* d_stmt_c, const uint32_t* d_stmt_Q, const uint32_t* d_c_key,
                           const uint32_t* d_q1, const mpe_pdl_proof* proof, uint8_t* d_ok, void* stream);

/* ---- Lindell'17, key generation and the ephemeral exchange (lindell_2017/party_one.rs, party_two.rs) ------------------ */
/* Sampled values (secrets, nonces, blind factors) are inputs; scalars [batch][8] are reduced mod q as read, points [batch][16],
 * commitments and blind factors [batch][8].  Every d_ok is [batch], ok[i] = 1 accepts.  The four calls between the
 * commitments run on the caller's stream without synchronising it.
 * `HashCommitment::create_commitment_with_user_defined_randomness(m, blind)` for a 256-bit m [batch][8]: SHA-256 over
 * BigInt::to_bytes(m) | BigInt::to_bytes(blind) — minimal big-endian bytes, leading zero bytes of m dropped, zero as the context's
 * encoding says (mpe_encoding.zero_bytes); the rule mpe_hash_commit_point applies to its blind factor.  (party_two.rs:345-351) */
int mpe_hash_commit_bigint(mpe_ctx* ctx, int batch, const uint32_t* d_m, const uint32_t* d_blind, uint32_t* d_com, void* stream);
/* Party one, `KeyGenFirstMsg::create_commitments_with_fixed_secret_share(x1)` with its witness (party_one.rs:179-219):
 * (d_Q1, d_R, d_z) = DLogProof::prove(x1) — the words mpe_dlog_prove gives for (x1, nonce) —, d_pk_com = Com(Q1; blind_pk),
 * d_pok_com = Com(R; blind_pok), both over the compressed point as mpe_hash_commit_point computes. */
int mpe_lindell_keygen_first_msg(mpe_ctx* ctx, int batch, const uint32_t* d_x1, const uint32_t* d_nonce, const uint32_t* d_blind_pk,
                                 const uint32_t* d_blind_pok, uint32_t* d_Q1, uint32_t* d_R, uint32_t* d_z, uint32_t* d_pk_com,
                                 uint32_t* d_pok_com, void* stream);
/* Party two, `KeyGenSecondMsg::verify_commitments_and_dlog_proof` (party_two.rs:180-223): ok = pk_com == Com(Q1; blind_pk)  &&
 * pok_com == Com(R; blind_pok)  &&  DLogProof::verify (as mpe_dlog_verify).  A Q1 or R that is no valid point (off the curve, not
 * canonical, neutral) refuses the item: the reference cannot hold such a point. */
int mpe_lindell_keygen_verify_first_msg(mpe_ctx* ctx, int batch, const uint32_t* d_pk_com, const uint32_t* d_pok_com,
                                        const uint32_t* d_blind_pk, const uint32_t* d_blind_pok, const uint32_t* d_Q1, const uint32_t* d_R,
                                        const uint32_t* d_z, uint8_t* d_ok, void* stream);
/* Party two, `EphKeyGenFirstMsg::create_commitments` with its witness (party_two.rs:315-371): d_pub = k2 G, d_c = k2 H
 * (H = base_point2), (d_a1, d_a2, d_z) = ECDDHProof::prove over (G, pub, H, c) — the words mpe_ecddh_prove gives for that statement
 * and nonce —, d_pk_com = Com(pub; blind_pk), d_pok_com = Com(Sha256(chain_points([a1, a2])) as a BigInt; blind_pok), the digest NOT
 * reduced mod q and hashed by the rule of mpe_hash_commit_bigint. */
int mpe_lindell_eph_first_msg(mpe_ctx* ctx, int batch, const uint32_t* d_k2, const uint32_t* d_nonce, const uint32_t* d_blind_pk,
                              const uint32_t* d_blind_pok, uint32_t* d_pub, uint32_t* d_c, uint32_t* d_a1, uint32_t* d_a2, uint32_t* d_z,
                              uint32_t* d_pk_com, uint32_t* d_pok_com, void* stream);
/* Party one, `EphKeyGenSecondMsg::verify_commitments_and_dlog_proof` (party_one.rs:437-483): ok = both commitments recomputed as above
 * and equal  &&  ECDDHProof::verify over (G, pub, H, c) (as mpe_ecddh_verify).  An invalid pub, c, a1 or a2 refuses the item. */
int mpe_lindell_eph_verify_first_msg(mpe_ctx* ctx, int batch, const uint32_t* d_pk_com, const uint32_t* d_pok_com, const uint32_t* d_blind_pk,
                                     const uint32_t* d_blind_pok, const uint32_t* d_pub, const uint32_t* d_c, const uint32_t* d_a1,
                                     const uint32_t* d_a2, const uint32_t* d_z, uint8_t* d_ok, void* stream);
/* `party_one::verify(signature, pubkey, message)` (party_one.rs:567-592): d_pub [batch][16], d_msg, d_r, d_s [batch][8].
 * ok = pub is a valid, finite point  &&  1 <= s  &&  s < q - s (so s >= q and high s are refused)  &&
 *      P = (m mod q) s^-1 G + (r mod q) s^-1 pub is finite  &&  r == P.x AS INTEGERS (P.x is not reduced mod q; r is reduced only where
 *      it enters the second scalar).  Where the reference would panic (s = 0, P at infinity) the item is refused. */
int mpe_ecdsa_verify(mpe_ctx* ctx, int batch, const uint32_t* d_pub, const uint32_t* d_msg, const uint32_t* d_r, const uint32_t* d_s,
                     uint8_t* d_ok, void* stream);
/* d_out = a b mod q, rows [batch][8], both factors reduced mod q as read: what `Party1Private::refresh_private_key` (party_one.rs:260-261)
 * and `Party2Private::update_private_key` (party_two.rs:241-246) do to a share, without the share leaving the device. */
int mpe_scalar_mul(mpe_ctx* ctx, int batch, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, void* stream);
/* `party_one::generate_h1_h2_n_tilde()` (party_one.rs:594-607) — NOT the rule of mpe_ntilde_generate: N~ = p~ q~,
 * phi = (p~ - 1)(q~ - 1), h1 = sample_below(phi), xhi = sample_below(2^256), h2 = (h1^-1 mod N~)^xhi mod N~ (a 256-bit ladder).
 * Field f draws stream `counter | f << 56` (counter < 2^56), item = row: f = 6 p~, 7 q~, 14 h1, 15 xhi.  d_Nt, d_h1, d_h2 [count][64],
 * d_xhi [count][8].  An item whose prime search or draw gave up, or whose h1 is no unit modulo N~ (the reference would unwrap() a
 * None), gets zero rows and adds 1 to *d_fail (may be NULL).  Synchronises the stream (the prime search does, once per pass). */
int mpe_lindell_ntilde_generate(mpe_ctx* ctx, int count, const uint8_t* h_seed32, uint64_t counter, int max_attempts, uint32_t* d_Nt,
                                uint32_t* d_h1, uint32_t* d_h2, uint32_t* d_xhi, int32_t* d_fail, void* stream);

/* ---- GG18 signing (src/protocols/multi_party_ecdsa/gg_2018/party_i.rs:384-737, examples/gg18_sign_client.rs) ------------------ */
/* The calls of the reference's ten signing rounds that are not already one call of this header.  Those that are stay that call:
 *   phase1_broadcast (:408-424)                  mpe_hash_commit_point(g_gamma_i, blind)
 *   MessageA::a(k_i, ek, &[]) (client :111)      mpe_paillier_encrypt of k_i zero-extended to [64] words, under the sender's key
 *   verify_proofs_get_alpha (client :226-232)    mpe_mta_verify_get_alpha
 * Conventions.  S <= 8 signers: h_signers [S], HOST array of party indices, ascending; the parties this process plays: h_local
 * [n_local], HOST array of signer ordinals (positions in h_signers), ascending.  Points are [16] words, scalars, commitments and blind
 * factors [8], ciphertexts [128].  Sampled values are inputs; scalars are reduced mod q as read.
 *   broadcast values   sender-major [S][batch][w], own value included
 *   local values       [n_local][batch][w] — with every signer local an output array is the next phase's input array as it stands
 *   per-peer values    [n_local][S-1][batch][w]; peer slot jj of signer ordinal i is ordinal jj (jj < i) or jj + 1
 *   per-session        d_msg [batch][8], d_y [batch][16], d_pk_vec [batch][n][16]
 * d_status [n_local][batch] int32 is written by mpe_gg18_sign_keys and carried through the other calls: the FIRST failure of a
 * (session, party) wins, in the reference's evaluation order, and it sticks; no call stops the batch for one bad item.  A party whose
 * status is not 0 when a call starts, or becomes so inside it, gets all-zero words as that call's outputs (a zero point is no valid
 * point: its peers refuse it with the code of the phase in which they read it).  Every incoming point is checked (on the curve,
 * canonical, not neutral) before a secret is multiplied into it; one that fails refuses the item with the code of its phase.
 *    91  k_i / gamma_i is not a value Scalar::random() returns (zero or >= q)                       party_i.rs:396,402
 *   201  verify_proofs_get_alpha -> InvalidKey                                                      gg_2018/test.rs:265,272
 *   202  the peer's w-side b_proof.pk differs from THAT PEER's g_w entry: the check the comment at   gg_2018/test.rs:274-277
 *        test.rs:274-277 describes (the assert at :278 compares with the receiver's own g_w_i, which is the sender's only with two
 *        signers); gg18_sign_client.rs:235-241 compares as this call does
 *   301  the sum of the deltas is zero (the reference panics: expect("sum of deltas is zero"))      party_i.rs:451
 *   401  phase4 -> InvalidKey                                                                       party_i.rs:481
 *   402  R is the point at infinity (the reference panics: R.x_coord().unwrap())                    party_i.rs:496-497
 *   531  phase5c -> InvalidCom                                                                      party_i.rs:634
 *   541  phase5d -> InvalidCom                                                                      party_i.rs:671
 *   542  phase5d -> InvalidKey                                                                      party_i.rs:668
 *   601  output_signature -> InvalidSig                                                             party_i.rs:709 */
/* `SignKeys::create` (:385-406) with k_i, gamma_i handed in.  d_x_i, d_k_i, d_gamma_i [n_local][batch][8] ->
 * d_w_i = lambda_i x_i (lambda_i = map_share_to_new_params(params, index, s)), d_g_w_i = w_i G, d_g_gamma_i = gamma_i G, and d_g_w
 * [S][batch][16] = lambda_j pk_vec[s_j] of every signer (a pk_vec entry that is no valid point leaves a zero row).  Writes d_status:
 * 0, or 91 with zero outputs. */
int mpe_gg18_sign_keys(mpe_ctx* ctx, int t, int n, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch,
                       const uint32_t* d_x_i, const uint32_t* d_pk_vec, const uint32_t* d_k_i, const uint32_t* d_gamma_i, uint32_t* d_w_i,
                       uint32_t* d_g_w_i, uint32_t* d_g_gamma_i, uint32_t* d_g_w, int32_t* d_status, void* stream);
/* `MessageB::b_with_predefined_randomness(b, ek, m_a, r, beta_tag, &[])` (mta/mod.rs:111-158) with an empty statement set: no range
 * proof is read or checked; everything else is mpe_mta_message_b (flat items, d_key_idx selects Alice's key, same words out). */
int mpe_gg18_message_b(mpe_ctx* ctx, const mpe_paillier* pk, int batch, const int32_t* d_key_idx, const uint32_t* d_b, const uint32_t* d_ca,
                       const uint32_t* d_r, const uint32_t* d_beta_tag, const uint32_t* d_nonce_b, const uint32_t* d_nonce_bt, uint32_t* d_cb,
                       uint32_t* d_beta, const mpe_dlog_proof* b_proof, const mpe_dlog_proof* beta_tag_proof, void* stream);
/* The verdicts of the 2 (S-1) mpe_mta_verify_get_alpha calls in the order of gg18_sign_client.rs:221-244 (per peer: gamma side, w side
 * -> 201; w-side pk == d_g_w of that peer -> 202), then `phase2_delta_i` and `phase2_sigma_i` (:426-444).  Per-peer inputs: d_alpha,
 * d_beta (gamma side: the alphas received, the betas kept), d_miu, d_ni (w side) [..][8], d_ok_gamma, d_ok_w uint8, d_w_pk [..][16]. */
int mpe_gg18_phase2(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_k_i,
                    const uint32_t* d_gamma_i, const uint32_t* d_w_i, const uint32_t* d_alpha, const uint32_t* d_beta, const uint32_t* d_miu,
                    const uint32_t* d_ni, const uint8_t* d_ok_gamma, const uint8_t* d_ok_w, const uint32_t* d_w_pk, const uint32_t* d_g_w,
                    uint32_t* d_delta_i, uint32_t* d_sigma_i, int32_t* d_status, void* stream);
/* `phase3_reconstruct_delta` and `phase4` (:446-483) as gg18_sign_client.rs:272-309 uses them.  d_delta, d_g_gamma, d_blind, d_com:
 * broadcast; d_b_pk: per-peer, the gamma-side b_proof.pk received.  301 when the deltas sum to zero; 401 unless every PEER's
 * b_proof.pk == g_gamma_i and Com(g_gamma_i; blind) == com (the own decommitment is only added); d_R = delta^-1 sum g_gamma_i, 402
 * when that is the neutral point. */
int mpe_gg18_phase4(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_delta,
                    const uint32_t* d_b_pk, const uint32_t* d_g_gamma, const uint32_t* d_blind, const uint32_t* d_com, uint32_t* d_R,
                    int32_t* d_status, void* stream);
/* `phase5_local_sig` and `phase5a_broadcast_5b_zkproof` (:487-559) with l_i, rho_i, the blind factor, the HomoElGamal nonces s1, s2 and
 * the DLog nonce handed in.  d_s_i = m k_i + r sigma_i stays with the caller; V_i = s_i R + l_i G, A_i = rho_i G, B_i = l_i rho_i G;
 * d_com = Com(Sha256(chain_points([V, A, B])) as a BigInt; blind), the digest NOT reduced mod q and hashed by the rule of
 * mpe_hash_commit_bigint; heg = HomoELGamalProof::prove(witness {r: l_i, x: s_i}, statement (G: A_i, H: R, Y: g, D: V_i, E: B_i)) as
 * mpe_heg_prove; dlog = DLogProof::prove(rho_i) as mpe_dlog_prove.  d_status is only read. */
int mpe_gg18_phase5a(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_k_i,
                     const uint32_t* d_sigma_i, const uint32_t* d_msg, const uint32_t* d_R, const uint32_t* d_l_i, const uint32_t* d_rho_i,
                     const uint32_t* d_blind, const uint32_t* d_s1, const uint32_t* d_s2, const uint32_t* d_nonce, uint32_t* d_s_i, uint32_t* d_V,
                     uint32_t* d_A, uint32_t* d_B, uint32_t* d_com, const mpe_heg_proof* heg, const mpe_dlog_proof* dlog, const int32_t* d_status,
                     void* stream);
/* what every signer broadcast in 5A and 5B, each array [S][batch][..]: Phase5ADecom1 {V_i, A_i, B_i, blind_factor}, Phase5Com1 {com},
 * the HomoELGamalProof (T, A3, z1, z2) and the DLogProof of rho_i */
typedef struct { const uint32_t *V, *A, *B, *blind, *com, *T, *A3, *z1, *z2, *dlog_pk, *dlog_R, *dlog_z; } mpe_gg18_phase5b_msgs;
/* `phase5c` (:561-636) per local party over its PEERS' entries of `in` (aligned as gg18_sign_client.rs:381-401): 531 unless every
 * commitment opens, every HomoELGamalProof verifies over (A_j, R, g, V_j, B_j) and every DLogProof verifies.  d_u = rho_i (sum of
 * every V - m G - r y), d_t = l_i (sum of the PEERS' A), d_com2 = Com(Sha256(chain_points([u_i, t_i])) as a BigInt; blind2). */
int mpe_gg18_phase5c(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_msg,
                     const uint32_t* d_y, const uint32_t* d_R, const uint32_t* d_l_i, const uint32_t* d_rho_i, const uint32_t* d_blind2,
                     const mpe_gg18_phase5b_msgs* in, uint32_t* d_u, uint32_t* d_t, uint32_t* d_com2, int32_t* d_status, void* stream);
/* `phase5d` (:638-673) over all S decommitments of 5D (d_u, d_t, d_blind2 against d_com2) and the B_i of 5A: 541 unless every
 * commitment opens, then 542 unless g + sum t_i + sum B_i - sum u_i == g. */
int mpe_gg18_phase5d(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch, const uint32_t* d_u,
                     const uint32_t* d_t, const uint32_t* d_blind2, const uint32_t* d_com2, const uint32_t* d_B, int32_t* d_status, void* stream);
/* `output_signature` with its `verify` (:674-737): s = d_s_own + the peers' rows of d_s_all (broadcast; the own row is not read),
 * r = R.x mod q, recid = R.y & 1; s > q - s: s = q - s, recid ^= 1.  verify accepts iff s != 0 and ((m s^-1) G + (r s^-1) y).x mod q
 * == r — no low-s rule (mpe_ecdsa_verify is Lindell's, another rule).  601 otherwise.  d_r, d_s [n_local][batch][8], d_recid
 * [n_local][batch]: zero unless the status is 0. */
int mpe_gg18_output_signature(mpe_ctx* ctx, int S, const int32_t* h_signers, int n_local, const int32_t* h_local, int batch,
                              const uint32_t* d_s_own, const uint32_t* d_s_all, const uint32_t* d_R, const uint32_t* d_msg, const uint32_t* d_y,
                              uint32_t* d_r, uint32_t* d_s, int32_t* d_recid, int32_t* d_status, void* stream);

/* Kernel geometry chosen for the last launch (for bench.py's roofline accounting). */
typedef struct {
  int waves;              /* workgroups (= waves) launched */
  int ints_per_wave;      /* big integers processed concurrently by one wave */
  int limbs;              /* internal limbs per integer (K) */
  int limb_bits;          /* internal radix (W) */
  int lds_bytes_per_wave;
  size_t table_scratch_bytes;
} mpe_launch_info;
int mpe_last_launch_info(const mpe_ctx* ctx, mpe_launch_info* out);

/* Per-launch timing of the heavy kernels with HIP events recorded on the launch stream (used by
 * bench.py for the roofline line).  kind: 0 = modexp kernel (bits = modulus width), 1 = modmul kernel, 3 = N-adic pair kernel
 * (bits = width of the SQUARE: 4096 for N^2, 2048 for p^2 | q^2), 4 = the pair kernel in `half` mode (plain Montgomery ladder
 * modulo N or p; bits = that width), 5 = fixed-base ladder modulo N~ (exp2_words = the table's window width in bits),
 * 6 = the pair kernel with a PUBLIC exponent (the key N): items ordered by key, sliding windows wherever a wave shares it. */
typedef struct {
  int kind; int bits; int exp_words; int batch; float ms;
  int exp2_words;       /* != 0: mpe_modexp2-style launch (two bases on one ladder) */
  float sliding_frac;   /* kind 6: the share of the launch's (wave, trip) pairs that really ran the sliding-window schedule, counted by
                         * the kernel (waves that straddle a key boundary, and two-base ladders whose first window would dip below
                         * the second exponent, keep fixed windows); 0 for the other kinds; -1 = not counted */
} mpe_prof_rec;
int mpe_prof_enable(mpe_ctx* ctx, int on);       /* clears earlier records */
int mpe_prof_collect(mpe_ctx* ctx, mpe_prof_rec* out, int max_records, int* n_out);  /* waits for the events */

#ifdef __cplusplus
}
#endif
#endif /* MPECDSA_HIP_H */
