/*
 * hipbls — MI355X (gfx950) BLS12-381 engine behind charon's tbls.Implementation.
 *
 * C-ABI only: plain pointers and sizes, no HIP or torch types.  All buffers are owned by the
 * caller; the library never keeps a caller pointer after a call returns (cgo pointer rules).
 * One process drives every GPU of the node (charon is one process per node: app/app.go:127 wires all components
 * through the one global tbls implementation, tbls/tbls.go:11-14): the library keeps a context per device it was
 * given (hipbls_init_devices) and splits every host-buffer batch into contiguous ranges -- whole validators /
 * message runs -- across them, writing each range's results straight into the caller's arrays.  Every entry point
 * is thread-safe and binds the right device on the calling thread (cgo goroutines move between OS threads).  Calls
 * that share a device workspace are ordered on the device even when they are issued on different streams.  A HIP
 * failure is reported as HIPBLS_ERR_DEVICE for the whole call and NEVER as a per-item "verified".
 *
 * Reference interface each entry point replaces (paths relative to the charon repository):
 *   hipbls_verify                      tbls.Implementation.Verify (one item, coalesced by the submission queue)
 *                                      tbls/tbls.go:53-55, tbls/herumi.go:285-301
 *   hipbls_verify_batch                tbls.Implementation.Verify            tbls/tbls.go:53-55, tbls/herumi.go:285-301
 *   hipbls_verify_signed_data_batch    eth2util/signing.Verify (signing root + zero-signature check + tbls.Verify)
 *                                      eth2util/signing/signing.go:57-69, 88-107
 *   hipbls_threshold_aggregate_batch   tbls.Implementation.ThresholdAggregate tbls/tbls.go:50-51, tbls/herumi.go:244-283
 *   hipbls_sign_batch                  tbls.Implementation.Sign              tbls/tbls.go:57-59, tbls/herumi.go:303-313
 *   hipbls_secret_to_public_key_batch  tbls.Implementation.SecretToPublicKey tbls/tbls.go:36-38, tbls/herumi.go:67-80
 *   hipbls_sign_batch_ct, hipbls_secret_to_public_key_batch_ct: the same two for real secrets, secret-independent
 *   hipbls_verify_aggregate[_batch]    tbls.Implementation.VerifyAggregate   tbls/tbls.go:61-63, tbls/herumi.go:315-339
 *   hipbls_aggregate                   tbls.Implementation.Aggregate         tbls/tbls.go:65-67, tbls/herumi.go:220-242
 *   hipbls_threshold_split             tbls.Implementation.ThresholdSplit[Insecure] tbls/tbls.go:40-47, tbls/herumi.go:84-181
 *   hipbls_recover_secret              tbls.Implementation.RecoverSecret     tbls/tbls.go:49, tbls/herumi.go:183-218
 *   hipbls_threshold_split_batch_ct, hipbls_recover_secret_batch_ct: the same two for many validators in one call, with
 *                                      the public keys their callers ask for next (dkg/keycast.go:156-179,
 *                                      cmd/combine/combine.go:106-119); the two single calls are one-validator calls of them
 *   hipbls_pubshare_table_load         the pubshare set charon builds from the cluster lock at startup
 *                                      (app/app.go:343-381, core/parsigex/parsigex.go:139-163 lookup)
 *   hipbls_verify_batch_keys           tbls.Verify with that pubshare (tbls/herumi.go:285-301)
 *   hipbls_batch_verify_rlc            many tbls.Verify calls at once: the per-item loops of
 *                                      core/parsigex/parsigex.go:139-163, core/validatorapi/validatorapi.go:246-283,
 *                                      core/sigagg/sigagg.go:138-159 (optional BatchVerifier extension)
 * Underneath, these replace herumi's cgo entry points blsVerify / blsSignatureRecover /
 * blsSign / blsGetPublicKey / blsFastAggregateVerify / blsAggregateSignature
 * (github.com/herumi/bls-eth-go-binary v1.32.1, imported at tbls/herumi.go:12).
 *
 * Wire formats (herumi ETH mode): secret key 32 bytes big-endian; public key 48-byte compressed G1;
 * signature 96-byte compressed G2 (x = c1 || c0), ZCash flag bits.
 */
#ifndef HIPBLS_H
#define HIPBLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-item and per-call status codes.  1..5 map onto the reference's error strings. */
enum {
  HIPBLS_OK = 0,
  HIPBLS_ERR_PUBKEY = 1,    /* "cannot set compressed public key in Herumi format" */
  HIPBLS_ERR_SIGNATURE = 2, /* "cannot unmarshal signature into Herumi signature" */
  HIPBLS_ERR_VERIFY = 3,    /* "signature not verified" (Verify) / "signature verification failed" (VerifyAggregate) */
  HIPBLS_ERR_SECRET = 4,    /* "cannot unmarshal secret into Herumi secret key" / "cannot obtain public key from secret" */
  HIPBLS_ERR_COMBINE = 5,   /* "cannot combine signatures" (empty set, id 0, duplicate id) */
  HIPBLS_ERR_ZERO_SIG = 6,  /* eth2util/signing.Verify: "no signature found" (all-zero signature, signing.go:99-102) */
  HIPBLS_ERR_ARG = 16,      /* bad arguments (null pointer, size overflow) */
  HIPBLS_ERR_DEVICE = 17    /* HIP runtime failure; see hipbls_last_error() */
};

/* Library/ABI version (bumped on any signature change). */
#define HIPBLS_ABI_VERSION 12
int hipbls_abi_version(void);

/* Bind the library to the n devices ids[0..n) (n <= 64; a device may repeat: each entry is one context, e.g. to
 * test the range split on one GPU).  Host-buffer batches are split across them; each device holds its own copy of
 * the pubshare table and its own H(m) cache and submission queue.  Idempotent for the same list; a different list
 * after the first bind is HIPBLS_ERR_ARG.  Without any init call the first entry point binds the devices named by
 * the environment variable HIPBLS_DEVICES ("all" or "0,1,2") or else the calling thread's current device. */
int hipbls_init_devices(const int32_t* ids, uint32_t n);
/* hipbls_init_devices(&device, 1); device < 0: device 0, or the existing binding. */
int hipbls_init(int device);
/* Number of device contexts (0 before the first bind); their device ids in ids[0..min(n, cap)). */
int hipbls_device_slots(int32_t* ids, uint32_t cap);
/* The split planner the batch entry points use (no GPU needed): bounds[0] = 0 <= ... <= bounds[parts] = n, equal
 * shares; with run_keys (e.g. each item's message index) an inner bound moves forward to the next change of key, by
 * at most half a share, so a validator's partials stay on one device. */
int hipbls_plan_ranges(uint64_t n, uint32_t parts, const uint32_t* run_keys, uint64_t* bounds);
/* Number of visible HIP devices (0 when none). */
int hipbls_device_count(void);
/* Streams the library created on `device` (its library stream, two fork sub-streams and the submission queue's
 * stream), shared by every context bound to that device: at most 4 whatever the number of contexts, so the library's
 * launches never need more than GPU_MAX_HW_QUEUES hardware queues.  0 for a device without a context. */
int hipbls_device_streams(int device);
/* Scratch budget of `device`.  Each hardware queue that runs the library's kernels holds a scratch
 * block of per_lane (the deepest kernel's private segment) x 64 lanes x 32 wave slots x CUs, rounded to 2 MiB
 * (*per_queue); all of a process's queues on the device share one region of *limit bytes (the HSA agent's scratch
 * limit, 32 GiB on MI355X; 0 = not reported), and *queues is GPU_MAX_HW_QUEUES (HIP's normal-priority queues per
 * process).  The library holds 4 queues (hipbls_device_streams), reserves their blocks at init (HIPBLS_SCRATCH_RESERVE=0
 * skips it), refuses a device where they do not fit (hipbls_init* -> HIPBLS_ERR_DEVICE), and never launches on a
 * stream that would take another queue: a *_device call on a priority or CU-masked stream (or on any caller stream when
 * *queues blocks would not fit) runs on the library stream, ordered after the caller's stream and before its later
 * work (hipbls_stream_joins counts those calls).  So (*limit - 4 x *per_queue) is what other queues of the process
 * may still hold.  HIPBLS_ERR_ARG for a device without a context. */
int hipbls_scratch_budget(int device, uint64_t* per_lane, uint64_t* per_queue, uint64_t* limit, uint32_t* queues);
int hipbls_stream_joins(uint64_t* calls);
/* Space-separated names of every kernel the library can launch (no GPU needed; the scratch budget's kernel set). */
const char* hipbls_kernel_names(void);
/* Thread-local text of the last HIPBLS_ERR_DEVICE / HIPBLS_ERR_ARG (and, after an init on a runtime without a
 * scratch-limit query, the note that every *_device call runs on the library's streams). */
const char* hipbls_last_error(void);
/* "src=<sha256> flags=<sha256>": digests of the sources and compile flags the library was built from
 * (charon_amd/build.py); smoke(), the GPU test session and bench.py compare them with the shipped sources. */
const char* hipbls_build_id(void);
/* Device index the library is bound to (-1 before the first call). */
int hipbls_current_device(void);
/* Per-kernel HIP-event timing (hipbls_kernel_timing); off by default, or HIPBLS_TIMING=1 in the environment. */
int hipbls_set_timing(int enabled);
/* Pairing-check layout.  HIPBLS_PAIR_SINGLE: one lane per check.  HIPBLS_PAIR_LANES: a lane pair per check (the
 * two Miller loops side by side, the final exponentiation split across the pair; about half the latency, twice
 * the lanes).  HIPBLS_PAIR_QUADS: four lanes per Verify-shaped check (each Miller loop split across a lane pair,
 * the two pairs side by side; RLC windows keep lane pairs).  HIPBLS_PAIR_OCTETS: eight lanes per Verify (the quad
 * layout with every Fp2 product and square split across twin lanes, charon_amd/csrc/verify_lat.hip: the drop-in
 * n = 1 latency path; other checks as QUADS).  HIPBLS_PAIR_AUTO (default): the widest layout the batch leaves
 * lanes for (Verify: octets up to 4,096 items, quads up to the quad limit, then pairs up to 32,768 items; RLC
 * sub-batches up to 32,768 windows, every RLC fallback list and FastAggregateVerify on pairs).  AUTO alone also
 * takes the lone sigagg route: a threshold-aggregate(-verify) call of at most 4 groups and 64 partials runs its keys,
 * hashes and partials on octets and its check on sixteen lanes; every forced mode keeps the
 * throughput kernels, HIPBLS_LAT_HEX=0 turns the sixteen-lane paths off, HIPBLS_LAT_SIGAGG=0 this route alone.
 * Results are identical in every mode.  Returns the previous mode, or HIPBLS_ERR_ARG for an unknown one.  The environment
 * variable HIPBLS_PAIR_MODE (0-4) sets the initial mode. */
enum { HIPBLS_PAIR_AUTO = 0, HIPBLS_PAIR_SINGLE = 1, HIPBLS_PAIR_LANES = 2, HIPBLS_PAIR_QUADS = 3,
       HIPBLS_PAIR_OCTETS = 4 };
int hipbls_set_pair_mode(int mode);
/* Replicas of a Verify batch of at most 8 items on octets (the drop-in n = 1 path): that many copies of its one
 * workgroup race, one per XCD, and the first to finish each stage wins (the others end early); the results are the
 * same.  A single wave's check time varies 7.2-9.8 ms with where it runs.  Default 8
 * (HIPBLS_LAT_REPLICAS); 1 turns it off.  Returns the previous value, HIPBLS_ERR_ARG outside 1-32. */
int hipbls_set_latency_replicas(uint32_t replicas);

/* ------------------------------------------------ single-item Verify through the submission queue ---- */
/* tbls.Verify for one item.  Concurrent callers (any thread) are coalesced into one kernel launch per batch:
 * while a batch runs on the GPU the next one fills, so the batch size follows the offered load; an idle queue
 * waits gather_us for company.  *status as hipbls_verify_batch.  The queue has its own stream and buffers and
 * no lock is held while the GPU runs. */
int hipbls_verify(const uint8_t* pk48, const uint8_t* msg, uint64_t msg_len, const uint8_t* sig96, int32_t* status);
/* Asynchronous form: submit returns a ticket; wait blocks until that item's batch completed (each ticket once). */
int hipbls_verify_submit(const uint8_t* pk48, const uint8_t* msg, uint64_t msg_len, const uint8_t* sig96,
                         uint64_t* ticket);
int hipbls_verify_wait(uint64_t ticket, int32_t* status);
/* Queue policy (defaults 65,536 items, 50 us) and counters (batches launched, items verified), summed over the
 * devices.  An item goes to the device its message hashes to, so the partials of one signing root meet in one
 * batch.  A batch of >= 8 items whose keys are all in the resident pubshare table runs as an RLC BatchVerify with
 * keys by index over its distinct messages, through the H(m) cache (statuses unchanged); the number of batches
 * that took this keyed path is hipbls_queue_keyed_batches.  With the H(m) cache enabled, keyed batches below 8
 * items (a serial caller's lone Verify) run keyed too and count the same way, but on hipbls_verify_batch_keys'
 * latency route instead of an RLC check: octets / sixteen lanes, H(m) from the cache, a miss inserted
 * (HIPBLS_LAT_VERIFY_KEYS=0: the RLC path as before). */
int hipbls_queue_config(uint64_t max_batch, uint32_t gather_us);
int hipbls_queue_stats(uint64_t* batches, uint64_t* items);
int hipbls_queue_keyed_batches(uint64_t* batches);
/* Completion polls of the queue workers (a batch in flight is polled every 20 us from 85 % of the running estimate
 * of its time on) and wire batches collected, summed over the devices. */
int hipbls_queue_worker_stats(uint64_t* wakeups, uint64_t* batches);

/* ---------------------------------------------------------------- batched, host buffers ---- */

/* Verify n items: item i is (pks[48 i..], msgs[msg_offsets[i] .. msg_offsets[i+1]), sigs[96 i..]).
 * status[i] = HIPBLS_OK | HIPBLS_ERR_PUBKEY | HIPBLS_ERR_SIGNATURE | HIPBLS_ERR_VERIFY,
 * exactly the outcome tbls.Herumi.Verify returns for that item. */
int hipbls_verify_batch(const uint8_t* pks, const uint8_t* msgs, const uint64_t* msg_offsets,
                        const uint8_t* sigs, uint64_t n, int32_t* status);

/* eth2util/signing.Verify for n items: the signing root SHA-256(object_root || domain) (SSZ SigningData) is
 * computed on the GPU from object_roots[32 i ..] and domains[32 i ..]; status[i] as hipbls_verify_batch, or
 * HIPBLS_ERR_ZERO_SIG for an all-zero signature. */
int hipbls_verify_signed_data_batch(const uint8_t* pks, const uint8_t* object_roots, const uint8_t* domains,
                                    const uint8_t* sigs, uint64_t n, int32_t* status);

/* ThresholdAggregate for n_groups sets: group g holds partials
 * sigs[96 k ..], share_idx[k] for k in [group_offsets[g], group_offsets[g+1]).
 * out_sigs[96 g ..] = sum_k lambda_k(0) * sig_k: Lagrange at 0 over the share indices taken as Fr elements the
 * way herumi parses strconv.Itoa(idx) (tbls/herumi.go:264-271): a signed Go int reduced mod r, so -k is r - k.
 * status[g] = HIPBLS_OK | HIPBLS_ERR_SIGNATURE | HIPBLS_ERR_COMBINE (empty set, id = 0, duplicate id).
 * A lone call (at most 4 groups and 64 partials, HIPBLS_PAIR_AUTO) takes the latency route: one octet of lanes per
 * partial, then per group the sum and [L^-1] S on an octet (kernels timed as tv_prep8, tagg_sum8).
 * Same bytes and statuses. */
int hipbls_threshold_aggregate_batch(const uint8_t* sigs, const int64_t* share_idx,
                                     const uint64_t* group_offsets, uint64_t n_groups,
                                     uint8_t* out_sigs, int32_t* status);

/* Sign n messages: out_sigs[96 i ..] = sks[32 i ..] * H(msg_i).  status[i] = OK | ERR_SECRET. */
int hipbls_sign_batch(const uint8_t* sks, const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t n,
                      uint8_t* out_sigs, int32_t* status);

/* out_pks[48 i ..] = sks[32 i ..] * g1.  status[i] = OK | ERR_SECRET (zero or >= r). */
int hipbls_secret_to_public_key_batch(const uint8_t* sks, uint64_t n, uint8_t* out_pks, int32_t* status);

/* hipbls_sign_batch for real secrets (tbls.Implementation.Sign, tbls/herumi.go:303-313): same arguments, bytes,
 * statuses and argument errors, computed by kernels whose instruction stream and memory addresses do not depend on
 * sks.  The public messages are hashed by one kernel (timed as sign_ct_hash); the only kernel that
 * reads the secrets (sign_ct_mul) computes [sk] H(m) with 64 x (double, full scan of a 16-entry table, unconditional
 * addition, select by mask) and compresses with the sign flag and the infinity encoding chosen by mask.  A secret
 * >= r runs the same stream and yields ERR_SECRET with a zero-filled output.  The device copy of sks is zeroed on the
 * call's stream before the call returns.  hipbls_sign_batch stays the variable-time generator for test and bench
 * data. */
int hipbls_sign_batch_ct(const uint8_t* sks, const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t n,
                         uint8_t* out_sigs, int32_t* status);

/* hipbls_secret_to_public_key_batch for real secrets (tbls.Implementation.SecretToPublicKey, tbls/herumi.go:67-80):
 * same arguments, bytes and statuses (ERR_SECRET for zero or >= r), by a fixed 4-bit window over [0..15] g1 read by a
 * full scan (kernel timed as sk_to_pk_ct).  The device copy of sks is zeroed before the call returns. */
int hipbls_secret_to_public_key_batch_ct(const uint8_t* sks, uint64_t n, uint8_t* out_pks, int32_t* status);

/* FastAggregateVerify(pks[0..n), sig, msg).  *status = OK | ERR_PUBKEY | ERR_SIGNATURE | ERR_VERIFY. */
int hipbls_verify_aggregate(const uint8_t* pks, uint64_t n, const uint8_t* sig, const uint8_t* msg,
                            uint64_t msg_len, int32_t* status);

/* n_groups FastAggregateVerify calls in one launch: group g checks sigs[96 g ..] over message
 * msgs[msg_offsets[g] .. msg_offsets[g+1]) against the keys pks[48 k ..], k in
 * [key_offsets[g], key_offsets[g+1]).  status[g] as hipbls_verify_aggregate.  Sync-committee and
 * cluster-lock checks (cluster/lock.go:178,267) batch this way. */
int hipbls_verify_aggregate_batch(const uint8_t* pks, const uint64_t* key_offsets, uint64_t n_groups,
                                  const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_offsets,
                                  int32_t* status);

/* hipbls_verify_aggregate_batch with key k of the call = table[key_idx[k]] (hipbls_pubshare_table_load): group g checks
 * sigs[96 g ..] over message g against the keys table[key_idx[k]], k in [key_offsets[g], key_offsets[g+1]).  status[g]
 * is exactly what the wire-format call returns for the same key bytes, in every pair mode: the signature's encoding or
 * G2-membership error first, then a table entry that failed to load (HIPBLS_ERR_PUBKEY), then HIPBLS_ERR_VERIFY (also
 * for an empty group, the identity key, a key sum at infinity).  No key is decompressed or subgroup-tested: the table
 * load did that once.  The groups' messages are folded to the distinct ones, and each of those is looked up in the
 * context's H(m) cache (hipbls_hcache_config; counted per distinct message in hipbls_hcache_stats): a hit is read from
 * its column, a miss is hashed once into a table of the call's own, also with the cache disabled or smaller than the
 * call's distinct messages.  The call only reads the cache (FastAggregateVerify is the last consumer of a root): it
 * never inserts or evicts.  HIPBLS_ERR_ARG for the whole call, before anything is launched, when a key index is outside
 * the table.  Routes as the wire-format call's: at most 16 groups in AUTO pair mode are timed as "fav_prep8_keys" +
 * "fav_lq16_keys", anything else as "rlc_hash" (the missing hashes) + "fav_keys".  A group of more than 2,048 keys
 * (the cluster lock's aggregate over every pubshare) is cut into slices of that many keys, each summed by a workgroup
 * of its own ("fav_sum_keys") before the check adds the partial sums; the environment variable HIPBLS_FAV_SUM_SPLIT,
 * read at init, overrides the threshold, 0 turns the split off.  Statuses do not depend on it. */
int hipbls_verify_aggregate_batch_keys(const uint32_t* key_idx, const uint64_t* key_offsets, uint64_t n_groups,
                                       const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_offsets,
                                       int32_t* status);

/* herumi's Deserialize of n points, one status each: kind 1 = 48-byte public keys (OK | ERR_PUBKEY), kind 2 = 96-byte
 * signatures (OK | ERR_SIGNATURE); flags, x < p, on the curve, in the subgroup (the point at infinity deserializes).
 * The Go binding uses it to name the failing item in Aggregate / ThresholdAggregate errors, the
 * z.Int("signature_number", idx) field of tbls/herumi.go:229-233, 255-258. */
int hipbls_deserialize_status(const uint8_t* data, uint64_t n, int32_t kind, int32_t* status);

/* Plain G2 sum of n signatures (decoded in parallel, tree-summed).  *status = OK | ERR_SIGNATURE.  As herumi
 * (tbls/herumi.go:220-242), n == 0 is not an error: the sum is the point at infinity, 0xc0 || 0^95. */
int hipbls_aggregate(const uint8_t* sigs, uint64_t n, uint8_t* out_sig, int32_t* status);

/* Shamir split: share_i = secret + sum_j poly_tail[j] * i^(j+1) mod r, i = 1..total.
 * poly_tail holds threshold-1 secrets of 32 bytes (the reference draws them from a CSPRNG or an
 * insecure reader; the caller supplies them).  *status = OK | ERR_SECRET.  A one-validator call of
 * hipbls_threshold_split_batch_ct without public keys. */
int hipbls_threshold_split(const uint8_t* secret, const uint8_t* poly_tail, uint32_t total, uint32_t threshold,
                           uint8_t* out_shares, int32_t* status);

/* Lagrange recovery of the secret at 0 from n (id, share) pairs; ids as in ThresholdAggregate (int mod r).
 * *status = OK | ERR_SECRET | ERR_COMBINE.  A one-group call of hipbls_recover_secret_batch_ct. */
int hipbls_recover_secret(const uint8_t* shares, const int64_t* ids, uint32_t n, uint8_t* out_secret,
                          int32_t* status);

/* Deal n_val validators in one call, on kernels whose instruction stream and memory addresses do not depend on the
 * secrets.  Validator v has secret secrets[32 v ..] and polynomial tail
 * poly_tails[32 (threshold-1) v ..] (threshold-1 coefficients).
 * out_shares[32 (total v + i-1) ..] = f_v(i), i = 1..total: exactly hipbls_threshold_split's bytes.
 * status[v] = OK | ERR_SECRET (the secret or any coefficient >= r: every output of that validator is zero bytes).
 * out_pubs / pub_status (both null, or both given): entry v (total+1) + k is [f_v(k)] g1 compressed, k = 0 the
 * root key, k = 1..total the pubshares, with exactly hipbls_secret_to_public_key_batch_ct's bytes and status for
 * that scalar (ERR_SECRET and zero bytes for a zero scalar, and for every entry of a validator whose status[v]
 * is ERR_SECRET).  One kernel (timed as deal_ct), one lane per (v, k): Horner over the public threshold, then
 * [f_v(k)] g1 by 64 mixed additions over a fixed-base comb of g1 that each context builds once, at first use (timed as
 * g1_comb_build, on the library's stream; calls are ordered behind it by a stream wait, never a host wait).
 * n_val == 0 is OK; threshold == 0, total == 0, a null tail with
 * threshold > 1, only one of out_pubs / pub_status, or n_val (total+1) >= 2^31 is HIPBLS_ERR_ARG.  Validators are
 * split over the contexts whole.  The device copies of secrets, tails and shares are zeroed on the call's stream before
 * the call returns. */
int hipbls_threshold_split_batch_ct(const uint8_t* secrets, const uint8_t* poly_tails, uint64_t n_val,
                                    uint32_t total, uint32_t threshold, uint8_t* out_shares, int32_t* status,
                                    uint8_t* out_pubs, int32_t* pub_status);

/* Recover n_groups secrets in one call, secret-independent as above (kernel timed as recover_ct, one lane per group).
 * Group g: shares[32 k ..], ids[k] for k in [group_offsets[g], group_offsets[g+1]); ids as hipbls_recover_secret.
 * status[g] = OK | ERR_COMBINE (empty, id 0, duplicate id: public, decided first) | ERR_SECRET (a share >= r).
 * out_secrets[32 g ..] as hipbls_recover_secret (zero bytes on error).
 * out_pubkeys / pk_status (both null or both given): [secret_g] g1 as above (ERR_SECRET and zero bytes for a group
 * that failed or a zero secret).  The ids and the group sizes are public: the Lagrange coefficients are computed from
 * them by variable-time code, and every lane runs as many steps as the call's largest group has shares.  n_groups == 0
 * is OK; n_groups or the share count >= 2^31 is HIPBLS_ERR_ARG.  Groups are split over the contexts whole; the device
 * copies of the shares and of the recovered secrets are zeroed before the call returns. */
int hipbls_recover_secret_batch_ct(const uint8_t* shares, const int64_t* ids, const uint64_t* group_offsets,
                                   uint64_t n_groups, uint8_t* out_secrets, int32_t* status,
                                   uint8_t* out_pubkeys, int32_t* pk_status);

/* herumi blsPublicKeyShare, for many validators and many ids, with joint dealings (public data only).
 * Coefficient j of validator v is  A[v][j] = sum over d < n_dealers of C[v][d][j],
 * C[v][d][j] = commitments[48 ((v n_dealers + d) threshold + j) ..] (compressed G1, decoded with the subgroup test).
 * out_pubs[48 (v n_ids + i) ..] = sum_j [x_i^j] A[v][j],  x_i = ids[i] mod r (ids as in ThresholdAggregate).
 * status[v] = OK | ERR_PUBKEY (any commitment of v does not decode: all n_ids outputs of v are zero bytes).
 * Evaluation ids: one list, shared by every validator of the call (the cluster's operator indices).  Duplicate ids
 * are allowed (the same output twice).  An id that is 0 mod r is allowed: its output is A[v][0], the validator's group
 * public key -- a joint dealing's root key without host arithmetic.  Negative ids and INT64_MIN work:
 * [x] P = -[|x|] P with |x| <= 2^63.
 * Infinity: a commitment with the valid infinity encoding (0xc0 then 47 zero bytes) is the identity and takes part in
 * the arithmetic (a polynomial whose top coefficient is 0 is a legal dealing); an output that is the identity is
 * written as that encoding with status OK -- the caller decides what an identity key means.
 * n_val == 0 is OK.  HIPBLS_ERR_ARG: threshold == 0, n_dealers == 0, n_ids == 0, a null pointer with a non-zero
 * count, threshold > 65,535, or n_val, n_ids, n_val n_ids or n_val n_dealers threshold >= 2^31.  Validators are split
 * over the contexts whole.  Kernels: one lane per commitment (timed as g1_decode), for n_dealers > 1 one lane per
 * (v, j) (vss_dealer_sum), one lane per (v, i) (vss_eval); every addition is the complete one. */
int hipbls_public_key_share_batch(const uint8_t* commitments, uint64_t n_val, uint32_t n_dealers, uint32_t threshold,
                                  const int64_t* ids, uint32_t n_ids, uint8_t* out_pubs, int32_t* status);

/* herumi blsPublicKeyRecover for many groups.  Group g: pubshares[48 k ..], ids[k] for k in
 * [group_offsets[g], group_offsets[g+1]).  out_pubkeys[48 g ..] = sum_k lambda_k P_k (Lagrange at 0).
 * status[g] = OK | ERR_COMBINE (empty group, id = 0 mod r, duplicate id: decided first, as
 * hipbls_recover_secret_batch_ct does) | ERR_PUBKEY (a pubshare does not decode).  Zero bytes on error.
 * Infinity: a pubshare with the valid infinity encoding is the identity and takes part; an identity result is written
 * as 0xc0 then 47 zero bytes with status OK.  n_groups == 0 is OK; a null pointer with a non-zero count, or n_groups
 * or the pubshare count >= 2^31, is HIPBLS_ERR_ARG.  Groups are split over the contexts whole.  Kernels: one lane per
 * pubshare (vss_scale: decode, then the short integer multiple of ThresholdAggregate's small-id path or the full
 * Lagrange coefficient off it), one lane per group (vss_sum). */
int hipbls_public_key_recover_batch(const uint8_t* pubshares, const int64_t* ids, const uint64_t* group_offsets,
                                    uint64_t n_groups, uint8_t* out_pubkeys, int32_t* status);

/* One round of a joint-Feldman dealing in batches over all validators of a ceremony, secret-independent as the split
 * above: a dealer's shares with their Feldman commitments, a receiver's check of the shares it was
 * sent, and the sum of the qualified dealers' shares.
 *
 * hipbls_deal_commit_batch_ct: inputs, out_shares and status exactly as hipbls_threshold_split_batch_ct (its kernel,
 * timed as deal_ct, without public keys), then one lane per (v, j), j = 0..threshold-1 (timed as commit_ct):
 * out_commitments[48 (v threshold + j) ..] = [a_j] g1 compressed, a_0 the secret, a_j = poly_tails' coefficient j-1,
 * by 64 mixed additions over the context's comb: the layout hipbls_public_key_share_batch reads with n_dealers = 1.
 * com_status[v threshold + j] = OK | ERR_SECRET.  A zero coefficient gives the infinity encoding (0xc0 then 47 zero
 * bytes) with status OK (a legal dealing, as the share call reads it); a validator whose status[v] is ERR_SECRET gives
 * zero bytes and ERR_SECRET for all its commitments.  n_val == 0 is OK; HIPBLS_ERR_ARG as the split, and for a null
 * out_commitments or com_status, threshold > 65,535 or n_val threshold >= 2^31.  Validators are split over the
 * contexts whole; the device copies of secrets, tails and shares are zeroed on the call's stream before the call
 * returns. */
int hipbls_deal_commit_batch_ct(const uint8_t* secrets, const uint8_t* poly_tails, uint64_t n_val, uint32_t total,
                                uint32_t threshold, uint8_t* out_shares, int32_t* status, uint8_t* out_commitments,
                                int32_t* com_status);

/* The receiver's check.  shares[32 (v n_dealers + d) ..] is the share dealer d sent for validator v; commitments in
 * hipbls_public_key_share_batch's layout, C[v][d][j] = commitments[48 ((v n_dealers + d) threshold + j) ..].
 * status[v n_dealers + d], decided in this order: ERR_PUBKEY (a commitment of (v, d) does not decode: public),
 * ERR_SECRET (the share >= r), ERR_VERIFY ([share] g1 != sum_j [my_id^j] C[v][d][j]), OK.  The verdict is public (a
 * complaint is broadcast); nothing else about a share steers control flow or addresses.  A zero share is compared as
 * the infinity encoding, not rejected.  my_id follows the share call's rule for ids: negative values and INT64_MIN
 * work, and 0 evaluates at C[v][d][0].  Kernels: each (v, d) as a one-dealer validator of the share call evaluated at
 * my_id (g1_decode, vss_eval), then one lane per (v, d) on the same stream (share_check_ct): [share] g1 over the comb,
 * compressed, and compared with the expected 48 bytes on the device by an OR of XORs.  n_val == 0 is OK;
 * HIPBLS_ERR_ARG: threshold == 0, n_dealers == 0, a null pointer with a non-zero count, threshold > 65,535, or n_val,
 * n_val n_dealers or n_val n_dealers threshold >= 2^31.  Validators are split over the contexts whole; the device copy
 * of the shares is zeroed before the call returns. */
int hipbls_verify_secret_shares_batch_ct(const uint8_t* shares, const uint8_t* commitments, uint64_t n_val,
                                         uint32_t n_dealers, uint32_t threshold, int64_t my_id, int32_t* status);

/* A node's final share: out_shares[32 v ..] = sum over d of include[v n_dealers + d] ? shares[32 (v n_dealers + d) ..]
 * : 0, mod r.  include: one byte per (v, d), non-zero = the dealer is qualified (public); null = every dealer.
 * status[v] = ERR_COMBINE (no dealer included: public, decided first) | ERR_SECRET (an included share >= r) | OK;
 * zero bytes on error.  An excluded dealer's share is not looked at: it may be >= r.
 * out_pubs / pub_status (both null or both given): [out_share_v] g1 with hipbls_secret_to_public_key_batch_ct's bytes
 * and status (ERR_SECRET and zero bytes for a zero sum or a validator that failed).  One kernel, one lane per
 * validator (share_sum_ct).  n_val == 0 is OK; HIPBLS_ERR_ARG: n_dealers == 0, a null pointer with a non-zero count,
 * only one of out_pubs / pub_status, or n_val or n_val n_dealers >= 2^31.  Validators are split over the contexts
 * whole; the device copies of the shares and of the sums are zeroed before the call returns. */
int hipbls_combine_shares_batch_ct(const uint8_t* shares, const uint8_t* include, uint64_t n_val, uint32_t n_dealers,
                                   uint8_t* out_shares, int32_t* status, uint8_t* out_pubs, int32_t* pub_status);

/* Random-linear-combination BatchVerify.  Item i is (pks[48 i..], message msg_idx[i], sigs[96 i..]);
 * message m is msgs[msg_offsets[m] .. msg_offsets[m+1]) (n_msgs distinct messages, each hashed once).
 * status[i] is exactly hipbls_verify_batch's (i.e. tbls.Verify's) outcome for the item: items are
 * decoded and subgroup-checked one by one, windows of consecutive items are checked with one
 * multi-pairing under 64-bit random scalars derived from seed32 (32 bytes the caller draws from a
 * CSPRNG), and the items of a window that fails are re-verified individually.  Items sharing a
 * message should be adjacent (e.g. all partials of one validator): each run of equal msg_idx inside
 * a window costs one Miller loop.  HIPBLS_ERR_ARG when a msg_idx is out of range. */
int hipbls_batch_verify_rlc(const uint8_t* pks, const uint8_t* sigs, const uint32_t* msg_idx, uint64_t n,
                            const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t n_msgs, const uint8_t* seed32,
                            int32_t* status);
/* Resident pubshare table: decode + subgroup-check n public keys once and keep
 * them in HBM; replaces the previous table.  status[k] = OK | ERR_PUBKEY (an infinity key loads and
 * later verifies as ERR_VERIFY, like Verify).  The *_keys entry points name keys by table index and
 * return exactly what the wire-format calls return for the same key bytes. */
int hipbls_pubshare_table_load(const uint8_t* pks, uint64_t n, int32_t* status);
int hipbls_pubshare_table_size(uint64_t* n);
/* hipbls_verify_batch with pks[i] = table[key_idx[i]]; HIPBLS_ERR_ARG when an index is outside the table.
 * Batches the wire-format call would run on octets (AUTO up to 4,096 items, sixteen lanes up to 4; forced
 * HIPBLS_PAIR_OCTETS) take the same latency route with the keys copied from the table: each DISTINCT message is
 * looked up in the context's H(m) cache (hipbls_hcache_config; counted per distinct message per call in
 * hipbls_hcache_stats), a hit is read from its column, a miss is hashed once and INSERTED (on the proposer path the
 * lone Verify is the first call to see a root; the keyed sigagg that follows hits).  With the cache disabled or smaller
 * than the call's distinct messages, each is hashed once into a table of the call's own.  Statuses are unchanged in
 * every case.  Other pair modes, larger batches and HIPBLS_LAT_VERIFY_KEYS=0 keep one lane per item ("verify_keys"),
 * which leaves the cache alone.  Timed as "verify_prep8_keys" + "verify_gather_keys" + the check's name. */
int hipbls_verify_batch_keys(const uint32_t* key_idx, const uint8_t* msgs, const uint64_t* msg_offsets,
                             const uint8_t* sigs, uint64_t n, int32_t* status);
/* hipbls_batch_verify_rlc with pks[i] = table[key_idx[i]]. */
int hipbls_batch_verify_rlc_keys(const uint32_t* key_idx, const uint8_t* sigs, const uint32_t* msg_idx, uint64_t n,
                                 const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t n_msgs,
                                 const uint8_t* seed32, int32_t* status);

/* Windows checked, windows that failed, and items re-verified one by one in the last RLC call
 * (synchronizes the device). */
int hipbls_rlc_stats(uint64_t* windows, uint64_t* windows_failed, uint64_t* items_fallback);
/* Batch-wide check (charon_amd/csrc/rlcb.h): one multi-pairing over the whole batch with a Pippenger MSM for
 * sum r_i sig_i, ahead of the windows.  It decides an all-valid batch alone; when it fails, the windows decide
 * item by item, so statuses never depend on the mode.  HIPBLS_RLC_AUTO (default): batch-wide first for batches of
 * >= 1,024 items unless the last batch-wide check failed (then 8 calls windows-only); HIPBLS_RLC_WINDOWS: windows
 * only; HIPBLS_RLC_BATCH: batch-wide first always.  Returns the previous mode or HIPBLS_ERR_ARG. */
enum { HIPBLS_RLC_AUTO = 0, HIPBLS_RLC_WINDOWS = 1, HIPBLS_RLC_BATCH = 2 };
int hipbls_rlc_set_mode(int mode);
/* The batch-wide check's G1 side for batches that average >= 8 items per message (committee roots): each message
 * with >= `min` items gets one Pippenger sum of [r_i] pk_i (charon_amd/csrc/g1msm.h) and one Miller loop, instead of
 * a scalar multiplication per item.  0 turns it off; default 64.  Statuses never depend on it.  Returns the previous
 * value. */
int hipbls_rlc_set_g1_msm_min(uint32_t min);
/* Batch-wide checks launched and passed since load, and the last verdict (-1 none, 0 failed, 1 passed); waits for
 * the last one in flight. */
int hipbls_rlc_batch_stats(uint64_t* attempted, uint64_t* passed, int32_t* last);

/* Resident H(m) cache used by the host-buffer RLC calls: each distinct message is hashed to G2
 * once and kept in HBM across calls (FIFO over `capacity` slots, 192 B each); 0 disables it (the default).
 * Statuses are unchanged by the cache. */
int hipbls_hcache_config(uint64_t capacity);
int hipbls_hcache_stats(uint64_t* hits, uint64_t* misses, uint64_t* entries);
/* A hint: hash the n_msgs signing roots msgs[msg_offsets[m] .. msg_offsets[m+1]) into the H(m) cache before any
 * signature over them exists (the randao root at epoch start, a duty's root once consensus has decided the unsigned
 * data), so that the first hipbls_verify_batch_keys / queued hipbls_verify / keyed sigagg of each root is a hit.  The
 * call touches no signature, key or status.  Duplicate roots are folded; each distinct root the cache does not hold is
 * hashed on eight lanes ("hcache_fill8"; above 4,096 misses on one lane each, "rlc_hash") and inserted under the FIFO
 * replacement of the other writers, in EVERY context's cache.  *hashed / *present (each may be null; summed over
 * contexts): roots this call hashed and inserted / roots the cache already held.  The hits / misses of
 * hipbls_hcache_stats do not move (they count consumers; a Verify after a prefetch shows up as a hit); entries does.
 * With the cache disabled, or more distinct roots than its capacity, nothing is launched and both outputs are 0.  The
 * call returns after the columns are written.  HIPBLS_ERR_ARG for null or non-monotone offsets or null msgs with a
 * non-zero total; n_msgs == 0 is OK. */
int hipbls_hcache_prefetch(const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t n_msgs, uint64_t* hashed,
                           uint64_t* present);

/* Resident key cache used by the wire-format calls (hipbls_verify_batch[_device], hipbls_batch_verify_rlc[_device],
 * the submission queue's wire batches): the kernels look each 48-byte public key up in a per-context table in HBM and,
 * on a hit, skip its decompression and subgroup test; a key that decodes as a valid G1 point is published once and
 * never replaced (no eviction: a full probe window means the key is not cached).  Invalid encodings, points outside G1
 * and the infinity key are never cached.  Statuses are unchanged by the cache.  `slots` is rounded up to a power of
 * two (256 B each); 0 turns the cache off.  Default: 65,536 slots per context, or HIPBLS_KEYCACHE_SLOTS.  The call
 * waits for the device and empties the cache and its counters; it may run beside any other call, hipbls_verify
 * included (no kernel is enqueued on buffers it has released).  Stats are summed over contexts: items served from the
 * cache, items decoded by the kernel, entries written.  hipbls_keycache_stats also waits for the device, with each
 * context's lock held, so that it counts every call enqueued before it: a diagnostic, not for a hot path. */
int hipbls_keycache_config(uint64_t slots);
int hipbls_keycache_stats(uint64_t* hits, uint64_t* misses, uint64_t* inserts);

/* Resident root cache used by the wire-format Verify batches that run one lane per item (hipbls_verify_batch[_device]
 * above the lane-pair sizes, the submission queue's wire batches under HIPBLS_PAIR_SINGLE): a lookup kernel finds each
 * 32-byte message in a per-context table in HBM, and on a hit the Verify kernel takes H(m) from the entry -- after
 * comparing all 32 bytes and a check value -- instead of hashing the message to G2; a message it hashes is published
 * once.  Messages of any other length bypass the cache.  Statuses are unchanged by the cache.  Entries are never
 * replaced; when half the slots are written, the next call first waits for the device and empties the table (a
 * rollover).  `slots` is rounded up to a power of two (256 B each, at most 2^22); 0 turns the cache off.  Default:
 * 262,144 slots per context (64 MiB + 1 MiB), or HIPBLS_ROOTCACHE_SLOTS.  HIPBLS_ROOTCACHE_PARTITION=0 keeps the
 * items in their own order instead of dealing the hits to the front.  hipbls_rootcache_config waits for the device
 * and empties the cache and its counters; like hipbls_keycache_config it may run beside any other call.  Stats are
 * summed over contexts, since the last config: eligible items found by the lookup, eligible items not found, entries
 * written, rollovers.  hipbls_rootcache_stats waits for the device under each context's lock: a diagnostic. */
int hipbls_rootcache_config(uint64_t slots);
int hipbls_rootcache_stats(uint64_t* hits, uint64_t* misses, uint64_t* inserts, uint64_t* rollovers);

/* Line blocks of the root cache: beside H(m), the lane that publishes a root also records the 68 Miller-loop lines of
 * e(., H(m)) before their scaling by the key (19,712 B per root, in a pool of `blocks` blocks), and a later Verify of
 * that root replays them instead of walking H(m) through 63 doublings and 5 additions; the replayed words carry a
 * check value bound to the root, and a block that fails it is followed by the full loop.  Statuses are unchanged.
 * Default: half the root cache's slots (131,072 blocks, about 2.4 GiB per context, allocated by the first batch that
 * takes the one-lane route), or HIPBLS_ROOTCACHE_LINES; 0 turns the lines off, at most 2^22, and UINT64_MAX asks for
 * the default again.  A full pool publishes H(m) alone.  hipbls_rootcache_lines_config acts as
 * hipbls_rootcache_config does and also empties the root cache and its counters.  Stats are summed over contexts, since the last config of either kind: Verifies that replayed a
 * block, blocks published, roots published without a block because the pool was full, replays discarded by the
 * check.  hipbls_rootcache_lines_stats waits for the device under each context's lock: a diagnostic. */
int hipbls_rootcache_lines_config(uint64_t blocks);
int hipbls_rootcache_lines_stats(uint64_t* line_hits, uint64_t* blocks_published, uint64_t* pool_full,
                                 uint64_t* check_failures);

/* Device-resident cache of decoded signatures, per context: the 96 wire bytes of a signature -> its affine point.  A
 * partial signature is verified when it arrives and later handed to sigagg with its duty's other partials; with the
 * cache on, the Verify side publishes every signature it decoded and proved to lie in G2 (hipbls_verify_batch[_keys]
 * on the prep + pair routes, hipbls_batch_verify_rlc[_keys], the submission queue's batches on those routes), and
 * hipbls_threshold_aggregate[_verify]_batch[_keys] looks each partial up before it decompresses and subgroup-tests
 * it.  Only valid points are entries, an entry checks itself, and a miss runs the code it ran before: outputs and
 * statuses never depend on the cache.  The one-lane Verify routes, the octet and sixteen-lane latency routes and the
 * lone sigagg route neither fill nor read it.  `slots` is rounded up to a power of two (256 B each, at least 8, at
 * most 2^22); 0 turns the cache off, which is the default (or HIPBLS_SIGCACHE_SLOTS): off, every call launches the
 * kernels it launched before the cache existed.  When half the slots are written, the next Verify-side call first waits
 * for the device and empties the table (a rollover).  hipbls_sigcache_config waits for the device and empties the
 * cache and its counters; it may run beside any other call.  Stats are summed over contexts, since the last config:
 * partials found by sigagg, partials not found, entries written, rollovers.  hipbls_sigcache_stats waits for the
 * device under each context's lock: a diagnostic. */
int hipbls_sigcache_config(uint64_t slots);
int hipbls_sigcache_stats(uint64_t* hits, uint64_t* misses, uint64_t* inserts, uint64_t* rollovers);

/* ------------------------------------------- device-resident variants (inputs already in HBM) ---- */
/* Same semantics; every pointer is a device pointer; work is enqueued on `stream` (a hipStream_t,
 * NULL = the library's own non-blocking stream of that device, which is NOT ordered with the caller's default
 * stream: a caller that reads the results with other work must pass that work's stream) and the call returns
 * without synchronizing.  The call runs on the
 * device that owns the status array. */
int hipbls_verify_batch_device(const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_msg_offsets,
                               const uint8_t* d_sigs, uint64_t n, int32_t* d_status, void* stream);
/* n_parts = group_offsets[n_groups], passed explicitly so the call never reads device memory.  The _device sigagg
 * call is three kernels on `stream`; calls enqueued on different streams overlap (two workspace sets, each call's
 * first kernel after the previous call's), so a caller with consecutive duties can keep two in flight. */
/* core/sigagg (sigagg.go:138-159) in one call: ThresholdAggregate of every group (as
 * hipbls_threshold_aggregate_batch: out_sigs, agg_status) and Verify(dv_pks[g], msg g, out_sigs[g]) of each
 * aggregate (verify_status, as hipbls_verify_batch).  A group whose aggregation failed reports its aggregation
 * status in verify_status too.  The key decode and hash run beside the aggregation, and the aggregate goes to the
 * pairing check without being decompressed again: the same verdicts as the two calls, in less time.
 * A lone call -- one proposer duty: at most 4 groups and 64 partials, however they are split over the groups, in
 * HIPBLS_PAIR_AUTO -- takes the latency route instead of one lane per unit of work: keys, hashes and partials on
 * octets, then per group the sum, the check on sixteen lanes and [L^-1] S beside it (two kernels, timed as tv_prep8
 * and tv_lq16).  Same bytes and statuses. */
int hipbls_threshold_aggregate_verify_batch(const uint8_t* sigs, const int64_t* share_idx,
                                            const uint64_t* group_offsets, uint64_t n_groups, const uint8_t* dv_pks,
                                            const uint8_t* msgs, const uint64_t* msg_offsets, uint8_t* out_sigs,
                                            int32_t* agg_status, int32_t* verify_status);
int hipbls_threshold_aggregate_verify_batch_device(const uint8_t* d_sigs, const int64_t* d_share_idx,
                                                   const uint64_t* d_group_offsets, uint64_t n_groups,
                                                   uint64_t n_parts, const uint8_t* d_dv_pks, const uint8_t* d_msgs,
                                                   const uint64_t* d_msg_offsets, uint8_t* d_out_sigs,
                                                   int32_t* d_agg_status, int32_t* d_verify_status, void* stream);
int hipbls_threshold_aggregate_batch_device(const uint8_t* d_sigs, const int64_t* d_share_idx,
                                            const uint64_t* d_group_offsets, uint64_t n_groups, uint64_t n_parts,
                                            uint8_t* d_out_sigs, int32_t* d_status, void* stream);
/* hipbls_threshold_aggregate_verify_batch with dv_pks[g] = table[dv_key_idx[g]] (the validators' root keys loaded
 * into the resident table beside the pubshares, hipbls_pubshare_table_load) and message g = message msg_idx[g] of
 * n_msgs DISTINCT messages, msgs[msg_offsets[m] .. msg_offsets[m+1]) as in hipbls_batch_verify_rlc: an attester
 * duty's groups share a few roots, and each is hashed at most once.  out_sigs and both status arrays are exactly what
 * the wire-format call returns for the same key bytes, in every pair mode (a table entry that failed to load:
 * HIPBLS_ERR_PUBKEY; the infinity key: HIPBLS_ERR_VERIFY).  No key is decompressed or subgroup-tested: the table load
 * did that once.  Each distinct message is looked up in the context's H(m) cache (hipbls_hcache_config; counted in
 * hipbls_hcache_stats): a hit -- by sigagg time the RLC BatchVerify of the root's partials has normally cached it --
 * is read from its column, a miss is hashed once into a table of the call's own, also with the cache disabled.  The
 * call only reads the cache (sigagg is the last consumer of a root): it never inserts or evicts.  HIPBLS_ERR_ARG for
 * the whole call when a key index is outside the table or a message index is >= n_msgs.  Routes and kernels as the
 * wire-format call's, timed as tv_prep8_keys + tv_gather_keys + tv_lq16 (lone) and tv_phase_a_keys (throughput). */
int hipbls_threshold_aggregate_verify_batch_keys(const uint8_t* sigs, const int64_t* share_idx,
                                                 const uint64_t* group_offsets, uint64_t n_groups,
                                                 const uint32_t* dv_key_idx, const uint32_t* msg_idx,
                                                 const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t n_msgs,
                                                 uint8_t* out_sigs, int32_t* agg_status, int32_t* verify_status);
/* Device variant: the host never sees the messages, so every distinct message is hashed once into the call's own
 * table and the H(m) cache is untouched.  An out-of-range key or message index yields verify_status[g] =
 * HIPBLS_ERR_ARG, also where the group's aggregation failed; agg_status[g] and out_sigs are the aggregation's. */
int hipbls_threshold_aggregate_verify_batch_keys_device(
    const uint8_t* d_sigs, const int64_t* d_share_idx, const uint64_t* d_group_offsets, uint64_t n_groups,
    uint64_t n_parts, const uint32_t* d_dv_key_idx, const uint32_t* d_msg_idx, const uint8_t* d_msgs,
    const uint64_t* d_msg_offsets, uint64_t n_msgs, uint8_t* d_out_sigs, int32_t* d_agg_status,
    int32_t* d_verify_status, void* stream);
int hipbls_aggregate_device(const uint8_t* d_sigs, uint64_t n, uint8_t* d_out_sig, int32_t* d_status, void* stream);
int hipbls_sign_batch_device(const uint8_t* d_sks, const uint8_t* d_msgs, const uint64_t* d_msg_offsets,
                             uint64_t n, uint8_t* d_out_sigs, int32_t* d_status, void* stream);
int hipbls_secret_to_public_key_batch_device(const uint8_t* d_sks, uint64_t n, uint8_t* d_out_pks,
                                             int32_t* d_status, void* stream);
/* Device variants of hipbls_sign_batch_ct / hipbls_secret_to_public_key_batch_ct (tbls/herumi.go:303-313, 67-80):
 * they only enqueue.  The secrets stay in the caller's buffer; clearing it is the caller's. */
int hipbls_sign_batch_ct_device(const uint8_t* d_sks, const uint8_t* d_msgs, const uint64_t* d_msg_offsets,
                                uint64_t n, uint8_t* d_out_sigs, int32_t* d_status, void* stream);
int hipbls_secret_to_public_key_batch_ct_device(const uint8_t* d_sks, uint64_t n, uint8_t* d_out_pks,
                                                int32_t* d_status, void* stream);

/* Device variants of hipbls_threshold_split_batch_ct / hipbls_recover_secret_batch_ct: they only enqueue (the first
 * call on a context also enqueues the build of its comb table, and the call's stream waits for it on the device).
 * n_parts = group_offsets[n_groups], passed explicitly.  The secrets stay in the caller's buffers; clearing them is the caller's. */
int hipbls_threshold_split_batch_ct_device(const uint8_t* d_secrets, const uint8_t* d_poly_tails, uint64_t n_val,
                                           uint32_t total, uint32_t threshold, uint8_t* d_out_shares,
                                           int32_t* d_status, uint8_t* d_out_pubs, int32_t* d_pub_status,
                                           void* stream);
int hipbls_recover_secret_batch_ct_device(const uint8_t* d_shares, const int64_t* d_ids,
                                          const uint64_t* d_group_offsets, uint64_t n_groups, uint64_t n_parts,
                                          uint8_t* d_out_secrets, int32_t* d_status, uint8_t* d_out_pubkeys,
                                          int32_t* d_pk_status, void* stream);
/* As hipbls_public_key_share_batch / hipbls_public_key_recover_batch on device buffers: they only enqueue (on the
 * context that owns d_status), with the same argument rules; n_parts is the pubshare count, group_offsets[n_groups]. */
int hipbls_public_key_share_batch_device(const uint8_t* d_commitments, uint64_t n_val, uint32_t n_dealers,
                                         uint32_t threshold, const int64_t* d_ids, uint32_t n_ids, uint8_t* d_out_pubs,
                                         int32_t* d_status, void* stream);
int hipbls_public_key_recover_batch_device(const uint8_t* d_pubshares, const int64_t* d_ids,
                                           const uint64_t* d_group_offsets, uint64_t n_groups, uint64_t n_parts,
                                           uint8_t* d_out_pubkeys, int32_t* d_status, void* stream);
/* As hipbls_deal_commit_batch_ct / hipbls_verify_secret_shares_batch_ct / hipbls_combine_shares_batch_ct on device
 * buffers: they only enqueue (on the context that owns d_status; the first call on a context also enqueues the build
 * of its comb table), with the same argument rules.  my_id is passed by value.  The share check keeps the expected
 * bytes in the context's workspace, ordered against calls on other streams.  The secrets stay in the caller's
 * buffers; clearing them is the caller's. */
int hipbls_deal_commit_batch_ct_device(const uint8_t* d_secrets, const uint8_t* d_poly_tails, uint64_t n_val,
                                       uint32_t total, uint32_t threshold, uint8_t* d_out_shares, int32_t* d_status,
                                       uint8_t* d_out_commitments, int32_t* d_com_status, void* stream);
int hipbls_verify_secret_shares_batch_ct_device(const uint8_t* d_shares, const uint8_t* d_commitments, uint64_t n_val,
                                                uint32_t n_dealers, uint32_t threshold, int64_t my_id,
                                                int32_t* d_status, void* stream);
int hipbls_combine_shares_batch_ct_device(const uint8_t* d_shares, const uint8_t* d_include, uint64_t n_val,
                                          uint32_t n_dealers, uint8_t* d_out_shares, int32_t* d_status,
                                          uint8_t* d_out_pubs, int32_t* d_pub_status, void* stream);

/* As hipbls_batch_verify_rlc; seed32 is a host pointer.  An out-of-range msg_idx[i] yields
 * status[i] = HIPBLS_ERR_ARG. */
int hipbls_batch_verify_rlc_device(const uint8_t* d_pks, const uint8_t* d_sigs, const uint32_t* d_msg_idx, uint64_t n,
                                   const uint8_t* d_msgs, const uint64_t* d_msg_offsets, uint64_t n_msgs,
                                   const uint8_t* seed32, int32_t* d_status, void* stream);

/* Device variant of hipbls_verify_aggregate_batch (nkeys = key_offsets[n_groups], passed explicitly). */
int hipbls_verify_aggregate_batch_device(const uint8_t* d_pks, uint64_t nkeys, const uint64_t* d_key_offsets,
                                         uint64_t n_groups, const uint8_t* d_sigs, const uint8_t* d_msgs,
                                         const uint64_t* d_msg_offsets, int32_t* d_status, void* stream);

/* Device variant of hipbls_verify_aggregate_batch_keys (nkeys = key_offsets[n_groups], passed explicitly).  The host
 * never sees the messages, so each group's message is hashed and the H(m) cache is untouched.  A key index outside the
 * table yields status[g] = HIPBLS_ERR_ARG for that group only. */
int hipbls_verify_aggregate_batch_keys_device(const uint32_t* d_key_idx, uint64_t nkeys, const uint64_t* d_key_offsets,
                                              uint64_t n_groups, const uint8_t* d_sigs, const uint8_t* d_msgs,
                                              const uint64_t* d_msg_offsets, int32_t* d_status, void* stream);

/* Device variants of the *_keys calls: an out-of-range key or message index yields
 * status[i] = HIPBLS_ERR_ARG. */
int hipbls_verify_batch_keys_device(const uint32_t* d_key_idx, const uint8_t* d_msgs, const uint64_t* d_msg_offsets,
                                    const uint8_t* d_sigs, uint64_t n, int32_t* d_status, void* stream);
int hipbls_batch_verify_rlc_keys_device(const uint32_t* d_key_idx, const uint8_t* d_sigs, const uint32_t* d_msg_idx,
                                        uint64_t n, const uint8_t* d_msgs, const uint64_t* d_msg_offsets,
                                        uint64_t n_msgs, const uint8_t* seed32, int32_t* d_status, void* stream);

/* Average duration (ms) per launch of a kernel over the calls since the last reset, measured with HIP
 * events on the stream it runs on (bench.py roofline; enable with hipbls_set_timing).  Names: "verify"
 * (k_verify_fused), "verify_prep" + "verify_pair_lg2" (lane-pair Verify), "verify_keys", "rlc_items",
 * "rlc_hash", "rlc_window" / "rlc_window_lg2", "rlc_fallback" / "rlc_fallback_lg2", "tagg_scale", "tagg_sum",
 * "fav"; sigagg in one call: "tv_phase_a", "tv_check_unscale", "tv_prep8", "tv_lq16", and with keys by index
 * "tv_phase_a_keys", "tv_prep8_keys", "tv_gather_keys"; the keyed Verify latency route: "verify_prep8_keys",
 * "verify_gather_keys" (then "verify_pair_lq16" / "verify_pair_lq8" as the wire-format call); FastAggregateVerify
 * on the lone route: "fav_prep8", "fav_lq16", and with keys by index "fav_prep8_keys", "fav_lq16_keys", "fav_keys",
 * "fav_sum_keys". */
int hipbls_kernel_timing(const char* name, double* avg_ms, uint64_t* launches);
int hipbls_kernel_timing_reset(void);

#ifdef __cplusplus
}
#endif

#endif /* HIPBLS_H */
