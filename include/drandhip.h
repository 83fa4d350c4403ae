/*
 * drandhip.h — C ABI of libdrandhip, the MI355X (gfx950) beacon-verification engine for drand.
 *
 * Plain pointers and sizes only (cgo / ctypes / JNI friendly). Every entry point is thread-safe and
 * reentrant: concurrent callers each get their own HIP stream and device workspace from an internal
 * pool. Inputs are borrowed for the duration of the call and never retained; outputs are written into
 * caller-owned buffers. Batch calls block until their results are on the host.
 *
 * Replaces, for the verification hot path, the kyber / kyber-bls12381 / kilic arithmetic that drand
 * reaches through (reference at /root/reference, drand snapshot 2025-01-17):
 *   crypto.Scheme.VerifyBeacon            crypto/schemes.go:70-72
 *   crypto.Scheme.DigestBeacon            crypto/schemes.go:106-114 (chained), 147-151, 187-191
 *   crypto.RandomnessFromSignature        crypto/schemes.go:249-252
 *   crypto.SchemeFromName                 crypto/schemes.go:206-217
 *   sign.ThresholdScheme.VerifyRecovered  [kyber v1.1.18 sign/tbls], called at crypto/schemes.go:71,
 *                                         chain/beacon/chainstore.go:207
 *   sign.ThresholdScheme.Recover          [kyber v1.1.18 sign/tbls], called at chain/beacon/chainstore.go:202
 *   sign.Scheme.Verify (AuthScheme)       [kyber v1.1.18 sign/bls], crypto/schemes.go:102,143,183, called at
 *                                         key/keys.go:61-64 (Identity.ValidSignature)
 *   sign.Scheme.Verify (DKGAuthScheme)    [kyber v1.1.18 sign/schnorr], crypto/schemes.go:103,144,184, called at
 *                                         core/drand_beacon_control.go:354,476 and core/group_setup.go:384
 * and adds the batch entry point the serial per-round loops need:
 *   chain/beacon/sync_manager.go:191-225 (CheckPastBeacons), client/verify.go:139-160, lp2p relays;
 * and the read path of the trimmed bolt store that loop runs over, parsed on the device from the store file:
 *   chain/boltdb/trimmed.go:87-107,156-193 (dh_store_*); and of the legacy untrimmed store, chain/boltdb/store.go:172-210
 *   (dh_store_open_bolt_format, dh_store_beacons_device, dh_store_deferred).
 * INTEGRATION.md shows the cgo binding a drand maintainer would add.
 */
#ifndef DRANDHIP_H
#define DRANDHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes (>= 0 success) */
#define DH_OK 0
#define DH_EINVAL (-1)   /* bad argument: unknown scheme, wrong key/sig length, unsupported message shape */
#define DH_EDEVICE (-2)  /* HIP runtime / kernel failure; the caller should fall back to its CPU path */
#define DH_ENOMEM (-3)   /* device allocation failed */
#define DH_EKEY (-4)     /* the group public key does not decode to a subgroup point */
#define DH_ERECOVER (-5) /* Recover: fewer than t valid partial signatures */
#define DH_EBUSY (-6)    /* every library worker is held (DRANDHIP_MAX_WORKERS, default 24): dh_batch_begin at once,
                            a blocking call after DRANDHIP_LEASE_TIMEOUT_MS when node batches hold them all */
#define DH_EABANDONED (-7) /* node-wide batch: some rank's dh_batch_begin failed, every rank abandons the batch */
#define DH_ECORRUPT (-8)   /* the store file is structurally invalid (which check failed: dh_last_error_string) */
#define DH_ENOBEACON (-9)  /* chainerrors.ErrNoBeaconStored: empty store, or Last() has no previous record (chained) */

/* scheme ids, in the order of crypto/schemes.go:206-219 plus the RFC 9380 quicknet scheme */
#define DH_SCHEME_CHAINED 0      /* "pedersen-bls-chained":   sig G2 (96 B), key G1 (48 B), msg SHA256(prev||round) */
#define DH_SCHEME_UNCHAINED 1    /* "pedersen-bls-unchained": sig G2, key G1, msg SHA256(round) */
#define DH_SCHEME_G1_LEGACY 2    /* "bls-unchained-on-g1":    sig G1 (48 B), key G2 (96 B), G2 hash DST (legacy) */
#define DH_SCHEME_G1_RFC9380 3   /* "bls-unchained-g1-rfc9380" (quicknet): sig G1, key G2, G1 hash DST */

/*
 * Select the device: bit i of device_mask = HIP device i, at most one bit (one process per GPU);
 * 0 = device 0 or the device already selected. Idempotent; asking for another device after initialisation is
 * DH_EINVAL until dh_shutdown.
 */
int dh_init(uint32_t device_mask);
/*
 * Release all device resources. Safe while other threads are inside calls: their workers are retired and freed
 * when those calls return. Calls after this re-initialise lazily.
 */
void dh_shutdown(void);

/* crypto.SchemeFromName: scheme id or DH_EINVAL */
int dh_scheme_from_name(const char* name);
/* byte lengths for a scheme: compressed signature / group public key; DH_EINVAL for unknown ids */
int dh_sig_len(int scheme);
int dh_key_len(int scheme);

/*
 * Batch VerifyBeacon over n rounds sharing one group public key.
 *   pk           compressed key-group point (dh_key_len bytes)
 *   rounds[i]    round numbers
 *   sigs         n signatures, record i at sigs + i*sig_stride (sig_stride >= dh_sig_len, multiple of 4)
 *   prevs        chained scheme only (NULL otherwise): previous signature of round i at prevs + i*prev_stride;
 *                length prev_lens[i] (or prev_stride when prev_lens is NULL), any length <= prev_stride: the
 *                record is hashed as stored, like crypto/schemes.go:106-114 (0 = none, 32 = genesis seed,
 *                96 = stored G2 signature; a corrupted 31- or 100-byte record simply fails its round).
 *                prev_lens[i] > prev_stride is DH_EINVAL here and rejects round i on the device entry point.
 *   verdict_out  n bytes: 1 = VerifyBeacon returns nil, 0 = it returns an error
 *   rand_out     n*32 bytes SHA-256(sig) (RandomnessFromSignature) or NULL
 *   seed         0 = draw the random-linear-combination seed from the OS CSPRNG; otherwise deterministic
 * One call runs on one internal stream by default (its per-round kernels, then its MSM and pairing checks on a
 * high-priority stream): a 4M-round call runs at ~94% of the rate of 8 concurrent 1M calls, a 1M-round call at
 * ~85% (its ~8 ms latency tail, MSM + pairing check, is exposed). DRANDHIP_SPLIT="chunk,workers" / dh_set_split cut a call into
 * chunks verified on several streams instead.
 * A large batch tests subgroup membership once per batch on the MSM's buckets, with an exact per-round fallback:
 * DRANDHIP_SUB_BATCH_MIN (G1 signatures, 131072) / DRANDHIP_SUB_BATCH_MIN_G2 (G2 signatures, 393216) rounds and
 * more; DRANDHIP_SUBGROUP_BATCH=0 keeps the per-round test for both. Verdicts are the same.
 * Returns DH_OK or a negative error code (no verdicts are valid on error).
 */
int dh_verify_batch(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* rounds, const uint8_t* sigs,
                    size_t sig_stride, const uint8_t* prevs, size_t prev_stride, const uint32_t* prev_lens, size_t n,
                    uint8_t* verdict_out, uint8_t* rand_out, uint64_t seed);

/* Set the one-call split of dh_verify_batch / dh_verify_batch_device (chunk_rounds 0 = one stream per call, the
 * default). */
int dh_set_split(uint64_t chunk_rounds, int workers);

/*
 * Same as dh_verify_batch with every array already resident in device memory (HIP device pointers). The inputs
 * may still be in production on `hip_stream` (a hipStream_t): the library's streams wait for that stream's work
 * first; NULL = the inputs are ready. Blocks until done. `stats_out` (nullable, host) receives
 * {levels, groups_failed, leaf_rounds, rounds_rejected} (levels: the deepest chunk's).
 */
int dh_verify_batch_device(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* d_rounds, const uint8_t* d_sigs,
                           size_t sig_stride, const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens,
                           size_t n, uint8_t* d_verdict_out, uint8_t* d_rand_out, uint64_t seed, void* hip_stream,
                           uint64_t stats_out[4]);

/* Single VerifyBeacon (crypto/schemes.go:70-72): 1 valid, 0 invalid, < 0 error */
int dh_verify_beacon(int scheme, const uint8_t* pk, size_t pk_len, uint64_t round, const uint8_t* sig, size_t sig_len,
                     const uint8_t* prev, size_t prev_len);

/*
 * ThresholdScheme.VerifyRecovered(pk, msg, sig) (kyber sign/tbls = bls.Verify; called at
 * chain/beacon/chainstore.go:207 on every recovered signature) for a 32-byte msg (a beacon digest):
 * 1 valid / 0 invalid / < 0 error.
 */
int dh_verify_recovered(int scheme, const uint8_t* pk, size_t pk_len, const uint8_t* msg32, const uint8_t* sig,
                        size_t sig_len);

/*
 * Batch VerifyRecovered: n (32-byte digest, signature) pairs under one key, host buffers, same batching and
 * bit-exact per-item verdicts as dh_verify_batch (verdict_out[i] = 1 valid, 0 invalid).
 */
int dh_verify_recovered_batch(int scheme, const uint8_t* pk, size_t pk_len, const uint8_t* msgs32, const uint8_t* sigs,
                              size_t sig_stride, size_t n, uint8_t* verdict_out, uint64_t seed);

/* crypto.Scheme.DigestBeacon for n rounds (host-side SHA-256, no device): out n*32 bytes */
int dh_digest_batch(int scheme, const uint64_t* rounds, const uint8_t* prevs, size_t prev_stride,
                    const uint32_t* prev_lens, size_t n, uint8_t* out);

/* RandomnessFromSignature for n signatures on the device: out n*32 bytes */
int dh_randomness_batch(int scheme, const uint8_t* sigs, size_t sig_stride, size_t n, uint8_t* out);

/*
 * Batch tbls Recover (kyber sign/tbls Recover + share.RecoverCommit, called at chain/beacon/chainstore.go:202):
 * for each of n_rounds rounds, partials[part_off[j] .. part_off[j+1]) are (2-byte BE index || sig) records
 * of (2 + sig_len) bytes for message msgs32[j] (32-byte digests). Each partial is verified against
 * PubPoly.Eval(index) (commits = t compressed key-group points); the first t valid ones (in the given
 * order) are kept, sorted by index, and Lagrange-interpolated at 0 in the signature group.
 * sig_out: n_rounds * sig_len bytes; status_out[j] = 1 recovered, 0 not enough valid partials. n_nodes <= 65536
 * (every 2-byte index); a caller that wants kyber's any-index semantics passes max(n, largest index + 1).
 */
int dh_recover_batch(int scheme, const uint8_t* commits, int t, int n_nodes, const uint8_t* msgs32,
                     const uint8_t* partials, const uint32_t* part_off, size_t n_rounds, uint8_t* sig_out,
                     uint8_t* status_out);

/*
 * Batch ThresholdScheme.VerifyPartial(pubPoly, msg, partial) (kyber sign/tbls; called per incoming partial at
 * chain/beacon/node.go:150): same input layout as dh_recover_batch; ok_out[k] (one byte per partial, in
 * input order) = 1 when the k-th partial's signature verifies under PubPoly.Eval(index) for its round's
 * message, 0 otherwise.
 * Deviation from kyber, documented: kyber's VerifyPartial evaluates PubPoly.Eval(i) for ANY index i, so a partial
 * validly signed with f(i+1) for i >= n_nodes would pass there; here indices >= n_nodes have no share in the group
 * and are reported invalid (and skipped by dh_recover_batch). drand never hands such a partial to the scheme:
 * chain/beacon/node.go:138-141 rejects indices outside the group before VerifyPartial and the partial cache.
 */
int dh_verify_partials_batch(int scheme, const uint8_t* commits, int t, int n_nodes, const uint8_t* msgs32,
                             const uint8_t* partials, const uint32_t* part_off, size_t n_rounds, uint8_t* ok_out);

/*
 * sign.Scheme.Verify(public, msg, sig) in batch (kyber sign/bls Verify: the schemes' AuthScheme, crypto/schemes.go:102,
 * 143,183, in the groups, hash and DST of the scheme's beacon signatures) under MANY keys and for messages of ANY
 * length, 0 included: item i = key key_idx[i] of the table, message msgs[msg_off[i] .. msg_off[i+1]), signature i at
 * sigs + i*sig_stride. Replaces per-item bls.Verify loops such as key/group.go:487-495 and the per-chain calls of a
 * process that follows several chains of one scheme. Host buffers; blocks.
 *   keys         n_keys compressed key-group points (dh_key_len bytes each); duplicates allowed
 *   key_idx      n indices < n_keys (else DH_EINVAL); NULL = item i uses key i, and then n_keys must equal n
 *   msg_off      n + 1 non-decreasing offsets into msgs (else DH_EINVAL)
 *   verdict_out  n bytes: 1 exactly when Verify returns nil (signatures subgroup-checked, infinity rejected)
 *   key_ok_out   n_keys bytes or NULL: 1 when the key decodes to a subgroup point (the rule of the group key of
 *                dh_verify_batch). A bad key is not a call error: every item under it gets verdict 0, items under
 *                other keys are unaffected
 *   seed         as dh_verify_batch
 *   stats_out    NULL or {levels, keys_failed, leaf_items, items_rejected}
 * n = 0 is DH_OK and writes nothing; items with no keys are DH_EINVAL. The check: one product of n_keys + 1 pairings
 * over random linear combinations per key; when it fails, one 2-pairing check per key, then per-item checks under
 * the failing keys only; small batches and batches with few items per key go straight to per-item checks
 * (DESIGN.md §10). DRANDHIP_AUTH_PATH=leaf|rlc (read at every call) forces per-item checks / the combined check.
 */
int dh_bls_verify_batch(int scheme, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                        const uint32_t* msg_off, const uint8_t* sigs, size_t sig_stride, size_t n, uint8_t* verdict_out,
                        uint8_t* key_ok_out, uint64_t seed, uint64_t stats_out[4]);

/* Identity.Hash for n keys (key/keys.go:53-57): BLAKE2b-256 of each compressed key (dh_key_len bytes), host only, no
 * device; out32: n*32 bytes */
int dh_identity_hash_batch(int scheme, const uint8_t* keys, size_t n, uint8_t* out32);

/* Identity.ValidSignature for n identities (key/keys.go:61-64; the serial loop of Group.UnsignedIdentities,
 * key/group.go:487-495): verdict_out[i] = 1 when sigs[i] is key i's signature of Identity.Hash(key i), i.e.
 * dh_bls_verify_batch over dh_identity_hash_batch with one key per item */
int dh_identity_verify_batch(int scheme, const uint8_t* keys, const uint8_t* sigs, size_t sig_stride, size_t n,
                             uint8_t* verdict_out);

/*
 * schnorr.Verify(public, msg, sig) in batch: kyber's sign/schnorr over the scheme's key group, the schemes'
 * DKGAuthScheme (crypto/schemes.go:103,144,184). It is what dkg.VerifyPacketSignature checks on every deal, response
 * and justification bundle (core/drand_beacon_control.go:354,476) and what authenticates the leader's signature over
 * group.Hash() (core/group_setup.go:384); the matching Sign (core/drand_beacon_control.go:1011) stays on the host.
 * Items, keys and messages as dh_bls_verify_batch: item i = key key_idx[i] of the table, message
 * msgs[msg_off[i] .. msg_off[i+1]) of any length, signature i at sigs + i*sig_stride. Host buffers; blocks;
 * thread-safe. No reference vector exists for this scheme: the behaviour is the restatement in DESIGN.md §11.
 *   sigs         dh_schnorr_sig_len bytes each: R, a compressed key-group point (dh_key_len bytes), then s, a 32-byte
 *                big-endian integer. Verdict 0 when s >= r, when R does not decode (flags, x < p, on the curve) or is
 *                the point at infinity. The last is a documented choice, like the index rule of
 *                dh_verify_partials_batch above: kyber's behaviour for R at infinity is not pinned by any vector,
 *                and no honest signer produces it. R is not subgroup-tested: [s]G - [h]P lies in the subgroup, so an
 *                R outside it never satisfies the equation
 *   verdict_out  n bytes: 1 exactly when [s]G == R + [h]P with h = SHA-512(R bytes || P bytes || msg) read as a
 *                big-endian integer mod r, G the key group's generator and P the item's key
 *   key_ok_out   n_keys bytes or NULL, the key rule of dh_bls_verify_batch: 1 when the key is a compressed subgroup
 *                point other than infinity. A bad key is not a call error: its items get verdict 0
 * DH_EINVAL: key_idx out of range, msg_off decreasing, key_idx NULL with n_keys != n, sig_stride below the signature
 * length or not a multiple of 4, items but no keys. n = 0 is DH_OK and writes nothing. Each item is checked on its
 * own (two scalar multiplications sharing one chain, no pairing). DRANDHIP_SCHNORR_PATH=plain (read at every call)
 * selects the cross-check form, two plain double-and-add multiplications per item.
 */
int dh_schnorr_verify_batch(int scheme, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                            const uint32_t* msg_off, const uint8_t* sigs, size_t sig_stride, size_t n, uint8_t* verdict_out,
                            uint8_t* key_ok_out);
/* bytes of one Schnorr signature: dh_key_len(scheme) + 32 */
int dh_schnorr_sig_len(int scheme);

/*
 * Node-wide batch check over the GPUs of one node (one process per GPU; the sharded form of
 * chain/beacon/sync_manager.go:191-225). Every rank prepares its shard of rounds and its level-0
 * random-linear-combination sums with dh_batch_begin, which writes one record of dh_partial_bytes(scheme) bytes into
 * d_partials_out (device memory): A = sum r_i sigma_i, B = sum r_i H(m_i) (Jacobian), a status word (0) and padding.
 * The ranks all-gather the records (RCCL over xGMI); a rank whose dh_batch_begin failed contributes a record with a
 * nonzero status word, so every rank learns it from the gathered data. dh_batch_check queues, on the batch's own
 * worker, the sum of the k gathered records and ONE pairing check e(g, sum A) = e(pk, [h] sum B) for the whole node;
 * when it passes, every decoded round of the batch is marked valid on the device. dh_batch_finish(b,
 * DH_NODE_CHECKED, ...) then waits for that result: it returns 1 (the node check passed), or 0 (it failed: the
 * shard's own level-0 check and bisection ran, so the verdicts are per-round exact either way), or DH_EABANDONED
 * (some rank's record carried a nonzero status: nothing is valid), or another error.
 *
 * Streams: the batch's record is written, and its check and bisection run, on ONE stream of the library,
 * dh_batch_stream(b) (a hipStream_t): the caller queues the collective there (e.g. torch.cuda.ExternalStream), so the
 * record, the all-gather and the check follow each other in stream order, with no host wait and, for one rank, no
 * cross-stream wait. dh_batch_begin returns as soon as the batch is queued; with hip_stream (a hipStream_t) non-NULL
 * it orders the batch after hip_stream's work (inputs still in production there), with NULL the inputs must be
 * complete (NULL means "no stream": work on the legacy NULL / default stream must be synchronised by the caller).
 * A host caller that wants the record itself waits for dh_batch_stream(b).
 * dh_batch_check orders the check after hip_stream's work when hip_stream is another stream (the gathered records
 * produced there); NULL or dh_batch_stream(b) adds no wait. The only host wait of a batch is in dh_batch_finish.
 *
 * A batch holds one library worker from begin to finish (DH_EBUSY if none is idle: begin never waits, since the
 * other ranks may be waiting in the collective); the arguments of dh_batch_begin must stay valid until
 * dh_batch_finish returns. A blocking call (any other entry point) made while EVERY worker is held by unfinished
 * batches waits at most DRANDHIP_LEASE_TIMEOUT_MS (default 30 s) for one and then fails with DH_EBUSY: finish the
 * batches first. A batch of one round contributes the identity to the node-wide sums, so its round always gets its
 * own check in dh_batch_finish, whatever the node-wide result. dh_batch_finish with node_pass 1 / 0 (a result the caller obtained itself, e.g. from
 * dh_check_partials) accepts every decoded round / runs the shard's own check and returns DH_OK; node_pass < 0
 * (other than DH_NODE_CHECKED) abandons the batch. dh_check_partials is the standalone check of k records (it
 * leases its own worker and blocks): pass_out = 1 / 0, DH_EABANDONED when a status word is nonzero.
 */
typedef struct dh_batch dh_batch;
#define DH_NODE_CHECKED 2 /* dh_batch_finish: take the result of dh_batch_check */
int dh_partial_bytes(int scheme);
int dh_batch_begin(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* d_rounds, const uint8_t* d_sigs,
                   size_t sig_stride, const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, size_t n,
                   uint8_t* d_verdict_out, uint8_t* d_rand_out, uint64_t seed, void* hip_stream, dh_batch** batch_out,
                   uint8_t* d_partials_out);
void* dh_batch_stream(dh_batch* batch);
int dh_batch_check(dh_batch* batch, const uint8_t* d_partials, size_t k, void* hip_stream);
int dh_check_partials(int scheme, const uint8_t* pk, size_t pk_len, const uint8_t* d_partials, size_t k, int* pass_out);
int dh_batch_finish(dh_batch* batch, int node_pass, uint64_t stats_out[4]);

/*
 * Trimmed bbolt chain stores on the device: the read path of chain/boltdb/trimmed.go:87-107,156-193 (bucket "beacons",
 * key = round as 8 bytes big-endian, value = the raw signature, PreviousSig of round r = the stored value of r - 1;
 * the default layout of every new store, chain/boltdb/store.go:82-93) and the CheckPastBeacons loop over it
 * (chain/beacon/sync_manager.go:170-235), without the serial bbolt cursor. `file` is the image of the store file
 * (go.etcd.io/bbolt format v2, any page size: the meta page names it), e.g. a read-only mmap; it is borrowed for the
 * call. Every structural defect of the file is DH_ECORRUPT, never a read outside [file, file + len).
 *
 * dh_bolt_index: host only, no device (like dh_identity_hash_batch). What a bbolt cursor does before its first Next():
 * the valid meta page with the larger txid, the "beacons" entry of the root bucket, then the branch pages depth-first
 * in key order: one BYTE OFFSET per leaf (an inline bucket is the one leaf inside its bucket value). More than `cap`
 * leaves: DH_EINVAL with *n_leaves_out = the number needed.
 */
int dh_bolt_index(const uint8_t* file, size_t len, uint32_t* page_size_out, uint64_t* leaf_off_out, size_t cap,
                  size_t* n_leaves_out);

/*
 * Open a store: index the file on the host, upload the image (it stays resident in device memory until close: a
 * mainnet-size store is ~0.6 GB), validate and summarise every leaf on the device. Files above
 * DRANDHIP_STORE_MAX_BYTES (default 16 GiB) are refused with DH_ENOMEM, as is a failed allocation: the caller keeps
 * its host reader. Replaces boltdb.newTrimmedStore's bolt.Open for reading (chain/boltdb/trimmed.go:47-85).
 * Handles are independent of the library's workers; calls on one handle from several threads are serialised by a
 * mutex in the handle. dh_shutdown invalidates every handle (a handle inside a call when that call returns): later
 * calls on it fail with DH_EINVAL and only dh_store_close is valid.
 */
typedef struct dh_store dh_store;
int dh_store_open_bolt(const uint8_t* file, size_t len, dh_store** out);
/* Store.Len / the cursor's First and Last (trimmed.go:109-122,195-221): out = {len (every element of the bucket that
 * is not a nested bucket, as Len counts keys), round records (8-byte keys), first round, last round, longest value
 * in bytes, leaves} */
int dh_store_stat(const dh_store* store, uint64_t out[6]);
/*
 * The records of rounds first..last as columns in device memory, in key order (the cursor walk of
 * trimmedStore.Cursor / Get, trimmed.go:156-193,223-262, for a whole range): d_rounds[i], d_lens[i] = the stored length,
 * the value at d_rows + i*row_stride (row_stride a multiple of 4, at most 1 MiB), copied in full and zero-padded when it fits and left
 * ALL ZERO when it is longer than row_stride (never cut to a prefix: a wrong-length record must not decode). d_missing
 * (nullable) receives the rounds of [first, last] with no record, ascending. The layout serves the verifier with no
 * second copy: gather first-1..last and pass d_sigs = d_rows + row_stride, d_prevs = d_rows, d_prev_lens = d_lens,
 * d_rounds + 1 to dh_verify_batch_device. Too little room (cap_rows, cap_missing): DH_EINVAL with *n_rows_out and
 * *n_missing_out = the sizes needed and nothing written; at most 16M rows per call. Outputs still in use on
 * hip_stream (nullable) are waited for; the call blocks until the columns are complete.
 */
int dh_store_columns_device(dh_store* store, uint64_t first, uint64_t last, size_t row_stride, uint64_t* d_rounds,
                            uint8_t* d_rows, uint32_t* d_lens, size_t cap_rows, size_t* n_rows_out, uint64_t* d_missing,
                            size_t cap_missing, size_t* n_missing_out, void* hip_stream);
/*
 * SyncManager.CheckPastBeacons (chain/beacon/sync_manager.go:170-235) over the store: the faulty rounds, ascending,
 * among rounds 1 .. min(up_to, Last().Round), visited while round < Len() as that loop does. A round is faulty when
 * its record is missing, when the scheme is chained and the record of round - 1 is missing (the Get error of
 * trimmed.go:183-190), when its stored length is not dh_sig_len, or when dh_verify_batch_device rejects it. Rounds are
 * verified `window` at a time on the columns in place, rows of roundup4(max(dh_sig_len, the longest value in the
 * window's leaves)) bytes, so an odd-length stored record is hashed as stored and marks only its own round; a window
 * whose rows would exceed 64 KiB is DH_EINVAL (keep the host path). `cb` (nullable) is called ONCE PER WINDOW with the
 * window's first round, not once per round as the reference's callback is. More than `cap` faulty rounds: every round
 * is still counted, DH_EINVAL with *n_faulty_out = the number needed. DH_ENOBEACON when Last() fails.
 */
int dh_store_check_past(dh_store* store, int scheme, const uint8_t* pk, size_t pk_len, uint64_t up_to, size_t window,
                        uint64_t seed, uint64_t* faulty_out, size_t cap, size_t* n_faulty_out,
                        void (*cb)(uint64_t round, uint64_t up_to, void* arg), void* cb_arg);
void dh_store_close(dh_store* store);

/*
 * Legacy untrimmed bbolt chain stores on the device: BoltStore of chain/boltdb/store.go:143-210, the
 * format every store created before the trimmed one still has (store.go:82-110 keeps it). Same bucket and keys; the
 * value is Beacon.Marshal() (chain/beacon.go:31-39), hexjson: {"PreviousSig":P,"Round":D,"Signature":S}. PreviousSig
 * is the record's own field, so a missing round r - 1 does not fail round r, and Last() fails on an empty bucket only.
 *
 * The device decodes the CANONICAL form only: exactly those bytes, nothing before, between or after; P and S each null
 * or a quoted even number (0 allowed) of characters 0-9a-f; D a decimal of 1-20 digits without a leading zero (0
 * itself excepted) that fits 64 bits and equals the key. Stores written by drand are canonical throughout. Every other
 * value (uppercase hex, odd digit count, whitespace, reordered or extra fields, Round != key, cut or trailing bytes)
 * is DEFERRED: the device reports the record's key and decides nothing. The caller's host decoder decides it;
 * drand_amd.store does so with its own restatement of Beacon.Unmarshal (beacon_from_hexjson), which is NOT pinned to
 * nikkolasg/hexjson's decoder, so a verdict on a deferred record is that restatement's.
 *
 * dh_store_open_bolt_format: dh_store_open_bolt (= DH_STORE_TRIMMED) with the format named. DH_STORE_AUTO restates
 * shouldUseTrimmedBolt on the first value of the bucket: canonical -> untrimmed; an empty bucket -> trimmed; a first
 * byte '{' but not canonical -> DH_EINVAL (name the format); anything else -> trimmed.
 */
#define DH_STORE_TRIMMED 0
#define DH_STORE_UNTRIMMED 1
#define DH_STORE_AUTO 2
#define DH_DEFERRED 1 /* success: the call skipped records that are not canonical hexjson (dh_store_deferred lists them) */
int dh_store_open_bolt_format(const uint8_t* file, size_t len, int format, dh_store** out);
/* out = {format (TRIMMED / UNTRIMMED, never AUTO), deferred round records, longest decoded Signature in bytes, longest
 * decoded PreviousSig in bytes}; the last three are 0 for a trimmed store */
int dh_store_format_stat(const dh_store* store, uint64_t out[4]);
/*
 * The beacons of rounds first..last of an untrimmed store (DH_EINVAL on a trimmed handle) as columns in device memory,
 * in key order: d_rounds[i] = the key, d_deferred[i] = 1 for a deferred record (zero rows, zero lengths), else
 * d_sig_lens[i] / d_prev_lens[i] = the decoded byte lengths and the hex-DECODED Signature / PreviousSig at
 * d_sigs + i*sig_stride / d_prevs + i*prev_stride, copied whole and zero-padded when it fits its stride and left ALL
 * ZERO when it does not (never a prefix). d_prevs and d_prev_lens are nullable together. Strides are multiples of 4,
 * at most 1 MiB. The outputs feed dh_verify_batch_device directly (d_prevs / d_prev_lens for the chained scheme, NULL
 * otherwise). d_missing, the capacities, DH_EINVAL with the sizes needed and hip_stream are those of
 * dh_store_columns_device, which on an untrimmed handle keeps returning the raw stored values (the JSON text).
 */
int dh_store_beacons_device(dh_store* store, uint64_t first, uint64_t last, size_t sig_stride, size_t prev_stride,
                            uint64_t* d_rounds, uint8_t* d_sigs, uint32_t* d_sig_lens, uint8_t* d_prevs, uint32_t* d_prev_lens,
                            uint8_t* d_deferred, size_t cap_rows, size_t* n_rows_out, uint64_t* d_missing, size_t cap_missing,
                            size_t* n_missing_out, void* hip_stream);
/*
 * dh_store_check_past on an untrimmed handle: the same loop bounds (Last(), the clamp, round < Len(), stop after the
 * first round >= up_to), windows verified in place on the columns above with strides roundup4(max(dh_sig_len, the
 * longest decoded value in the window's leaves)), a window above 64 KiB per row DH_EINVAL. A round is faulty when its
 * record is missing, when its decoded Signature is not dh_sig_len bytes, or when dh_verify_batch_device rejects it
 * with the PreviousSig it stores. Deferred records are skipped and the call then returns DH_DEFERRED instead of DH_OK;
 * a deferred LAST record is DH_EINVAL (Last().Round is its Round field, which only the host decoder reads);
 * DH_ENOBEACON only for an empty bucket.
 *
 * dh_store_deferred: the keys of the deferred records among rounds first..last, ascending (none on a trimmed handle);
 * more than `cap`: DH_EINVAL with *n_out = the number needed.
 */
int dh_store_deferred(dh_store* store, uint64_t first, uint64_t last, uint64_t* out, size_t cap, size_t* n_out);

/*
 * Writing a trimmed store file from columns in device memory: the image of the file that
 * chain/boltdb/trimmed.go:87-107 fills (bucket "beacons", key = round as 8 bytes big-endian, value = the raw
 * signature, leaves packed full: bucket.FillPercent = 1.0). This is a FILE WRITER, not bbolt: no transactions, no
 * update of a live store, no freelist reuse. It serves the two things the reference leaves to a serial Put loop:
 * converting a legacy store, whose format shouldUseTrimmedBolt (chain/boltdb/store.go:82-110) keeps for ever, and
 * acting on CheckPastBeacons the way CorrectPastBeacons does (chain/beacon/sync_manager.go:237-268). The layout is
 * fixed: pages 0 / 1 meta (txid 3 / 2), 2 an empty freelist, 3 the root bucket's leaf, the bucket's leaves from page 4
 * (a record needs 16 + 8 + vsize bytes, a leaf closes when 16 + the sum would pass the page size, a record that alone
 * passes it gets overflow pages), then branch levels of (page_size - 16) / 24 children up to one root.
 *
 * dh_bolt_write_trimmed_device: the primitive. d_rounds / d_rows / d_lens: n rows in the layout
 * dh_store_columns_device and dh_store_beacons_device produce (strictly ascending rounds, value i = d_lens[i] bytes at
 * d_rows + i*row_stride, d_lens[i] <= row_stride; a violation is DH_EINVAL, found on the device before anything is
 * written). page_size: a power of two from 256 to 65536, else DH_EINVAL. image_out: HOST memory of `cap` bytes;
 * *len_out = the size of the image, a multiple of page_size; cap too small: DH_EINVAL with *len_out set and nothing
 * written. n = 0: DH_ENOBEACON (no empty store is written). An image above DRANDHIP_STORE_MAX_BYTES or a failed
 * allocation: DH_ENOMEM. stats_out (nullable) = {rows, leaves, pages}. Work queued on hip_stream is waited for first; the
 * call returns when the image is complete. The call runs as a loop over the windowed writer below, in windows of
 * DRANDHIP_STORE_WRITE_WINDOW rows (read at every call; default and upper bound: the device scan's limit of 16M rows;
 * values below 1 are ignored), so n has no limit of its own; the image does not depend on the window. dh_profile stages:
 * bolt_write_plan, bolt_write_pack, bolt_write_download, and bolt_write_window once per window.
 */
#define DH_PATCH_DELETE 0xFFFFFFFFu
int dh_bolt_write_trimmed_device(const uint64_t* d_rounds, const uint8_t* d_rows, size_t row_stride, const uint32_t* d_lens,
                                 size_t n, uint32_t page_size, uint8_t* image_out, size_t cap, size_t* len_out,
                                 uint64_t stats_out[3], void* hip_stream);
/*
 * dh_store_save_trimmed: the round records of first..last of an open store, of either format, as a trimmed file image.
 * A trimmed handle copies the values as stored, of any length (a compacted or ranged copy); an untrimmed handle writes
 * each canonical record's decoded Signature (chain/boltdb/store.go:143-168 -> trimmed.go:87-107). Elements that are not
 * round records (keys not 8 bytes, nested buckets) are not copied.
 * Patches (CorrectPastBeacons' Put of the refetched rounds, sync_manager.go:237-268): n_patch <= 2^20 rounds, strictly
 * ascending and inside [first, last], else DH_EINVAL; patch i replaces the record of its round or inserts it with the
 * patch_lens[i] <= patch_stride bytes at patch_sigs + i*patch_stride; patch_lens[i] == DH_PATCH_DELETE drops the record.
 * A deferred record in the range that no patch covers: DH_DEFERRED with *len_out = 0 and nothing written; list them
 * with dh_store_deferred, decode them, pass them as patches (or delete them) and call again.
 * The trimmed reader takes the previous signature of round r from the value of round r - 1 (trimmed.go:156-193), while
 * an untrimmed record stored its own. A row taken from a canonical record is UNLINKED when its decoded PreviousSig has
 * nonzero length and the output holds no row for round - 1 or that row's value differs from it in length or bytes:
 * exactly the rounds for which the written file hands a chained verifier another previous signature than the record
 * stored. unlinked_out: those rounds, ascending; more than unlinked_cap: DH_EINVAL with *n_unlinked_out = the number
 * and *len_out = the image size, nothing written. Always empty for a trimmed handle.
 * image_out / cap / len_out / page_size as above. stats_out (nullable) = {rows written, leaves, pages, unlinked, patches
 * that replaced or deleted a record, patches that inserted one}. The call runs as a loop over the windowed writer
 * below: the range is cut at leaf boundaries of the source (dh_store_split) into windows of at most
 * DRANDHIP_STORE_WRITE_WINDOW stored rows (default: what keeps rows + patches of a window within the scan's 16M), so
 * the range has no row limit of its own; more than one window costs a sizing pass over the range first. The image, the
 * unlinked list and the stats do not depend on the window.
 * dh_profile stages: store_save_merge, store_save_plan, store_save_pack, store_save_download, and store_save_window
 * once per window.
 */
int dh_store_save_trimmed(dh_store* store, uint64_t first, uint64_t last, const uint64_t* patch_rounds, const uint8_t* patch_sigs,
                          size_t patch_stride, const uint32_t* patch_lens, size_t n_patch, uint32_t page_size,
                          uint8_t* image_out, size_t cap, size_t* len_out, uint64_t* unlinked_out, size_t unlinked_cap,
                          size_t* n_unlinked_out, uint64_t stats_out[6]);

/*
 * The windowed writer: the same file, written from rows that arrive in windows, with bounded
 * device memory and no row limit on the file (row counts and page ids are 64-bit; the host keeps 16 bytes per leaf).
 * Every leaf is emitted as soon as it is closed, i.e. once a following record is known not to fit; the rows of the open
 * leaf (at most page_size - 24 bytes of records) are carried in the writer to the next window; the branch levels and
 * pages 0-3 are written by dh_bolt_writer_finish.
 * THE FILE INVARIANT: out[0, *len_out) of every append belongs at file offset *file_off_out; the runs of successive
 * appends are contiguous and start at 4 * page_size; the tail of dh_bolt_writer_finish follows the last run; head_out
 * belongs at offset 0; and head || runs || tail is byte for byte the image dh_bolt_write_trimmed_device gives for the
 * concatenated rows, for every split into appends, whatever their strides.
 *
 * dh_bolt_writer_open: page_size as above. dh_bolt_writer_close frees the handle (NULL is ignored). A handle is used by
 * one call at a time; two handles run concurrently. dh_shutdown releases a handle's device memory: every later call on
 * it fails with DH_EINVAL, and dh_bolt_writer_close still frees it.
 *
 * dh_bolt_writer_append_device: n rows in the layout of dh_bolt_write_trimmed_device, at most 16M a call, their rounds
 * above every round appended before. out: HOST memory of `cap` bytes for the pages of the leaves this append closes;
 * *len_out = their size (0 when it closes none); stats_out (nullable) = {rows taken, leaves closed, pages emitted}.
 * n = 0 is DH_OK with *len_out = 0. DH_OK means the rows were taken. NOTHING IS CONSUMED ON FAILURE: with cap too small
 * (cap 0 sizes) DH_EINVAL with *len_out = the size needed; rounds not strictly ascending, inside the append or against
 * the last round appended, or a length above row_stride: DH_EINVAL; a run above DRANDHIP_STORE_MAX_BYTES (which bounds
 * what one call emits, not the file) DH_ENOMEM; in each case the writer is exactly as before the call and a later
 * correct call continues the same file. Work queued on hip_stream is waited for first; the columns are free again when
 * the call returns.
 *
 * dh_bolt_writer_finish: closes the open leaf. tail_out: HOST memory of `cap` bytes for its pages and the branch pages,
 * which belong at *file_off_out; head_out: 4 * page_size bytes of HOST memory for pages 0-3. cap too small (cap 0
 * sizes) or head_out NULL: DH_EINVAL with *len_out = the size needed, nothing consumed. A writer that never received a
 * row: DH_ENOBEACON. stats_out (nullable) = {rows, leaves, pages} of the file, as the one-shot call reports them. After
 * DH_OK the writer takes no further call but dh_bolt_writer_close.
 * dh_profile stages: bolt_write_plan, bolt_write_pack, bolt_write_download per append, bolt_write_window once per append.
 */
typedef struct dh_bolt_writer dh_bolt_writer;
int dh_bolt_writer_open(uint32_t page_size, dh_bolt_writer** out);
int dh_bolt_writer_append_device(dh_bolt_writer* w, const uint64_t* d_rounds, const uint8_t* d_rows, size_t row_stride,
                                 const uint32_t* d_lens, size_t n, uint8_t* out, size_t cap, size_t* len_out,
                                 uint64_t* file_off_out, uint64_t stats_out[3], void* hip_stream);
int dh_bolt_writer_finish(dh_bolt_writer* w, uint8_t* tail_out, size_t cap, size_t* len_out, uint64_t* file_off_out,
                          uint8_t* head_out, uint64_t stats_out[3]);
void dh_bolt_writer_close(dh_bolt_writer* w);
/*
 * dh_store_save_trimmed_append: one round window first..last of an open store, merged with its patches exactly as
 * dh_store_save_trimmed takes them, appended to a writer: a windowed convert or repair. Windows are passed in ascending
 * round order (a window's first written round must pass the writer's last, else DH_EINVAL); one file may take windows
 * of several stores and rows of dh_bolt_writer_append_device. out / cap / len_out / file_off_out as
 * dh_bolt_writer_append_device. The first written row of a window is tested for UNLINKED against the last row the
 * writer received: linked when that row is round - 1 and holds the stored PreviousSig, whichever window or patch it came
 * from. unlinked_out: this window's unlinked rounds, ascending (so the lists of successive windows concatenate
 * ascending). A window that produces no row (an empty range, or everything deleted) is DH_OK with *len_out = 0.
 * Nothing is consumed on failure: DH_DEFERRED, a cap too small (DH_EINVAL, *len_out = the size needed), more than
 * unlinked_cap unlinked rounds (DH_EINVAL, *n_unlinked_out = the number, *len_out = the size needed) and every other
 * refusal leave the writer as before the call. A window holds at most 16M rows and 2^20 patches. stats_out (nullable) =
 * {rows taken, leaves closed, pages emitted, unlinked, patches that replaced or deleted a record, patches that inserted}.
 * The store handle and the writer are both held for the call.
 *
 * dh_store_split: [first, last] cut into n windows at leaf boundaries of the source file, ascending: window i is
 * bounds_out[2i] .. bounds_out[2i + 1] inclusive, the first starts at `first`, the last ends at `last`, and window i + 1
 * starts one above the end of window i, so every round (and every patch) of the range lies in exactly one window. Each
 * window holds at most max(max_rows, rows of its largest leaf) stored rows. cap counts windows; too little room:
 * DH_EINVAL with *n_out = the number needed. first > last: no window. From the open handle's leaf index and counts
 * alone: no device work.
 */
int dh_store_save_trimmed_append(dh_store* store, dh_bolt_writer* w, uint64_t first, uint64_t last, const uint64_t* patch_rounds,
                                 const uint8_t* patch_sigs, size_t patch_stride, const uint32_t* patch_lens, size_t n_patch,
                                 uint8_t* out, size_t cap, size_t* len_out, uint64_t* file_off_out, uint64_t* unlinked_out,
                                 size_t unlinked_cap, size_t* n_unlinked_out, uint64_t stats_out[6]);
int dh_store_split(dh_store* store, uint64_t first, uint64_t last, size_t max_rows, uint64_t* bounds_out, size_t cap, size_t* n_out);

/*
 * Synthetic-chain utilities (test fixtures and benchmark inputs; not part of the verification path):
 * sign n beacons with a 32-byte big-endian secret scalar, sig_i = [sk] H(DigestBeacon(round_i, prev_i)),
 * the mock chain pattern of client/test/result/mock/result.go:84-127; and the matching group key [sk] g.
 * sigs_out: n * dh_sig_len bytes; key_out: dh_key_len bytes.
 */
int dh_sign_batch(int scheme, const uint8_t* sk32, const uint64_t* rounds, const uint8_t* prevs, size_t n,
                  const uint32_t* prev_lens, size_t prev_stride, uint8_t* sigs_out);
int dh_public_key(int scheme, const uint8_t* sk32, uint8_t* key_out);

/*
 * RFC 9380 hash_to_curve (random-oracle encoding, expand_message_xmd with SHA-256) on the device for n arbitrary
 * messages (message i = msgs[msg_off[i] .. msg_off[i+1])) under one DST of 1..255 bytes: group 1 = G1 (SSWU on the
 * 11-isogenous curve), group 2 = G2 (3-isogenous). out: n compressed points (48 / 96 bytes). The general form of the
 * fixed-shape hashing inside the batch kernels (kilic HashToCurve as used by kyber-bls12381's Hash, [ext]); pinned
 * by the RFC 9380 J.9.1 / J.10.1 vectors in tests/kat.py.
 */
int dh_hash_to_curve(int group, const uint8_t* msgs, const uint32_t* msg_off, size_t n, const uint8_t* dst, size_t dst_len,
                     uint8_t* out);

/*
 * Test entry: the per-round kernel of a large local G1-signature batch (decode and hash on one lane, the hash
 * point's inversion carried by the signature's square-root chain) from hash_to_field's outputs on. us: n pairs
 * u0 || u1 as canonical 48-byte big-endian field elements (each < p); sigs: n 48-byte compressed signatures.
 * status_out: n bytes (1 = decoded; no subgroup test); sig_out: n x 96 bytes, sigma as canonical affine x || y (zeros
 * when rejected); hash_out: n x 96 bytes, map_to_curve(u0) + map_to_curve(u1) before cofactor clearing as canonical
 * affine x || y, zeros for the identity.
 */
int dh_g1_round_prep_debug(const uint8_t* us, const uint8_t* sigs, size_t n, uint8_t* status_out, uint8_t* sig_out,
                           uint8_t* hash_out);

/*
 * Test entry: the same kernel in the form that leaves the hash's 11-isogeny to the batch (DRANDHIP_G1_ISO_LATE, the
 * default for such a batch). Same inputs; sig_out and hash_out are read back from the 28-bit arrays the MSM reads:
 * sigma as above, and hash_out the sum swu(u0) + swu(u1) on the isogenous curve E1' (RFC 9380 8.8.1) as canonical
 * affine x || y, before the isogeny; zeros for the identity, whose round is rejected (status_out 0).
 */
int dh_g1_round_prep_late_debug(const uint8_t* us, const uint8_t* sigs, size_t n, uint8_t* status_out, uint8_t* sig_out,
                                uint8_t* hash_out);

/*
 * Test entry: the shape of the last level-0 MSM that a local batch (dh_verify_batch and its kin, not a node batch) ran
 * on the calling thread: the window rows per point set, the sorted-list entries, and whether the a-half and the b-half
 * of the rounds' scalars keyed rows. A large G1-signature batch keys the a-halves alone (DRANDHIP_G1_RLC_HALF, the
 * default): nwin rows, n x nwin entries, half_a = 1, half_b = 0; with the switch at 0, 2 nwin, 2 n x nwin, 1, 1.
 * Zeros before the thread's first such batch. A call split over workers (DRANDHIP_SPLIT) records the chunks that ran on
 * the calling thread.
 */
int dh_msm_level0_shape_debug(uint64_t* rows_per_set, uint64_t* entries, int* half_a, int* half_b);

/*
 * Test entry (test infrastructure, no product path calls it): one field-layer operation per lane, on caller-given
 * operand words, so that the arithmetic headers can be run at the bounds they state (DESIGN.md "Field-layer op kernel"
 * has the op table and the record layout). ops: n opcodes; in: n operand records of in_words 32-bit words (at least
 * 176); out: n result records of out_words words (at least 88), words an operation does not write are zero. All host
 * pointers. n = 0 succeeds; a null pointer with n > 0, an unknown opcode or records too small are DH_EINVAL.
 */
int dh_field_ops_debug(const uint32_t* ops, const uint32_t* in, size_t in_words, size_t n, uint32_t* out, size_t out_words);

/*
 * Test entry (test infrastructure, no product path calls it): the lane-parallel pairing interpreter (k_vm.hip vm_exec)
 * on n records, one 64-lane workgroup each, stopped after `stop` phases; out receives each record's whole slot image,
 * nslots x 16 words (14 limbs of 28 bits and two pad words a slot), so out_words must be nslots x 16.
 * tag 0..7: a committed program, in the order NP1, NP2, ML1, MUL12, FE, NP2C, NP1J, NP2J; phases, nphases, ops, nops and
 *   nslots are ignored (the program's own hold). A record is the program's inputs in INPUT_SLOT order: 12-word
 *   Montgomery values (radix 2^384, below p), so in_words = 12 x inputs; for MUL12 and FE the inputs are VM-form slots
 *   of 16 words, in_words = 16 x inputs.
 * tag -1: the caller's program. phases: 2 nphases words (kind | count << 8, then the phase's first op); ops: nops records
 *   of 32 words in pairing_vm.hpp's layout (the entry appends the 16 pad words and aligns the buffer); a record is the
 *   initial slot image, in_words = nslots x 16. DH_EINVAL, with nothing launched, for: nphases above the largest
 *   committed check program's, nslots 0 or above the check kernels' slot array, a kind above 2, a count above 64, an INV
 *   phase whose count is not 1 or whose op has a second half, more than 15 terms in a half, a first-op word that is not
 *   the running sum of the counts, nops that is not their total, word 16 of a record that is not nb << 16, a non-zero
 *   term word past its half's count, any slot index >= nslots, and a phase in which two ops write one slot or an op
 *   reads a slot the phase writes.
 * Either mode: stop above the program's phase count, a tag outside -1..7, in_words or out_words other than stated, more
 * than 65536 records and a null pointer with n > 0 are DH_EINVAL; n = 0 succeeds. All host pointers.
 */
int dh_vm_debug(int tag, const uint32_t* phases, size_t nphases, const uint32_t* ops, size_t nops, size_t nslots, size_t stop,
                const uint32_t* in, size_t in_words, size_t n, uint32_t* out, size_t out_words);

/*
 * client.RandomData JSON-lines archives on the device: the records the HTTP relays serve
 * (client/random.go:5-10, marshalled through hexjson), one per line:
 *   {"round":367,"randomness":"<64 hex>","signature":"<96|192 hex>","previous_signature":"<192 hex>"}
 * Framing: records are the maximal runs of bytes between '\n' bytes; a last run without a closing '\n' is a record when
 * it is not empty; empty runs are skipped; record index = 0-based ordinal of the non-empty run. A buffer whose first
 * byte outside '\n' is '[' (the JSON-array form) is DH_EINVAL: the caller keeps the host reader.
 * Canonical records are decoded on the device: exactly '{' fields '}', the fields a subsequence of "round":D,
 * "randomness":"H", "signature":"H", "previous_signature":"H" in that order joined by single commas ({} is canonical);
 * D = 1-20 digits, no leading zero, not 0, below 2^64; H = a non-zero even number of characters 0-9a-f. Every other
 * record (and every line above 4096 bytes) is DEFERRED: the device reports its index and decides nothing; the caller's
 * host decoder does.
 *
 * dh_archive_open_ndjson: uploads buf[0, len) (never read outside it), indexes it. The image stays resident until
 * close. Above DRANDHIP_STORE_MAX_BYTES (or 8 GiB): DH_ENOMEM. An empty buffer or one of '\n' bytes only opens with
 * 0 records. A mutex in the handle serialises calls on it; dh_shutdown invalidates it (every call but close DH_EINVAL).
 * dh_archive_stat: {records, deferred, longest line (4097 for every longer one), longest decoded signature, longest
 * previous_signature, longest randomness, tile bytes of the index kernels}.
 * dh_archive_lines: byte offset and length of records first_rec .. first_rec + n_rec - 1 into HOST arrays; n_rec is
 * clamped to the archive here and below.
 * dh_archive_deferred: the indices of the deferred records among them, ascending; more than cap: DH_EINVAL with *n_out
 * = the number.
 * dh_archive_beacons_device: the records' columns in DEVICE memory, in the layout dh_verify_batch_device and
 * dh_bolt_writer_append_device take: rounds, signature rows of sig_stride bytes with their lengths, previous_signature
 * rows (d_prevs / d_prev_lens nullable together), randomness rows of 32 bytes (d_rands / d_rand_lens nullable
 * together), deferred flags. A value that fits its stride is copied whole and zero-padded; otherwise its row is all
 * zero, never a prefix, and the length is still the true one. A deferred record: zero rows, zero lengths, round 0.
 * Strides: positive multiples of 4, at most 1 MiB; at most 16M records per call. *n_out = the rows written.
 * dh_archive_check: verifies the records `window` at a time and writes one status byte per record (HOST memory):
 */
#define DH_AR_DEFERRED 1       /* not canonical: no other bit is set, the call returns DH_DEFERRED */
#define DH_AR_NO_SIGNATURE 2   /* decoded signature length 0 */
#define DH_AR_INVALID 4        /* signature length != dh_sig_len(scheme), or the verifier rejects the record */
#define DH_AR_RANDOMNESS 8     /* randomness present and not SHA-256(signature); informational */
#define DH_AR_SEQUENCE 16      /* round != the predecessor's round + 1 */
#define DH_AR_LINK 32          /* chained scheme: previous_signature != the predecessor's signature */
#define DH_AR_PRED_DEFERRED 64 /* the predecessor is deferred: bits 16 and 32 are left 0 for the caller to decide */
/*
 * The chained scheme verifies each record against its OWN previous_signature. The predecessor of record i is record
 * i - 1 of the archive, across windows; the predecessor of record 0 is the anchor {*anchor_round, anchor_sig} when
 * anchor_round is not NULL, else record 0 has none (bits 16 / 32 / 64 clear). Rows are roundup4(max(dh_sig_len, the
 * longest decoded value)) bytes; above 64 KiB: DH_EINVAL. counts_out = {records checked, deferred, invalid,
 * randomness mismatches, sequence breaks, link breaks}. dh_profile stages: archive_upload, archive_index,
 * archive_stat at open; archive_gather, archive_verify, archive_fold per window.
 */
typedef struct dh_archive dh_archive;
int dh_archive_open_ndjson(const uint8_t* buf, size_t len, dh_archive** out);
int dh_archive_stat(const dh_archive* archive, uint64_t out[7]);
int dh_archive_lines(dh_archive* archive, uint64_t first_rec, size_t n_rec, uint64_t* off_out, uint32_t* len_out);
int dh_archive_deferred(dh_archive* archive, uint64_t first_rec, size_t n_rec, uint64_t* idx_out, size_t cap, size_t* n_out);
int dh_archive_beacons_device(dh_archive* archive, uint64_t first_rec, size_t n_rec, size_t sig_stride, size_t prev_stride,
                              uint64_t* d_rounds, uint8_t* d_sigs, uint32_t* d_sig_lens, uint8_t* d_prevs, uint32_t* d_prev_lens,
                              uint8_t* d_rands, uint32_t* d_rand_lens, uint8_t* d_deferred, size_t* n_out, void* hip_stream);
int dh_archive_check(dh_archive* archive, int scheme, const uint8_t* pk, size_t pk_len, uint64_t first_rec, size_t n_rec,
                     const uint64_t* anchor_round, const uint8_t* anchor_sig, size_t anchor_sig_len, size_t window, uint64_t seed,
                     uint8_t* status_out, uint64_t counts_out[6]);
void dh_archive_close(dh_archive* archive);

/*
 * Protobuf beacon records on the device: the wire form SyncChain streams (BeaconPacket,
 * protobuf/drand/protocol.proto:113-118) and the relays publish (PublicRandResponse, protobuf/drand/api.proto:44-52).
 * A second front end of the dh_archive handle: the caller gives every record's length (a gossip message, a gRPC frame);
 * nothing is framed on the device. Canonical records, what proto.Marshal writes, are decoded on the device:
 *   BeaconPacket       := [0A L bytes] [10 V] [1A L bytes] [22 M Metadata]               prev, round, sig, metadata
 *   PublicRandResponse := [08 V] [12 L bytes] [1A L bytes] [22 L bytes] [2A M Metadata]  round, sig, prev, randomness, metadata
 *   Metadata           := [0A M NodeVersion] [12 L ascii] [1A L bytes]                   node_version, beaconID, chain_hash
 *   NodeVersion        := [08 V32] [10 V32] [18 V32] [22 M ascii]                        major, minor, patch, prerelease
 * fields in this order, each at most once, the record ending exactly at its end; minimal varints; 1 <= V < 2^64,
 * 1 <= V32 < 2^32, L >= 1, M >= 0, ascii = bytes below 0x80. A record of 0 bytes is canonical (round 0, nothing else).
 * Every other record, and every record above 4096 bytes, is DEFERRED, as for JSON lines.
 *
 * dh_archive_open_pb: records are buf[rec_off[i], rec_off[i] + rec_len[i]), offsets ascending, records not overlapping;
 * rec_off NULL = packed from 0, the lengths summing to len. A record outside the buffer: DH_EINVAL. Size rules as
 * dh_archive_open_ndjson. The offsets are summed on the host and uploaded: no index kernel runs, stat[6] is 0. Every
 * other dh_archive_* call works on the handle as on a JSON-lines one (dh_archive_lines gives the payload offset and the
 * true length); kind 1 has no randomness (lengths 0).
 * dh_archive_kind: 0 JSON lines, DH_PB_BEACON_PACKET, DH_PB_PUBLIC_RAND.
 * dh_archive_set_beacon_id: the ID dh_archive_check compares with (tryNode, chain/beacon/sync_manager.go:385-389): a
 * record whose metadata is present and whose beaconID differs, byte for byte, gets DH_AR_BEACON_ID. id NULL unsets it
 * (the state after open): the bit is never set, as on a JSON-lines handle. counts_out keeps its six entries.
 * dh_pb_frame_delimited (host only, no device needed, off the hot path): walks varint-delimited records (minimal
 * prefixes below 2^32) and gives each payload's offset and length. It stops at the first prefix that is malformed or
 * whose payload runs past len and still returns DH_OK, *consumed_out telling where; a cut stream is an ordinary event.
 * More than cap records: DH_EINVAL with *n_out = the count.
 * dh_pb_encode_device: rows of the verifier's columns (DEVICE memory, rows 4-byte aligned, strides multiples of 4) ->
 * beaconToProto's BeaconPacket each (chain/beacon/convert.go:9-16): previous_signature when its length is not 0, the
 * round when not 0, the signature when its length is not 0, then metadata {beaconID}: beacon_id NULL writes none,
 * length 0 writes 22 00. kind must be DH_PB_BEACON_PACKET. d_prevs / d_prev_lens NULL together. delimited: a varint
 * length before every packet. d_out NULL: the sizing call, only *len_out and d_rec_len_out (nullable, DEVICE, the
 * packet lengths without prefix) are produced. cap < *len_out: DH_EINVAL with *len_out set. A row whose packet would
 * exceed 4096 bytes, or whose length passes its stride: DH_EINVAL naming the row. 4 GiB or more in all, or more than
 * 16M rows: DH_EINVAL, split the call. The call waits for hip_stream first and returns with the bytes written.
 */
#define DH_AR_BEACON_ID 128 /* metadata present and its beaconID is not the one set with dh_archive_set_beacon_id */
#define DH_PB_BEACON_PACKET 1
#define DH_PB_PUBLIC_RAND 2
int dh_archive_open_pb(int kind, const uint8_t* buf, size_t len, const uint64_t* rec_off, const uint32_t* rec_len, size_t n_rec,
                       dh_archive** out);
int dh_archive_kind(const dh_archive* archive);
int dh_archive_set_beacon_id(dh_archive* archive, const uint8_t* id, size_t id_len);
int dh_pb_frame_delimited(const uint8_t* buf, size_t len, uint64_t* off_out, uint32_t* len_out, size_t cap, size_t* n_out,
                          size_t* consumed_out);
int dh_pb_encode_device(int kind, const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_lens,
                        const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, size_t n, const uint8_t* beacon_id,
                        size_t beacon_id_len, int delimited, uint8_t* d_out, size_t cap, uint32_t* d_rec_len_out, size_t* len_out,
                        void* hip_stream);

/*
 * The records a node or relay serves to the public, encoded on the device. Rows of the verifier's
 * columns (DEVICE memory, as for dh_pb_encode_device) -> one record each, carrying randomness = SHA-256(signature)
 * (crypto.RandomnessFromSignature):
 *   DH_ENC_RANDOM_DATA_JSON  client.RandomData through hexjson (http/server.go:336-342, cmd/relay-s3/main.go:127-141):
 *                            {"round":D,"randomness":"H","signature":"H","previous_signature":"H"}, lowercase hex
 *   DH_ENC_PUBLIC_RAND_PB    proto.Marshal of drand.PublicRandResponse (core/convert.go:15-22):
 *                            [08 V] [12 L sig] [1A L prev] [22 L rand] [2A M metadata], minimal varints
 * fields in this order, each left out when empty (round 0, a length of 0).
 * d_rands NULL: every record carries SHA-256 of its sig_len signature bytes (of the empty string for length 0), computed
 * in the encode kernel and stored nowhere else; else rows of 32 bytes (4-byte aligned), copied as given:
 * dh_verify_batch_device's d_rand_out. d_keep (nullable, one byte per row): a row whose byte is 0 writes nothing, no
 * newline and no prefix, has d_rec_len_out 0 and is neither measured nor refused; dh_verify_batch_device's
 * d_verdict_out plugs in. metadata (protobuf only; not NULL with the JSON form: DH_EINVAL): the caller's marshalled
 * common.Metadata, at most 4096 bytes, copied opaquely after 2A and its length; NULL writes no field, length 0 writes
 * 2A 00. flags: DH_ENC_NEWLINE (JSON only) writes '\n' after every record, DH_ENC_DELIMITED (protobuf only) a minimal
 * varint length before every record; the other combination or an unknown bit: DH_EINVAL.
 * Everything else is dh_pb_encode_device's: d_prevs / d_prev_lens NULL together, rows 4-byte aligned, strides positive
 * multiples of 4 up to 1 MiB, d_out NULL the sizing call, cap < *len_out DH_EINVAL with *len_out set, a kept row whose
 * record would exceed 4096 bytes (without prefix and newline) or whose length passes its stride DH_EINVAL naming the
 * row, 4 GiB or more in all or more than 16M rows DH_EINVAL (split the call), n == 0 DH_OK with length 0. The argument
 * refusals are decided before the device is touched. The call waits for hip_stream first and returns with the bytes
 * written. dh_profile stage: serve_encode (k_serve_size, k_serve_encode).
 */
#define DH_ENC_RANDOM_DATA_JSON 1
#define DH_ENC_PUBLIC_RAND_PB 2
#define DH_ENC_NEWLINE 1
#define DH_ENC_DELIMITED 2
int dh_rand_encode_device(int form, const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride, const uint32_t* d_sig_lens,
                          const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens, const uint8_t* d_rands, const uint8_t* d_keep,
                          size_t n, const uint8_t* metadata, size_t metadata_len, int flags, uint8_t* d_out, size_t cap,
                          uint32_t* d_rec_len_out, size_t* len_out, void* hip_stream);

/*
 * One chain from many unordered sources. The n candidates are rows of verifier columns in DEVICE
 * memory, in any order, from any number of sources, the layout dh_archive_beacons_device, dh_store_beacons_device and
 * dh_store_columns_device write; the call knows no source kind. Rules, in order (store.assemble_host restates them):
 *   1. a candidate whose d_skip byte (nullable column) is not 0 is SKIPPED;
 *   2. round 0, a round at or below *anchor_round, or above *up_to (each nullable) is STALE and never verified;
 *   3. a candidate that repeats an earlier live candidate of its round (the same lengths and bytes of the signature
 *      and, chained, of the previous_signature) is a DUPLICATE: not verified, it takes the INVALID bit of that one;
 *   4. every other candidate is a representative, verified once, `window` rows at a time through
 *      dh_verify_batch_device (the chained scheme against its OWN previous_signature): INVALID when its signature
 *      length is not dh_sig_len(scheme), when a value is longer than its stride, or when the verifier rejects it;
 *   5. per round the valid representative lowest in input order is CHOSEN; another valid one with other bytes is a
 *      CONFLICT (reported, never resolved);
 *   6. the chosen rows in ascending round order are the output: *m_out whole, zero-padded rows at sig_stride /
 *      prev_stride (room for n rows; d_prevs_out / d_prev_lens_out nullable together, chained only), d_src_out = the
 *      input position of each, d_flags_out = DH_AS_GAP when the round is not the row before's + 1, DH_AS_LINK (chained,
 *      consecutive rounds) when its own previous_signature is not that row's signature; the row before row 0 is the
 *      anchor when there is one;
 *   7. the gaps are the maximal ranges of missing rounds from anchor + 1 (without an anchor: from the first chosen
 *      round) to the last chosen round, or to *up_to when given: gap_first_out / gap_last_out (HOST, gap_cap entries);
 *      more than gap_cap: DH_EINVAL with *n_gaps_out = the number and everything else written.
 * Copies are collapsed against the first 16 candidates of their round only (ASSEMBLE_LOOKBACK): a later copy is
 * verified again, is not a CONFLICT and is marked DUPLICATE when it is valid; the output never depends on it.
 * DRANDHIP_ASSEMBLE_DEDUPE=0 (read at every call) makes every candidate a representative.
 * status_out: HOST, n bytes of DH_AS_* bits. counts_out = {candidates, skipped, stale, representatives verified,
 * invalid, duplicates, conflicts, chosen, missing rounds (saturating), link breaks}. n = 0 is DH_OK; more than 16M
 * candidates, a stride that is not a positive multiple of 4 up to 1 MiB or a row that is not 4-byte aligned is
 * DH_EINVAL. Blocking and thread-safe: a call owns its stream and buffers; it waits for hip_stream first. The same
 * input gives the same output, byte for byte, on every run. dh_profile stages: assemble_sort, assemble_class,
 * assemble_verify, assemble_select.
 */
#define DH_AS_CHOSEN 1
#define DH_AS_DUPLICATE 2
#define DH_AS_INVALID 4
#define DH_AS_STALE 8
#define DH_AS_SKIPPED 16
#define DH_AS_CONFLICT 32
#define DH_AS_GAP 1  /* output-row flags */
#define DH_AS_LINK 2
int dh_assemble_device(int scheme, const uint8_t* pk, size_t pk_len, const uint64_t* d_rounds, const uint8_t* d_sigs, size_t sig_stride,
                       const uint32_t* d_sig_lens, const uint8_t* d_prevs, size_t prev_stride, const uint32_t* d_prev_lens,
                       const uint8_t* d_skip, size_t n, const uint64_t* anchor_round, const uint8_t* anchor_sig, size_t anchor_sig_len,
                       const uint64_t* up_to, size_t window, uint64_t seed, uint64_t* d_rounds_out, uint8_t* d_sigs_out,
                       uint32_t* d_sig_lens_out, uint8_t* d_prevs_out, uint32_t* d_prev_lens_out, uint32_t* d_src_out, uint8_t* d_flags_out,
                       size_t* m_out, uint8_t* status_out, uint64_t* gap_first_out, uint64_t* gap_last_out, size_t gap_cap,
                       size_t* n_gaps_out, uint64_t counts_out[10], void* hip_stream);

/*
 * Test entry (test infrastructure, no product path calls it): the stable sort of dh_assemble_device alone. keys: n u64
 * keys, perm_out: n positions, both HOST; perm_out[j] = the position of the key that sorts j-th, equal keys in input
 * order. n = 0 succeeds; more than 16M keys is DH_EINVAL.
 */
int dh_sort_rounds_debug(const uint64_t* keys, size_t n, uint32_t* perm_out);

/*
 * Live kernel timing: when enabled, every device stage of the verification path is bracketed by HIP
 * events on the stream it is launched on; dh_profile_read writes a JSON object
 * {"stage": {"count": c, "total_ms": t}, ...} into buf (returns the full length). dh_profile resets.
 */
int dh_profile(int enable);
int dh_profile_read(char* buf, size_t cap);

/* Human-readable description of the last error on the calling thread ("" if none). */
const char* dh_last_error_string(void);

/* Build / device description, e.g. "libdrandhip gfx950 ..." */
const char* dh_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DRANDHIP_H */
