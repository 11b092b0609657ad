/*
 * tekubls.h -- C ABI of libtekubls_hip.so, the MI355X (gfx950) BLS12-381
 * signature-verification backend for Teku.
 *
 * Drop-in boundary: a new implementation of Teku's SPI
 *   tech.pegasys.teku.bls.impl.BLS12381
 *   (infrastructure/bls/src/main/java/tech/pegasys/teku/bls/impl/BLS12381.java:34-157)
 * next to BlstBLS12381 (impl/blst/BlstBLS12381.java), installed with
 * BLS.setBlsImplementation (bls/BLS.java:51-53).  Each entry point below names
 * the reference interface it replaces.  The JNI glue and the Java SPI classes a
 * maintainer would add are shown in INTEGRATION.md.
 *
 * Conventions
 *  - All points use the ZCash compressed encoding: G1 = 48 bytes, G2 = 96 bytes.
 *  - Inputs are caller-owned host buffers, copied on entry; outputs go to
 *    caller-provided buffers (SURVEY.md 8(b) "Ownership").
 *  - Return value: a TBLS_* status.  Codes 0..7 mirror blst's BLST_ERROR enum
 *    (the set jblst surfaces to BlstBLS12381); TBLS_DEVICE_ERROR is added.
 *    The JNI layer maps them to BlsException / booleans exactly as
 *    BlstBLS12381 does (BlstBLS12381.java:131-137, 169-188).
 *  - Thread-safe and re-entrant: per-device submission lock, per-call staging.
 *  - No CPU fallback: without a HIP device every call returns
 *    TBLS_DEVICE_ERROR.
 */
#ifndef TEKUBLS_H
#define TEKUBLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  TBLS_SUCCESS = 0,
  TBLS_BAD_ENCODING = 1,
  TBLS_POINT_NOT_ON_CURVE = 2,
  TBLS_POINT_NOT_IN_GROUP = 3,
  TBLS_AGGR_TYPE_MISMATCH = 4,
  TBLS_VERIFY_FAIL = 5,
  TBLS_PK_IS_INFINITY = 6,
  TBLS_BAD_SCALAR = 7,
  TBLS_DEVICE_ERROR = 8,
  TBLS_BAD_ARGUMENT = 9, /* e.g. an empty public-key list inside a batch */
};

/* Library lifecycle.  n_devices = -1 uses every visible device.
 * Replaces BlstLoader.INSTANCE (impl/blst/BlstLoader.java:32-51): a loader
 * that gets an error here yields Optional.empty().
 * flags: TBLS_INIT_SHARE_DEVICES makes n_devices (<= 32) library devices over
 * the visible hardware devices round-robin, each with its own streams,
 * workspace and lock -- so a one-GPU host runs the multi-device paths
 * (sharding, the record gather, per-shard settling) for tests; the gather of
 * devices that share hardware uses peer copies instead of RCCL. */
enum { TBLS_INIT_SHARE_DEVICES = 1u };
int tbls_init(int n_devices, uint32_t flags);
void tbls_shutdown(void);
int tbls_device_count(void);

/* BlstPublicKey.fromBytes + isValid (BlstPublicKey.java:38-45, 93-104):
 * TBLS_SUCCESS iff the key decodes, is not infinity and is in G1. */
int tbls_pk_validate(const uint8_t pk[48]);

/* BlstSignature.fromBytes + isInGroup (BlstSignature.java:35-47, 147-149). */
int tbls_sig_validate(const uint8_t sig[96], int* is_inf);

/* ---- host decoding: BlstPublicKey.fromBytes / BlstSignature.fromBytes ----
 * (BlstPublicKey.java:38-45, BlstSignature.java:35-47: P1_Affine / P2_Affine
 * deserialization = blst_p1/p2_uncompress, no subgroup check).  Decided on
 * the CALLER'S THREAD with no device call and no tbls_init needed: flags,
 * x < p, the curve equation has a root, x != 0.  Returns TBLS_SUCCESS,
 * TBLS_BAD_ENCODING, TBLS_POINT_NOT_ON_CURVE or TBLS_POINT_NOT_IN_GROUP (x = 0,
 * blst's "(0, +-2) is not in group"); *is_inf (nullable) = 1 for the
 * canonical infinity encoding.  The SPI's fromBytes throws BlsException on any
 * non-success code; the subgroup check stays with isInGroup / isValid
 * (tbls_sig_validate, tbls_pk_validate, the *_many forms) and the batch. */
int tbls_pk_decode(const uint8_t pk[48], int* is_inf);
int tbls_sig_decode(const uint8_t sig[96], int* is_inf);
/* The same for n items (codes[i], is_inf[i] nullable), spread over up to 16
 * host threads: one call for a whole gossip batch of fresh objects. */
int tbls_pk_decode_many(const uint8_t* pks, size_t n, uint8_t* codes, uint8_t* is_inf);
int tbls_sig_decode_many(const uint8_t* sigs, size_t n, uint8_t* codes, uint8_t* is_inf);

/* Call counters since load (or the last reset): out[0] batch pipelines queued,
 * out[1] single-object device validations (tbls_pk_validate /
 * tbls_sig_validate), out[2] helper device calls (hash, sign, aggregate,
 * *_many, single verifications), out[3] per-set verdict passes
 * (tbls_verify_each chunks), out[4] final exponentiations, out[5] points
 * decoded on the host, out[6] failed batches settled from their own Miller
 * values.  Entries past 7 are 0.  reset != 0 zeroes them after reading.
 * Observability for services (what a workload cost the device). */
int tbls_stats(uint64_t* out, size_t n, int reset);

/* BLS12381.aggregatePublicKeys -> BlstPublicKey.aggregate
 * (BLS12381.java:95, BlstPublicKey.java:55-71): k >= 1; any invalid key makes
 * the result the infinity key.  Decode failures -> TBLS_BAD_ENCODING etc. */
int tbls_aggregate_pks(const uint8_t* pks, size_t k, uint8_t out[48]);

/* BLS12381.aggregateSignatures -> BlstSignature.aggregate
 * (BLS12381.java:105-106, BlstSignature.java:57-68): group check per input;
 * k = 0 gives the infinity signature. */
int tbls_aggregate_sigs(const uint8_t* sigs, size_t k, uint8_t out[96]);

/* P2.hash_to (BlstBLS12381.java:59, HashToCurve.java:24-31). */
int tbls_hash_to_g2(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dlen, uint8_t out[96]);

/* BlstBLS12381.sign (BlstBLS12381.java:48-63); sk big-endian, 0 < sk < r. */
int tbls_sign(const uint8_t sk[32], const uint8_t* msg, size_t len, const uint8_t* dst, size_t dlen, uint8_t out[96]);

/* BlstSecretKey.derivePublicKey (BlstSecretKey.java:75-78); sk = 0 -> infinity. */
int tbls_sk_to_pk(const uint8_t sk[32], uint8_t out[48]);

/* BlstBLS12381.verify -> blst core_verify(pk, hash=true)
 * (BlstBLS12381.java:65-78).  *ok = 1 iff valid.  Decode errors are returned
 * as codes (the facade turns them into false, BLS.java:99-101). */
int tbls_verify(const uint8_t pk[48], const uint8_t* msg, size_t len, const uint8_t sig[96], const uint8_t* dst,
                size_t dlen, int* ok);

/* One signature set: n_pks keys (48 B each, contiguous), one message, one
 * signature.  The unit of BLS.prepareBatchVerify (BLS.java:353-368). */
typedef struct {
  const uint8_t* pks;
  uint32_t n_pks;
  const uint8_t* msg;
  uint32_t msg_len;
  const uint8_t* sig;
} tbls_set;

typedef struct {
  double total_ms;     /* API entry -> result, host clock */
  double device_ms;    /* sum over devices of the batch's kernel pipeline, HIP events (a settle after a failed batch is in total_ms only) */
  uint32_t n_devices;  /* devices used */
} tbls_timing;

/* Randomized batch verification: BLS.batchVerify(pks, msgs, sigs) for n >= 2
 * through prepareBatchVerify/completeBatchVerify (BLS.java:275-336,
 * BlstBLS12381.java:112-189).  rand[i] in [1, 2^64] as BlstBLS12381
 * .nextBatchRandomMultiplier (l.191-195) -- the caller owns the RNG.  n_gpus:
 * at most that many devices (0 = all initialised devices); the batch goes to
 * the least-loaded device, or is sharded over several idle ones when it has at
 * least 2 x tbls_shard_min() sets, or 2 x tbls_shard_knee() sets when every
 * device is idle (tbls_place_plan); each device produces one Fp12
 * partial product, gathered for one final exponentiation.  *ok = 1 iff every set is valid and the pairing product is
 * 1.  n == 0 -> *ok = 0 (BLS.java:240-241).  A set with n_pks == 0 ->
 * TBLS_BAD_ARGUMENT (BlstPublicKey.aggregate checkArgument, l.56).
 * With a key table loaded (tbls_pk_table_load), keys that the table holds are
 * taken from it by their bytes instead of being decompressed again; the
 * verdict is the same. */
int tbls_batch_verify(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, int* ok, tbls_timing* t);

/* ---- device-resident validator public-key table ----
 * Teku memoizes each key's decompression and validity per BLSPublicKey object
 * (BlstPublicKey.fromBytes / isInfinity / isInGroup, BlstPublicKey.java:38-45,
 * 74-75, 93-104) and looks keys up by validator index
 * (BeaconStateAccessors.getValidatorPubKey, spec/.../helpers/
 * BeaconStateAccessors.java:78-97).  tbls_pk_table_load makes that memo
 * device-resident: the K keys are decompressed and validated once on every
 * device (96-byte affine + status per key in HBM) and batches name keys by
 * index, so no key bytes travel and no key is decompressed per call.
 * Replaces any previous table.  codes (nullable, K bytes): per-key status as
 * tbls_pk_validate (TBLS_SUCCESS, TBLS_PK_IS_INFINITY, ...).
 *
 * The load also keeps the K compressed keys on every device and builds an
 * index over their bytes (an open-addressing hash table keyed by a seed drawn
 * at each load; a reload rebuilds it from empty).  Callers that name keys by
 * their bytes -- tbls_batch_verify, tbls_batch_verify_each, tbls_verify_each,
 * tbls_fast_aggregate_verify_many, tbls_dev_batch_partial -- then have each
 * key looked up first: a key whose 48 bytes equal a table key's takes the
 * table's point and status, any other key is decompressed and checked as
 * without a table.  The results are the same either way: the table's entry
 * was computed from the same bytes by the same kernel.  (Single-key batches
 * of up to 512 sets decode their keys inside their one key kernel and do not
 * look them up.)  TBLS_PK_LOOKUP=0 in the environment, read by tbls_init,
 * turns the index off: no keys are kept, no index is built, byte keys are
 * always decompressed and tbls_pk_table_resolve finds no index. */
int tbls_pk_table_load(const uint8_t* pks, size_t K, uint8_t* codes);
size_t tbls_pk_table_size(void);

/* Drop the table, its index and every resident committee on every device
 * (tbls_pk_table_size() becomes 0; the lookup counters are zeroed). */
int tbls_pk_table_clear(void);

/* The table index of each of n keys given by their bytes, in one device pass:
 * idx_out[i] is an index whose table key equals pks[48 i .. 48 i + 48) byte for
 * byte (of equal table keys, any one), or 0xFFFFFFFF when the table holds no
 * such key.  An integration memoizes the index in its public-key object and
 * moves to the index entries (tbls_batch_verify_idx, ...).  No table (or no
 * index, TBLS_PK_LOOKUP=0) -> TBLS_BAD_ARGUMENT.  Not counted in
 * tbls_pk_lookup_stats. */
int tbls_pk_table_resolve(const uint8_t* pks, size_t n, uint32_t* idx_out);

/* out[0] = keys the batch key stages took from the table, out[1] = keys they
 * looked up and did not find (and decompressed), since the last table load or
 * reset, summed over the devices; each device's counters are read under its
 * lock after its stream is synchronised.  reset != 0 zeroes them after
 * reading.  Both stay 0 without a table and with TBLS_PK_LOOKUP=0. */
int tbls_pk_lookup_stats(uint64_t out[2], int reset);

/* ---- learned key cache ----
 * Teku memoizes a key's decompression and its validity per key object
 * (BLSPublicKey.java:113-118, BlstPublicKey.java:74-75), so a node decodes
 * each validator key once.  The library does the same for callers that pass
 * key bytes and load no table: every device keeps a byte-keyed cache of the
 * keys its key stages decompressed and found valid (TBLS_SUCCESS), with their
 * affine points, and the same entries as above look a key up -- in the
 * loaded table's index first, then in the cache -- before decompressing it.
 * A hit takes the point computed from the same 48 bytes by the same code, so
 * every result is bit for bit what it is without the cache.  The infinity
 * key and invalid keys are never cached: they are decoded each time and fail
 * with the same codes.  By-index and committee entries never touch the cache,
 * and single-key batches of up to 512 sets neither read nor extend it.
 *
 * The capacity is fixed per process: TBLS_PK_CACHE_KEYS rows per device (read
 * by tbls_init; default 2,097,152, about 320 MB per device, allocated by the
 * first batch that looks keys up).  Nothing is evicted: when every row is
 * taken, further keys are decompressed per call and counted as refused.
 * A device on which the cache cannot be allocated goes on without one.
 * TBLS_PK_CACHE=0 turns the cache off (TBLS_PK_LOOKUP=0 does too).
 * tbls_pk_table_load and tbls_pk_table_clear leave the cache as it is: its
 * rows depend on key bytes only; a key in both is taken from the table.
 *
 * tbls_pk_cache_stats: out[0] = keys taken from the cache, out[1] = keys
 * learned, out[2] = valid keys a full cache refused, since the process began,
 * the last tbls_pk_cache_clear or the last reset; out[3] = rows in use (not
 * reset; a batch that holds a new key twice may leave a row unused).  Summed
 * over the devices, each read under its lock after its stream is synchronised.
 * tbls_pk_cache_clear forgets every learned key and zeroes the counters. */
int tbls_pk_cache_stats(uint64_t out[4], int reset);
int tbls_pk_cache_clear(void);

/* ---- per-key comb rows ----
 * For every key it keeps -- a row of the learned cache, a key of the loaded
 * table -- the device also keeps 15 affine multiples of the key (a 4-tooth
 * fixed-base comb, 1,440 bytes), computed once: by the batch that learns the
 * key, or by tbls_pk_table_load.  A single-key set of a large batch (one that
 * runs the two-wave key kernel: 32,768 sets or more per device, in the batch
 * entries and in tbls_verify_each alike; TBLS_W2_MIN, read once per process,
 * moves that threshold for all two-wave kernels and is meant for tests and
 * tuning) whose key has such a row takes [r] pk from it in 15
 * doublings and at most 16 additions instead of 62 and about 24 plus a
 * per-call table; the point is the same, so every result is bit for bit what
 * it is without the rows.  A batch never reads a row it builds itself.
 *
 * TBLS_PK_COMB=0 (read by tbls_init) turns the rows off.  TBLS_PK_COMB_KEYS
 * caps the cache's comb rows per device (default: every cache row; 3.0 GB at
 * 2,097,152 rows): cache rows beyond the cap never get one and are multiplied
 * as before.  A device on which a region cannot be allocated goes on without
 * it.  tbls_pk_cache_clear forgets the cache's comb rows with its keys;
 * tbls_pk_table_load and tbls_pk_table_clear rebuild and drop the table's.
 *
 * tbls_pk_comb_stats: out[0] = sets whose [r] pk came from a comb row, out[1]
 * = rows built for learned keys, out[2] = rows built for table keys, since the
 * process began or the last reset; out[3] = the caches' comb-row capacity (0:
 * none).  Summed over the devices as tbls_pk_cache_stats is. */
int tbls_pk_comb_stats(uint64_t out[4], int reset);

/* ---- hash-point memo ----
 * The service verifies gossip in batches of a few hundred sets whose signing
 * roots repeat from batch to batch: every attester of a committee signs the
 * same AttestationData, and a failed batch is verified again in halves
 * (AggregatingSignatureVerificationService.java:187-227).  H(m) =
 * hash_to_G2(m, DST) depends on the message bytes and the fixed Ethereum DST
 * alone (HashToCurve.java:24-31), so each device can keep the points it has
 * computed: a resident array of rows, each an affine G2 point with its skip
 * byte, and on the host an index from message bytes to rows.  With the memo
 * on, the host entries tbls_batch_verify*, tbls_batch_verify_each* (their
 * _idx and _grouped forms, and the settling of a failed batch included),
 * tbls_verify_each and tbls_fast_aggregate_verify_many* resolve every
 * set's message before they stage a shard, hash only the messages that are
 * neither resident nor repeated inside the shard, and give every pair its
 * point with one copy kernel.  A point from a row is the 192 bytes the same
 * kernels wrote for the same message, so every verdict is bit for bit what it
 * is without the memo.
 *
 * Messages of more than 64 bytes are hashed every time and never resident
 * (Teku's signing roots are 32 bytes).  When a shard brings more new messages
 * than there are free rows, the device's whole memo is flushed and refilled
 * from that shard.  A shard of more than 16,384 sets bypasses the memo: there
 * the host-side resolving costs more than any measured gain.
 * Calls with a DST of their own (tbls_verify,
 * tbls_aggregate_verify, tbls_sign*, tbls_hash_to_g2) and the
 * device-resident entries tbls_dev_batch_partial* never touch the memo.
 *
 * tbls_msg_memo_configure: rows per device, capped at 1,048,576 (about 200 MB
 * per device, allocated by the first batch that resolves); 0 turns the memo
 * off.  Forgets everything learned and zeroes the counters; takes effect for
 * batches staged afterwards.  TBLS_MSG_MEMO=rows in the environment, read by
 * tbls_init, does the same; the memo is off by default.  A device on which
 * the rows cannot be allocated goes on without a memo.
 * tbls_msg_memo_stats: out[0] = pairs whose point came from a row learned by
 * an earlier call, out[1] = messages hashed, out[2] = flushes, since the last
 * configure or reset; out[3] = rows in use (not reset).  Summed over the
 * devices, each read under its lock.
 * tbls_msg_memo_clear forgets every learned point; the counters stay. */
int tbls_msg_memo_configure(uint32_t rows);
int tbls_msg_memo_stats(uint64_t out[4], int reset);
int tbls_msg_memo_clear(void);

/* A signature set whose keys are table indices (the unit of
 * BLS.prepareBatchVerify, BLS.java:353-368, with keys by validator index). */
typedef struct {
  const uint32_t* key_idx;
  uint32_t n_pks;
  const uint8_t* msg;
  uint32_t msg_len;
  const uint8_t* sig;
} tbls_set_idx;

/* tbls_batch_verify with keys from the table; same semantics (an invalid
 * table key makes its set invalid, BlstPublicKey.aggregate l.58-65).  An
 * index >= tbls_pk_table_size() -> TBLS_BAD_ARGUMENT. */
int tbls_batch_verify_idx(const tbls_set_idx* sets, size_t n, const uint64_t* rand, int n_gpus, int* ok, tbls_timing* t);

/* fastAggregateVerify per set (BLS.java:185-207, BlstSignature.java:125-129):
 * ok_per_set[i] in {0,1}; an empty key list gives 0.  One batched device pass
 * (= tbls_verify_each on one device). */
int tbls_fast_aggregate_verify_many(const tbls_set* sets, size_t n, int* ok_per_set);

/* tbls_fast_aggregate_verify_many with keys from the table (BLS.java:185-207
 * over keys looked up by validator index, BeaconStateAccessors.java:78-97;
 * aggregation as BlstPublicKey.aggregate, BlstPublicKey.java:55-71): no key
 * bytes travel and no key is decompressed.  An empty key list gives 0; a set
 * naming an invalid table key gives 0; an index >= tbls_pk_table_size(), or no
 * table, -> TBLS_BAD_ARGUMENT.  One device. */
int tbls_fast_aggregate_verify_many_idx(const tbls_set_idx* sets, size_t n, int* ok_per_set);

/* ---- resident sync committees ----
 * A sync committee is one fixed list of validator indices for a whole period
 * (256 epochs; the same validator may appear more than once), and every
 * SyncAggregate carries a participation bitvector over it.  The reference
 * walks the committee, tests each bit and gathers the participants' keys
 * (BlockProcessorAltair.processSyncAggregate, BlockProcessorAltair.java:
 * 234-267) for BLS.fastAggregateVerify (BLS.java:185-207).
 * tbls_committee_load stores the index list in `slot` on every device beside
 * its key table, with the mask of members whose table key is invalid and the
 * sum of the valid members' keys (BlstPublicKey.aggregate,
 * BlstPublicKey.java:55-71), so that a nearly full set costs the few absent
 * keys.  Loading a slot replaces it; tbls_pk_table_load empties every slot.
 * TBLS_BAD_ARGUMENT: slot >= TBLS_COMMITTEE_SLOTS, size == 0 or
 * > TBLS_COMMITTEE_MAX, no table, an index >= tbls_pk_table_size(). */
#define TBLS_COMMITTEE_SLOTS 4
#define TBLS_COMMITTEE_MAX 2048
int tbls_committee_load(uint32_t slot, const uint32_t* key_idx, uint32_t size);
uint32_t tbls_committee_size(uint32_t slot); /* 0: empty slot */

/* One SyncAggregate-shaped set: bits is an SSZ bitvector of (size + 7) / 8
 * bytes over the committee; member i participates iff
 * (bits[i / 8] >> (i % 8)) & 1. */
typedef struct {
  const uint8_t* bits;
  const uint8_t* msg;
  uint32_t msg_len;
  const uint8_t* sig;
} tbls_set_bits;

/* ok_per_set[s] = BLS.fastAggregateVerify(participants' keys in committee
 * order, msg, sig) (BlockProcessorAltair.java:234-267, BLS.java:185-207,
 * BlstPublicKey.java:55-71): no participant gives 0, a participating member
 * with an invalid key gives 0 (an absent one does not matter), an aggregate
 * key equal to infinity gives 0.  A set bit at a position >= size, or an empty
 * slot, -> TBLS_BAD_ARGUMENT.  One device.  (eth2FastAggregateVerify's special
 * case -- no participants with the infinity signature is true -- sits above
 * BLS.fastAggregateVerify in the reference and stays with the caller.) */
int tbls_fast_aggregate_verify_many_bits(uint32_t slot, const tbls_set_bits* sets, size_t n, int* ok_per_set);

/* Per-set verdicts of a whole batch in one pass:
 * ok_per_set[i] = BLS.fastAggregateVerify(sets[i]) (BLS.java:185-207).
 * Replaces the recursive halving + per-task SIMPLE.verify fallback of
 * AggregatingSignatureVerificationService.batchVerifySignatures
 * (statetransition/.../signatures/AggregatingSignatureVerificationService.java:
 * 188-227) after a failed randomized batch.  Chunks of 65536 sets are spread
 * over at most n_gpus devices (0 = all), the least-loaded first. */
int tbls_verify_each(const tbls_set* sets, size_t n, int n_gpus, int* ok_per_set);

/* The service's batch with its failure path in one call: tbls_batch_verify
 * over the sets (*ok), and when it fails, every set's verdict
 * ok_per_set[i] = BLS.fastAggregateVerify(sets[i]) (BLS.java:185-207) settled
 * from the batch's own work on the devices that ran it -- per-set Miller
 * values from the batch's G2 lines, group tests (product + final
 * exponentiation) over 256- and 16-set groups, then single sets -- instead of
 * a second full pass (tbls_verify_each) or the reference's recursive halving
 * (AggregatingSignatureVerificationService.java:206-233).  When the batch
 * passes, every set with keys gets 1.  A set with n_pks == 0 gets 0 and makes
 * *ok 0 (it is left out of the batch).  rand as tbls_batch_verify. */
int tbls_batch_verify_each(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, int* ok, int* ok_per_set, tbls_timing* t);

/* ---- batched deserialization and aggregation ----
 * Gossip decoding validates every key / signature it sees (lazy
 * BLSSignature.getSignature, BLSSignature.java:83-87; the eth reference
 * tests' deserialization_G1/G2 executors), and aggregators sum signature
 * groups (BLS.aggregate from AggregateAttestationBuilder.java:74 and
 * SyncCommitteeMessagePool.java:200).  One device pass for all items:
 * codes[i] as tbls_pk_validate / tbls_sig_validate (is_inf nullable). */
int tbls_pk_validate_many(const uint8_t* pks, size_t n, uint8_t* codes);
int tbls_sig_validate_many(const uint8_t* sigs, size_t n, uint8_t* codes, uint8_t* is_inf);
/* Group g = sigs[off[g], off[g+1]) (96 B each) -> out[96 g] with
 * tbls_aggregate_sigs semantics; status[g] = first failing code, 0 = ok
 * (then out is meaningless).  An empty group gives the infinity signature. */
int tbls_aggregate_sigs_many(const uint8_t* sigs, const uint32_t* off, size_t groups, uint8_t* out, int* status);

/* aggregateVerify (BLS.java:144-170, BlstSignature.java:104-122): n distinct
 * (pk, msg) pairs against one aggregate signature. */
int tbls_aggregate_verify(const uint8_t* pks, const uint8_t* const* msgs, const uint32_t* msg_lens, size_t n,
                          const uint8_t sig[96], int* ok);

/* ---- device-resident batch (inputs already in HBM; used by bench.py) ----
 * All pointers are device pointers on `device`; `stream` is a hipStream_t (or
 * NULL for the library's stream).  Produces the device's partial record
 * (576-byte Fp12 product incl. the (-g1, sum r_i sig_i) pair, then a uint32
 * count of invalid sets) at `partial_out` (580 bytes, device memory). */
typedef struct {
  const uint8_t* pks;      /* K * 48 */
  const uint32_t* pk_off;  /* n + 1 offsets into pks (in keys) */
  uint32_t n_keys;         /* K */
  const uint8_t* msgs;     /* concatenated messages */
  const uint32_t* msg_off; /* n + 1 byte offsets */
  const uint8_t* sigs;     /* n * 96 */
  const uint64_t* rand;    /* n */
  uint32_t n;
} tbls_dev_batch;

#define TBLS_PARTIAL_BYTES 580

int tbls_dev_batch_partial(int device, const tbls_dev_batch* b, void* stream, void* partial_out);

/* tbls_dev_batch_partial with keys from `device`'s resident table: b->pks is
 * ignored and key_idx (device memory, b->n_keys entries, addressed through
 * b->pk_off) indexes the table.  No table -> TBLS_BAD_ARGUMENT. */
int tbls_dev_batch_partial_idx(int device, const tbls_dev_batch* b, const uint32_t* key_idx, void* stream, void* partial_out);

/* Same as tbls_dev_batch_partial, also returning the per-stage device time
 * (HIP events on `stream`) in stage_ms[7]: pk decompress, set pk
 * aggregation+[r], signature decode+G2 check+[r], hash_to_G2, G2 sum, Miller
 * loops, Fp12 product.  Blocks until the partial is ready. */
int tbls_dev_batch_partial_timed(int device, const tbls_dev_batch* b, void* stream, void* partial_out, float* stage_ms);

/* Profiling variant: every stage runs alone on `stream` (no stage overlap),
 * so stage_ms[7] are exclusive kernel times (the roofline's denominators). */
int tbls_dev_batch_stage_profile(int device, const tbls_dev_batch* b, void* stream, void* partial_out, float* stage_ms);

/* The Miller-accumulator plan the library uses for a batch of n sets of one
 * key (introspection for benchmarks and tuning; no device work): *per = pairs
 * per accumulator thread, *nseg = loop segments per pair (1: unsegmented),
 * *split = 1 when the split line / accumulator kernels run (0: one-workgroup
 * wave Miller loops for small batches).  Always TBLS_SUCCESS. */
int tbls_acc_plan(uint32_t n, uint32_t* per, uint32_t* nseg, int* split);

/* ---- Grouped batches: one hash_to_G2 and one pairing per distinct message ----
 * Attestations of one slot sign the same AttestationData, so a service batch
 * (AggregatingSignatureVerificationService.java:187-227) carries few distinct
 * signing roots.  The batch equation of BLS.batchVerify (BLS.java:275-336)
 * collapses over sets that share a message,
 *   prod_i e(r_i apk_i, H(m_i)) = prod_g e(sum_{i in g} r_i apk_i, H(m_g)),
 * an equality in GT: the verdict is exactly the ungrouped one for the same
 * randomizers.  With m distinct messages the pass runs m hashes and m + 64
 * Miller loops (the signature side is always the 64-pair bucket sum). */
enum { TBLS_GROUP_FORCE = 1u };

/* tbls_batch_verify over message groups (BLS.java:275-336,
 * AggregatingSignatureVerificationService.java:187-227): *ok and the return
 * code equal tbls_batch_verify's on the same arguments (n = 0, empty key
 * lists, decode failures included).  Messages are grouped by length and
 * bytes, per device shard.  A shard of n sets with m distinct messages runs
 * the grouped pass when grouping pays (tbls_group_plan), and with
 * TBLS_GROUP_FORCE in flags whenever m < n; otherwise, and always when m == n,
 * it runs tbls_batch_verify's pass. */
int tbls_batch_verify_grouped(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, uint32_t flags, int* ok, tbls_timing* t);

/* tbls_batch_verify_idx over message groups (BLS.java:275-336,
 * AggregatingSignatureVerificationService.java:187-227): verdict and return
 * code equal tbls_batch_verify_idx's (an index past the table ->
 * TBLS_BAD_ARGUMENT). */
int tbls_batch_verify_idx_grouped(const tbls_set_idx* sets, size_t n, const uint64_t* rand, int n_gpus, uint32_t flags, int* ok,
                                  tbls_timing* t);

/* tbls_batch_verify_each over message groups (BLS.java:185-207,275-336,
 * AggregatingSignatureVerificationService.java:187-233): *ok, ok_per_set[] and
 * the return code equal tbls_batch_verify_each's on the same arguments (n = 0,
 * sets with n_pks == 0 -- verdict 0, left out, *ok 0 -- and decode failures
 * included).  Placement, sharding and grouping as tbls_batch_verify_grouped.
 * When the batch fails, a shard that ran the grouped pass settles its sets'
 * verdicts from that pass's own work on its device -- the sets' [r] apk, the
 * decoded signatures, the messages' hash points: nothing is staged, decoded or
 * hashed again -- as the reference never re-decodes a task when it bisects a
 * failed batch (l.206-233); a shard that ran ungrouped settles as in
 * tbls_batch_verify_each.  Of several shards only those whose own record
 * fails settle. */
int tbls_batch_verify_each_grouped(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, uint32_t flags, int* ok, int* ok_per_set,
                                   tbls_timing* t);

/* tbls_dev_batch_partial (key_idx NULL) or tbls_dev_batch_partial_idx over
 * message groups, always grouped (BLS.java:275-336,
 * AggregatingSignatureVerificationService.java:187-227).  b->msgs and
 * b->msg_off (n_msgs + 1 offsets) hold the n_msgs distinct messages; grp_off
 * (n_msgs + 1 words) and grp_sets (b->n words), device memory, list each
 * message's sets: message g is signed by sets grp_sets[grp_off[g] ..
 * grp_off[g + 1]).  Every set appears in exactly one list.  The record is the
 * one tbls_dev_batch_partial writes: its product has the same final
 * exponentiation and its invalid-set count is the same.  Needs
 * 0 < n_msgs < b->n (every message distinct: tbls_dev_batch_partial), else
 * TBLS_BAD_ARGUMENT. */
int tbls_dev_batch_partial_grouped(int device, const tbls_dev_batch* b, const uint32_t* key_idx, uint32_t n_msgs, const uint32_t* grp_off,
                                   const uint32_t* grp_sets, void* stream, void* partial_out);

/* What the grouped host entries do with a shard of n sets and n_msgs distinct
 * messages (BLS.java:275-336, AggregatingSignatureVerificationService.java:
 * 187-227; introspection, no device work).  *grouped: 0 the ungrouped pass
 * whatever the flags (n_msgs == 0 or n_msgs >= n); 1 the grouped pass under
 * TBLS_GROUP_FORCE only; 2 the grouped pass without the flag as well
 * (n >= group_min and 100 n_msgs <= percent n; TBLS_GROUP_MIN="min[,percent]"
 * in the environment overrides the built-in thresholds).  *n_pairs: the
 * Miller loops of the grouped pass (n_msgs + 64) when *grouped is not 0, else
 * of the ungrouped pass.  Always TBLS_SUCCESS. */
int tbls_group_plan(uint32_t n, uint32_t n_msgs, int* grouped, uint32_t* n_pairs);

/* Device placement of a batch (introspection for tests and tuning; no device
 * work), the function tbls_batch_verify / tbls_verify_each / the single-call
 * entries use (tb_lib.hip place_plan): n sets (n_pks[i] keys
 * each; NULL = one key each) over n_devices devices with load[d] batches in
 * flight (NULL = all idle) are sharded over
 *   G = min(idle devices, n_devices capped by n_gpus > 0, max(1, n / shard_min_sets))
 * devices (shard_min_sets = 0: every allowed idle device) -- idle ones only,
 * ties broken round-robin from rr, in ascending order in dev_out[0..G) (the
 * first is the gather root); with no idle device, the least-loaded one --
 * with contiguous shards balanced by key count: device dev_out[k] gets sets
 * [cut_out[k], cut_out[k+1]) (cut_out: G + 1 entries).  When EVERY device is
 * idle, shard_knee_sets (if nonzero and smaller) replaces shard_min_sets: a
 * lone batch on an idle node shards down to the latency knee (a lone
 * 16,384-set batch: 4 devices of 4,096).  Returns G >= 1, or
 * -TBLS_BAD_ARGUMENT.  A concurrent caller of the live library sees the
 * devices other batches hold as loaded, so N service workers with
 * config-4-sized batches land on N different devices, one each
 * (AggregatingSignatureVerificationService.java:121-132, 202-205); a service
 * that has more batches waiting passes n_gpus = 1. */
int tbls_place_plan(size_t n, const uint32_t* n_pks, int n_devices, int n_gpus, const int* load, uint32_t rr, uint32_t shard_min_sets,
                    uint32_t shard_knee_sets, int* dev_out, size_t* cut_out);
/* The live shard_min_sets (32768) and shard_knee_sets (4096); TBLS_SHARD_MIN =
 * "min[,knee]" overrides them (a lone min also caps the knee at min). */
uint32_t tbls_shard_min(void);
uint32_t tbls_shard_knee(void);

/* Multiply g partial records (device memory, contiguous) and run the final
 * exponentiation: *ok = 1 iff no invalid set and the product is 1. */
int tbls_dev_final_verify(int device, const void* partials, uint32_t g, void* stream, int* ok);

/* Asynchronous form for a pipelined service (the final exponentiation of one
 * batch overlapping the next batch's stages): queues the same work on
 * `stream` and writes the verdict (1 / 0) to *ok_dev in DEVICE memory;
 * returns without synchronizing.  The kernel reads the records in place and
 * writes nothing but *ok_dev, so calls may overlap freely on any streams; the
 * caller orders `stream` after the work that wrote the records (an event) and
 * keeps the records untouched until the work on `stream` has run.  Replaces
 * the synchronous completeBatchVerify tail (BlstBLS12381.java:184-189) for
 * services that keep several batches in flight. */
int tbls_dev_final_verify_async(int device, const void* partials, uint32_t g, void* stream, int* ok_dev);

/* ---- batched generation of synthetic workloads (sk big-endian, 32 B) ---- */
int tbls_sk_to_pk_many(const uint8_t* sks, size_t n, uint8_t* out /* n*48 */);
int tbls_sign_many(const uint8_t* sks, const uint8_t* msgs, const uint32_t* msg_off /* n+1 */, size_t n, const uint8_t* dst,
                   size_t dlen, uint8_t* out /* n*96 */);

#ifdef __cplusplus
}
#endif

#endif /* TEKUBLS_H */
