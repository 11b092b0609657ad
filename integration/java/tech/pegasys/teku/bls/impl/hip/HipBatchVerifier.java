/*
 * Public entry of the GPU batch path for callers outside the SPI: the
 * gossip service's batch with its failure path in one device call
 * (tbls_batch_verify_each, include/tekubls.h), used by
 * HipAggregatingSignatureVerificationService.  Mirror and tests:
 * teku_amd/service.py (_hip_batch_each), tests/test_gpu_configs.py
 * test_config4_16k_through_service.
 */
package tech.pegasys.teku.bls.impl.hip;

import java.util.List;
import org.apache.tuweni.bytes.Bytes;
import tech.pegasys.teku.bls.BLSPublicKey;
import tech.pegasys.teku.bls.BLSSignature;
import tech.pegasys.teku.bls.impl.BlsException;

public final class HipBatchVerifier {
  private HipBatchVerifier() {}

  /* Library devices (tbls_device_count): the service runs one worker per device. */
  public static int deviceCount() {
    return HipLoader.INSTANCE.isPresent() ? Math.max(1, TekuBlsHip.deviceCount()) : 1;
  }

  /*
   * The library's hash-point memo (tbls_msg_memo_configure): rows per device,
   * 0 turns it off.  Gossip batches repeat a slot's signing roots
   * (AggregatingSignatureVerificationService.java:187-227); with the memo every
   * batch staged afterwards hashes only the messages whose H(m) no earlier
   * batch left on the device.  Verdicts are unchanged.  Process state.
   */
  public static void configureHashMemo(final int rows) {
    if (!HipLoader.INSTANCE.isPresent()) {
      return;
    }
    final int rc = TekuBlsHipMemo.msgMemoConfigure(Math.min(Math.max(rows, 0), TekuBlsHipMemo.MAX_ROWS));
    if (rc != 0) {
      throw new BlsException("tbls_msg_memo_configure failed: " + rc);
    }
  }

  /* {pairs whose H(m) came from a row, messages hashed, flushes, rows in use} (tbls_msg_memo_stats) */
  public static long[] hashMemoStats(final boolean reset) {
    final int[] words = new int[8];
    final int rc = TekuBlsHipMemo.msgMemoStats(words, reset);
    if (rc != 0) {
      throw new BlsException("tbls_msg_memo_stats failed: " + rc);
    }
    return new long[] {
      TekuBlsHipMemo.stat(words, 0), TekuBlsHipMemo.stat(words, 1), TekuBlsHipMemo.stat(words, 2), TekuBlsHipMemo.stat(words, 3)
    };
  }

  /*
   * BLS.batchVerify(keys, messages, signatures) over all sets as one
   * randomized device batch (BLS.java:230-336); when it fails, okPerSet[i] =
   * BLS.fastAggregateVerify(set i) (BLS.java:185-207), settled on the devices
   * that ran the batch from its own Miller work.  Returns the batch verdict
   * (okPerSet all true when it passes).  A set with no keys is false and makes
   * the batch false.  nGpus: at most that many devices (0 = every idle one);
   * a caller with more batches waiting passes 1.
   */
  public static boolean batchVerifyEach(final List<List<BLSPublicKey>> keys, final List<Bytes> messages,
                                        final List<BLSSignature> signatures, final int nGpus, final boolean[] okPerSet) {
    return batchVerifyEach(keys, messages, signatures, nGpus, okPerSet, false);
  }

  /*
   * The same with groupMessages: the batch first runs through
   * tbls_batch_verify_grouped -- one hash and one pairing per distinct message
   * where the library finds that grouping pays, the verdict of the ungrouped
   * batch (attestations of one slot sign the same AttestationData).  A batch
   * that passes is done; one that fails goes on to tbls_batch_verify_each,
   * which gives the per-set verdicts as without the flag.
   */
  public static boolean batchVerifyEach(final List<List<BLSPublicKey>> keys, final List<Bytes> messages,
                                        final List<BLSSignature> signatures, final int nGpus, final boolean[] okPerSet,
                                        final boolean groupMessages) {
    return batchVerifyEach(keys, messages, signatures, nGpus, okPerSet, groupMessages, false);
  }

  /*
   * groupMessages with groupSettle: the batch is one call,
   * tbls_batch_verify_each_grouped -- the grouped batch, and when it fails the
   * per-set verdicts settled from the grouped pass's own work (nothing staged,
   * decoded or hashed again), the verdicts of tbls_batch_verify_each.
   */
  public static boolean batchVerifyEachGrouped(final List<List<BLSPublicKey>> keys, final List<Bytes> messages,
                                               final List<BLSSignature> signatures, final int nGpus, final boolean[] okPerSet) {
    return batchVerifyEach(keys, messages, signatures, nGpus, okPerSet, true, true);
  }

  private static boolean batchVerifyEach(final List<List<BLSPublicKey>> keys, final List<Bytes> messages,
                                        final List<BLSSignature> signatures, final int nGpus, final boolean[] okPerSet,
                                        final boolean groupMessages, final boolean groupSettle) {
    final int n = keys.size();
    if (messages.size() != n || signatures.size() != n || okPerSet.length < n) {
      throw new IllegalArgumentException("Different collection sizes");
    }
    int k = 0;
    int m = 0;
    for (int i = 0; i < n; i++) {
      k += keys.get(i).size();
      m += messages.get(i).size();
    }
    final byte[] pks = new byte[48 * k];
    final int[] nPks = new int[n];
    final byte[] msgs = new byte[m];
    final int[] msgOff = new int[n + 1];
    final byte[] sigs = new byte[96 * n];
    final long[] rand = new long[n];
    int kk = 0;
    for (int i = 0; i < n; i++) {
      final List<BLSPublicKey> ks = keys.get(i);
      for (BLSPublicKey pk : ks) {
        System.arraycopy(pk.toBytesCompressed().toArrayUnsafe(), 0, pks, 48 * kk++, 48);
      }
      nPks[i] = ks.size();
      final byte[] msg = messages.get(i).toArrayUnsafe();
      System.arraycopy(msg, 0, msgs, msgOff[i], msg.length);
      msgOff[i + 1] = msgOff[i] + msg.length;
      System.arraycopy(signatures.get(i).toBytesCompressed().toArrayUnsafe(), 0, sigs, 96 * i, 96);
      rand[i] = HipBLS12381.nextBatchRandomMultiplier();
    }
    final int[] ok = new int[1];
    if (groupMessages && groupSettle) {
      final int[] eachGrouped = new int[n];
      final int rcEach = TekuBlsHipGroupedEach.batchVerifyEachGrouped(pks, nPks, msgs, msgOff, sigs, rand, nGpus, 0, ok, eachGrouped);
      if (rcEach != TekuBlsHip.SUCCESS) {
        throw new BlsException("GPU BLS backend: batchVerifyEachGrouped failed, code " + rcEach);
      }
      for (int i = 0; i < n; i++) {
        okPerSet[i] = eachGrouped[i] == 1;
      }
      return ok[0] == 1;
    }
    if (groupMessages) {
      final int rcGrouped = TekuBlsHipGrouped.batchVerifyGrouped(pks, nPks, msgs, msgOff, sigs, rand, nGpus, 0, ok);
      if (rcGrouped == TekuBlsHip.SUCCESS && ok[0] == 1) {
        java.util.Arrays.fill(okPerSet, 0, n, true);
        return true;
      } // a failed batch, an empty key list or an error: the per-set call decides
    }
    final int[] each = new int[n];
    final int rc = TekuBlsHip.batchVerifyEach(pks, nPks, msgs, msgOff, sigs, rand, nGpus, ok, each);
    if (rc != TekuBlsHip.SUCCESS) {
      throw new BlsException("GPU BLS backend: batchVerifyEach failed, code " + rc);
    }
    for (int i = 0; i < n; i++) {
      okPerSet[i] = each[i] == 1;
    }
    return ok[0] == 1;
  }

  /*
   * Makes `validatorIndices` (indices into the resident key table, duplicates
   * allowed) the committee of `slot` (0..3) on every device.  A node loads the
   * current and the next sync committee into two slots at each period boundary.
   */
  public static void loadCommittee(final int slot, final int[] validatorIndices) {
    final int rc = TekuBlsHipCommittee.committeeLoad(slot, validatorIndices);
    if (rc == TekuBlsHip.BAD_ARGUMENT) {
      throw new IllegalArgumentException("Committee slot, size or validator index out of range, or no key table");
    }
    if (rc != TekuBlsHip.SUCCESS) {
      throw new BlsException("GPU BLS backend: committeeLoad failed, code " + rc);
    }
  }

  /*
   * BLS.fastAggregateVerify(participants' keys, message, signature) per set
   * (BLS.java:185-207) for sets given as the SyncAggregate participation
   * bitvectors over the committee of committeeSize members in `slot`
   * (BlockProcessorAltair.java:234-267): bitvectors.get(i) has
   * (committeeSize + 7) / 8 bytes, member k participates iff bit k % 8 of byte
   * k / 8 is set.  A set without participants is false: the caller keeps
   * eth2FastAggregateVerify's infinity-signature case.
   */
  public static boolean[] fastAggregateVerifyCommittee(final int slot, final int committeeSize, final List<Bytes> bitvectors,
                                                       final List<Bytes> messages, final List<BLSSignature> signatures) {
    final int n = bitvectors.size();
    final int row = (committeeSize + 7) / 8;
    if (messages.size() != n || signatures.size() != n) {
      throw new IllegalArgumentException("Different collection sizes");
    }
    int m = 0;
    for (int i = 0; i < n; i++) {
      if (bitvectors.get(i).size() != row) {
        throw new IllegalArgumentException("Bitvector length does not match the committee");
      }
      m += messages.get(i).size();
    }
    final byte[] bits = new byte[row * n];
    final byte[] msgs = new byte[m];
    final int[] msgOff = new int[n + 1];
    final byte[] sigs = new byte[96 * n];
    for (int i = 0; i < n; i++) {
      System.arraycopy(bitvectors.get(i).toArrayUnsafe(), 0, bits, row * i, row);
      final byte[] msg = messages.get(i).toArrayUnsafe();
      System.arraycopy(msg, 0, msgs, msgOff[i], msg.length);
      msgOff[i + 1] = msgOff[i] + msg.length;
      System.arraycopy(signatures.get(i).toBytesCompressed().toArrayUnsafe(), 0, sigs, 96 * i, 96);
    }
    final int[] each = new int[n];
    final int rc = TekuBlsHipCommittee.fastAggregateVerifyManyBits(slot, committeeSize, bits, msgs, msgOff, sigs, each);
    if (rc == TekuBlsHip.BAD_ARGUMENT) {
      throw new IllegalArgumentException("Empty or reloaded committee slot, or a set bit past the committee");
    }
    if (rc != TekuBlsHip.SUCCESS) {
      throw new BlsException("GPU BLS backend: fastAggregateVerifyManyBits failed, code " + rc);
    }
    final boolean[] ok = new boolean[n];
    for (int i = 0; i < n; i++) {
      ok[i] = each[i] == 1;
    }
    return ok;
  }
}
