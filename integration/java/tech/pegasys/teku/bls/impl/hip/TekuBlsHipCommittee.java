/*
 * Native entry points of the sync-committee calls of libtekubls_hip.so
 * (include/tekubls.h: tbls_fast_aggregate_verify_many_idx,
 * tbls_committee_load, tbls_fast_aggregate_verify_many_bits), bound by
 * integration/native/tekubls_committee_jni.c.  As TekuBlsHip: every method
 * returns the library status code (TBLS_*), outputs go to the caller's
 * arrays, and no Java memory is referenced after a call returns.
 */
package tech.pegasys.teku.bls.impl.hip;

final class TekuBlsHipCommittee {
  static final int SLOTS = 4; // TBLS_COMMITTEE_SLOTS
  static final int MAX_SIZE = 2048; // TBLS_COMMITTEE_MAX

  private TekuBlsHipCommittee() {}

  /* BLS.fastAggregateVerify per set with keys by validator index into the
   * resident table (TekuBlsHip.pkTableLoad): keyIdx holds sum(nPks) indices,
   * messages concatenated with msgOff[n + 1], sigs n * 96 bytes, okPerSet[n]. */
  static native int fastAggregateVerifyManyIdx(int[] keyIdx, int[] nPks, byte[] msgs, int[] msgOff, byte[] sigs,
                                               int[] okPerSet); // tbls_fast_aggregate_verify_many_idx

  /* the committee's validator indices (duplicates allowed) into slot 0..3 */
  static native int committeeLoad(int slot, int[] keyIdx); // tbls_committee_load

  /* n sets over the committee of `size` members in `slot`: bits holds n SSZ
   * bitvectors of (size + 7) / 8 bytes, concatenated */
  static native int fastAggregateVerifyManyBits(int slot, int size, byte[] bits, byte[] msgs, int[] msgOff, byte[] sigs,
                                                int[] okPerSet); // tbls_fast_aggregate_verify_many_bits
}
