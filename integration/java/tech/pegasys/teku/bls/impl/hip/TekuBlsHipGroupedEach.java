/*
 * Native entry point of the grouped batch with its failure path of
 * libtekubls_hip.so (include/tekubls.h: tbls_batch_verify_each_grouped), bound
 * by integration/native/tekubls_grouped_each_jni.c.  As TekuBlsHip: the method
 * returns the library status code (TBLS_*), outputs go to the caller's arrays,
 * and no Java memory is referenced after a call returns.
 */
package tech.pegasys.teku.bls.impl.hip;

final class TekuBlsHipGroupedEach {
  private TekuBlsHipGroupedEach() {}

  /* TekuBlsHip.batchVerifyEach's arguments and verdicts over message groups
   * (flags as TekuBlsHipGrouped.batchVerifyGrouped): when the grouped batch
   * fails, okPerSet comes from the grouped pass's own work -- no task is decoded
   * or hashed again, as the reference never re-decodes one when it bisects
   * (BLS.java:185-207,275-336, AggregatingSignatureVerificationService.java:187-233) */
  static native int batchVerifyEachGrouped(byte[] pks, int[] nPks, byte[] msgs, int[] msgOff, byte[] sigs, long[] rand,
                                           int nGpus, int flags, int[] ok, int[] okPerSet); // tbls_batch_verify_each_grouped
}
