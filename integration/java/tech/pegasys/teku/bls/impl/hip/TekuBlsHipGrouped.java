/*
 * Native entry point of the grouped batch of libtekubls_hip.so
 * (include/tekubls.h: tbls_batch_verify_grouped), bound by
 * integration/native/tekubls_grouped_jni.c.  As TekuBlsHip: the method returns
 * the library status code (TBLS_*), outputs go to the caller's arrays, and no
 * Java memory is referenced after a call returns.
 */
package tech.pegasys.teku.bls.impl.hip;

final class TekuBlsHipGrouped {
  /** TBLS_GROUP_FORCE: group whenever a message repeats, not only where grouping pays. */
  static final int GROUP_FORCE = 1;

  private TekuBlsHipGrouped() {}

  /* TekuBlsHip.batchVerify's arguments and verdict, with one hash and one
   * pairing per distinct message where the library finds that grouping pays
   * (BLS.java:275-336, AggregatingSignatureVerificationService.java:187-227) */
  static native int batchVerifyGrouped(byte[] pks, int[] nPks, byte[] msgs, int[] msgOff, byte[] sigs, long[] rand,
                                       int nGpus, int flags, int[] ok); // tbls_batch_verify_grouped
}
