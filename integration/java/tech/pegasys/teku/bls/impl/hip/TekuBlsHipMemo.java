/*
 * Native entry points of the hash-point memo of libtekubls_hip.so
 * (include/tekubls.h: tbls_msg_memo_configure, tbls_msg_memo_stats,
 * tbls_msg_memo_clear), bound by integration/native/tekubls_memo_jni.c.  As
 * TekuBlsHip: every method returns the library status code (TBLS_*), outputs
 * go to the caller's arrays, and no Java memory is referenced after a call
 * returns.
 */
package tech.pegasys.teku.bls.impl.hip;

final class TekuBlsHipMemo {
  /** The most rows per device the library takes (more is capped). */
  static final int MAX_ROWS = 1 << 20;

  private TekuBlsHipMemo() {}

  /* rows per device of the memo (0: off); forgets everything learned; for
   * batches staged afterwards.  rows < 0 is a bad argument. */
  static native int msgMemoConfigure(int rows); // tbls_msg_memo_configure

  /* out[0..8): four 64-bit counters as pairs of words, low then high (stat()
   * joins them): pairs whose H(m) came from a row, messages hashed, flushes,
   * rows in use, summed over the devices; reset zeroes the first three */
  static native int msgMemoStats(int[] out, boolean reset); // tbls_msg_memo_stats

  /** Counter i of a msgMemoStats answer. */
  static long stat(final int[] out, final int i) {
    return (out[2 * i] & 0xffffffffL) | ((long) out[2 * i + 1] << 32);
  }

  /* forget every learned hash point on every device */
  static native int msgMemoClear(); // tbls_msg_memo_clear
}
