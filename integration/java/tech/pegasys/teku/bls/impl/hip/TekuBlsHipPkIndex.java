/*
 * Native entry points of the key table's byte index of libtekubls_hip.so
 * (include/tekubls.h: tbls_pk_table_resolve, tbls_pk_table_clear), bound by integration/native/tekubls_pkindex_jni.c.  As
 * TekuBlsHip: every method returns the library status code (TBLS_*), outputs
 * go to the caller's arrays, and no Java memory is referenced after a call
 * returns.
 */
package tech.pegasys.teku.bls.impl.hip;

final class TekuBlsHipPkIndex {
  /** The answer for a key the table does not hold (0xFFFFFFFF as an int). */
  static final int MISS = -1;

  private TekuBlsHipPkIndex() {}

  /* pks: n * 48 bytes; idxOut[i] = a table index whose key has the bytes of key
   * i, or MISS.  HipPublicKey memoizes the answer (INTEGRATION.md). */
  static native int pkTableResolve(byte[] pks, int[] idxOut); // tbls_pk_table_resolve

  /* drop the table, its index and the committees on every device */
  static native int pkTableClear(); // tbls_pk_table_clear
}
