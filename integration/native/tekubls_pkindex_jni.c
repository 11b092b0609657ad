/*
 * JNI glue of TekuBlsHipPkIndex (integration/java/.../hip/
 * TekuBlsHipPkIndex.java) onto the key table's byte index of
 * include/tekubls.h: the table index of keys given by their bytes, and dropping the
 * table.  Same conventions as tekubls_jni.c: arrays
 * are copied in with Get*ArrayRegion, and every argument is validated before
 * the library sees a pointer into a copy -- NULL arrays, a key array that is
 * not a whole number of 48-byte keys, an output array shorter than the keys;
 * a failed check returns TBLS_BAD_ARGUMENT (a failed allocation
 * TBLS_DEVICE_ERROR) without calling the library.
 *
 * Build beside tekubls_jni.c, into the same libtekubls_jni.so.
 */
#include <jni.h>
#include <stdlib.h>
#include <string.h>
#include "tekubls.h"

#define JNAME(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipPkIndex_##n

static jsize alen(JNIEnv* env, jarray a) { return a ? (*env)->GetArrayLength(env, a) : -1; }

/* tbls_pk_table_resolve: pks holds n keys of 48 bytes; idxOut gets n indices */
JNIEXPORT jint JNICALL JNAME(pkTableResolve)(JNIEnv* env, jclass c, jbyteArray pks, jintArray idxOut) {
  (void)c;
  const jsize nb = alen(env, pks), no = alen(env, idxOut);
  if (nb < 0 || no < 0 || nb % 48 != 0 || no < nb / 48) return TBLS_BAD_ARGUMENT;
  const jsize n = nb / 48;
  uint8_t* k = (uint8_t*)malloc(nb ? (size_t)nb : 1);
  uint32_t* idx = (uint32_t*)malloc(sizeof(uint32_t) * (n ? (size_t)n : 1));
  int rc = TBLS_SUCCESS;
  if (!k || !idx) {
    rc = TBLS_DEVICE_ERROR;
  } else {
    if (nb) (*env)->GetByteArrayRegion(env, pks, 0, nb, (jbyte*)k);
    if ((*env)->ExceptionCheck(env)) {
      rc = TBLS_BAD_ARGUMENT;
    } else {
      rc = tbls_pk_table_resolve(k, (size_t)n, idx);
      if (rc == TBLS_SUCCESS && n) (*env)->SetIntArrayRegion(env, idxOut, 0, n, (const jint*)idx);
    }
  }
  free(idx);
  free(k);
  return rc;
}

/* tbls_pk_table_clear */
JNIEXPORT jint JNICALL JNAME(pkTableClear)(JNIEnv* env, jclass c) {
  (void)env;
  (void)c;
  return tbls_pk_table_clear();
}
