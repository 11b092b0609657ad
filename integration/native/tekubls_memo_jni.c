/*
 * JNI glue of TekuBlsHipMemo (integration/java/.../hip/TekuBlsHipMemo.java)
 * onto the hash-point memo of include/tekubls.h: its rows per device, its
 * counters, and forgetting what it learned.  Same conventions as
 * tekubls_jni.c: every argument is validated before the library is called --
 * a negative row count, a NULL or short output array; a failed check returns
 * TBLS_BAD_ARGUMENT without calling the library, and the counters reach the
 * caller's array only when the library succeeded.
 *
 * Build beside tekubls_jni.c, into the same libtekubls_jni.so.
 */
#include <jni.h>
#include <stdint.h>
#include "tekubls.h"

#define JNAME(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipMemo_##n

/* tbls_msg_memo_configure */
JNIEXPORT jint JNICALL JNAME(msgMemoConfigure)(JNIEnv* env, jclass c, jint rows) {
  (void)env;
  (void)c;
  if (rows < 0) return TBLS_BAD_ARGUMENT;
  return tbls_msg_memo_configure((uint32_t)rows);
}

/* tbls_msg_memo_stats: out gets the four 64-bit counters as eight words, counter i in out[2 i] (low) and out[2 i + 1] (high) */
JNIEXPORT jint JNICALL JNAME(msgMemoStats)(JNIEnv* env, jclass c, jintArray out, jboolean reset) {
  (void)c;
  if (!out || (*env)->GetArrayLength(env, out) < 8) return TBLS_BAD_ARGUMENT;
  uint64_t v[4] = {0, 0, 0, 0};
  const int rc = tbls_msg_memo_stats(v, reset ? 1 : 0);
  if (rc != TBLS_SUCCESS) return rc;
  jint w[8];
  for (int i = 0; i < 4; i++) {
    w[2 * i] = (jint)(uint32_t)(v[i] & 0xffffffffu);
    w[2 * i + 1] = (jint)(uint32_t)(v[i] >> 32);
  }
  (*env)->SetIntArrayRegion(env, out, 0, 8, w);
  return (*env)->ExceptionCheck(env) ? TBLS_BAD_ARGUMENT : TBLS_SUCCESS;
}

/* tbls_msg_memo_clear */
JNIEXPORT jint JNICALL JNAME(msgMemoClear)(JNIEnv* env, jclass c) {
  (void)env;
  (void)c;
  return tbls_msg_memo_clear();
}
