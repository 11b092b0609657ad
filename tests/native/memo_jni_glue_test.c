/* Unit test of the hash-point memo's JNI glue (integration/native/tekubls_memo_jni.c)
 * against a recording fake of the C ABI entries it calls and the stub JNI
 * environment of jni_stub/jni.h: malformed Java arguments must return
 * TBLS_BAD_ARGUMENT without reaching the library (no write past the caller's
 * array: built with ASan/UBSan), well-formed ones must reach it as the Java
 * side passed them, and the counters must land in the caller's array as pairs
 * of words, low then high.  Prints "ok" and exits 0 on success.  Test
 * infrastructure only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jni.h"
#include "tekubls.h"

/* ---- the stub JNI environment ------------------------------------------ */
static int pending;
static jsize s_len(JNIEnv* e, jarray a) { (void)e; return a->len; }
static int oob(jarray a, jsize s, jsize n) { return s < 0 || n < 0 || s + n > a->len; }
static void s_getb(JNIEnv* e, jarray a, jsize s, jsize n, jbyte* b) { (void)e, (void)a, (void)s, (void)n, (void)b; pending = 1; }
static void s_setb(JNIEnv* e, jarray a, jsize s, jsize n, const jbyte* b) { (void)e, (void)a, (void)s, (void)n, (void)b; pending = 1; }
static void s_geti(JNIEnv* e, jarray a, jsize s, jsize n, jint* b) { (void)e, (void)a, (void)s, (void)n, (void)b; pending = 1; }
static void s_getl(JNIEnv* e, jarray a, jsize s, jsize n, jlong* b) { (void)e, (void)a, (void)s, (void)n, (void)b; pending = 1; }
static void s_seti(JNIEnv* e, jarray a, jsize s, jsize n, const jint* b) {
  (void)e;
  if (oob(a, s, n)) { pending = 1; return; }
  memcpy((jint*)a->data + s, b, (size_t)n * 4);
}
static jboolean s_exc(JNIEnv* e) { (void)e; return (jboolean)pending; }
static jbyte* s_elems(JNIEnv* e, jarray a, jboolean* c) { (void)e, (void)c; return (jbyte*)a->data; }
static void s_rel(JNIEnv* e, jarray a, jbyte* p, jint m) { (void)e, (void)a, (void)p, (void)m; }
static jstring s_str(JNIEnv* e, const char* s) { (void)e, (void)s; return NULL; }
static const struct JNINativeInterface_ TABLE = {s_len, s_getb, s_setb, s_geti, s_seti, s_getl, s_exc, s_elems, s_rel, s_str};
static JNIEnv ENV = &TABLE;

static jobject arr(jsize len, int elem) {
  struct stub_array* a = (struct stub_array*)calloc(1, sizeof *a);
  a->len = len;
  a->elem = elem;
  a->data = calloc(len ? (size_t)len : 1, (size_t)elem); /* exactly len elements: ASan sees any over-write */
  return a;
}
static void arr_free(jobject a) {
  if (!a) return;
  free(a->data);
  free(a);
}

/* ---- the recording fake of the C ABI ------------------------------------- */
static int configures, stats, clears, next_rc, last_reset;
static uint32_t last_rows;

int tbls_msg_memo_configure(uint32_t rows) {
  configures++;
  last_rows = rows;
  return next_rc;
}
int tbls_msg_memo_stats(uint64_t out[4], int reset) {
  stats++;
  last_reset = reset;
  if (next_rc) return next_rc;
  out[0] = 0x0000000500000007ull; /* a count past 2^32 */
  out[1] = 0xfffffffeull;         /* a low word with its top bit set */
  out[2] = 3;
  out[3] = 1048576;
  return TBLS_SUCCESS;
}
int tbls_msg_memo_clear(void) {
  clears++;
  return next_rc;
}

/* ---- the glue's entry points under test ----------------------------------- */
#define J(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipMemo_##n
jint J(msgMemoConfigure)(JNIEnv*, jclass, jint);
jint J(msgMemoStats)(JNIEnv*, jclass, jintArray, jboolean);
jint J(msgMemoClear)(JNIEnv*, jclass);

static int failures;
#define CHECK(cond, what)                            \
  do {                                               \
    if (!(cond)) {                                   \
      printf("FAIL %s (line %d)\n", what, __LINE__); \
      failures++;                                    \
    }                                                \
  } while (0)

int main(void) {
  CHECK(J(msgMemoConfigure)(&ENV, NULL, 4096) == TBLS_SUCCESS && configures == 1 && last_rows == 4096, "configure reaches the library");
  CHECK(J(msgMemoConfigure)(&ENV, NULL, 0) == TBLS_SUCCESS && configures == 2 && last_rows == 0, "rows = 0 turns it off");
  CHECK(J(msgMemoConfigure)(&ENV, NULL, -1) == TBLS_BAD_ARGUMENT && configures == 2, "a negative row count does not reach the library");

  /* the counters, with room to spare: nothing is written past the eight words */
  jobject out = arr(10, 4);
  jint* o = (jint*)out->data;
  o[8] = 77;
  CHECK(J(msgMemoStats)(&ENV, NULL, out, 1) == TBLS_SUCCESS && stats == 1 && last_reset == 1, "stats reaches the library, reset passed on");
  CHECK(o[0] == 7 && o[1] == 5 && o[2] == -2 && o[3] == 0 && o[4] == 3 && o[5] == 0 && o[6] == 1048576 && o[7] == 0, "low word, then high word");
  CHECK(o[8] == 77, "nothing written past the eight words");
  jobject out8 = arr(8, 4);
  CHECK(J(msgMemoStats)(&ENV, NULL, out8, 0) == TBLS_SUCCESS && stats == 2 && last_reset == 0, "an array of exactly eight words");

  /* malformed: NULL and short arrays */
  jobject out7 = arr(7, 4);
  CHECK(J(msgMemoStats)(&ENV, NULL, NULL, 0) == TBLS_BAD_ARGUMENT, "NULL output");
  CHECK(J(msgMemoStats)(&ENV, NULL, out7, 0) == TBLS_BAD_ARGUMENT, "a short output array");
  CHECK(stats == 2 && !pending, "malformed arguments do not reach the library");

  /* the library's status comes back, and the output stays as it was */
  next_rc = TBLS_DEVICE_ERROR;
  o[0] = 123;
  CHECK(J(msgMemoStats)(&ENV, NULL, out, 0) == TBLS_DEVICE_ERROR && o[0] == 123, "the library's status, the array untouched");
  CHECK(J(msgMemoConfigure)(&ENV, NULL, 8) == TBLS_DEVICE_ERROR && J(msgMemoClear)(&ENV, NULL) == TBLS_DEVICE_ERROR, "the status of the others");
  next_rc = 0;
  CHECK(J(msgMemoClear)(&ENV, NULL) == TBLS_SUCCESS && clears == 2, "clear");

  arr_free(out), arr_free(out8), arr_free(out7);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
