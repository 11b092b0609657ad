/* Unit test of the key-index JNI glue (integration/native/tekubls_pkindex_jni.c)
 * against a recording fake of the C ABI entries it calls and the stub JNI
 * environment of jni_stub/jni.h: malformed Java arguments must return
 * TBLS_BAD_ARGUMENT without reaching the library (no read past a copied array:
 * built with ASan/UBSan), well-formed ones must reach it with the keys as the
 * Java side passed them, and the answers must land in the caller's array.
 * Prints "ok" and exits 0 on success.  Test infrastructure only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jni.h"
#include "tekubls.h"

/* ---- the stub JNI environment ------------------------------------------ */
static int pending;
static jsize s_len(JNIEnv* e, jarray a) { (void)e; return a->len; }
static int oob(jarray a, jsize s, jsize n) { return s < 0 || n < 0 || s + n > a->len; }
#define REGION(name, T)                                                    \
  static void name(JNIEnv* e, jarray a, jsize s, jsize n, T* b) {          \
    (void)e;                                                               \
    if (oob(a, s, n)) { pending = 1; return; }                             \
    memcpy(b, (char*)a->data + (size_t)s * sizeof(T), (size_t)n * sizeof(T)); \
  }
REGION(s_getb, jbyte)
REGION(s_getl, jlong)
REGION(s_geti, jint)
static void s_seti(JNIEnv* e, jarray a, jsize s, jsize n, const jint* b) {
  (void)e;
  if (oob(a, s, n)) { pending = 1; return; }
  memcpy((jint*)a->data + s, b, (size_t)n * 4);
}
static void s_setb(JNIEnv* e, jarray a, jsize s, jsize n, const jbyte* b) {
  (void)e;
  if (oob(a, s, n)) { pending = 1; return; }
  memcpy((jbyte*)a->data + s, b, (size_t)n);
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
  a->data = calloc(len ? (size_t)len : 1, (size_t)elem);  /* exactly len elements: ASan sees any over-read */
  return a;
}
static void arr_free(jobject a) {
  if (!a) return;
  free(a->data);
  free(a);
}

/* ---- the recording fake of the C ABI ------------------------------------- */
static int calls, clears, next_rc;
static size_t last_n;
static uint8_t seen_first, seen_last;

int tbls_pk_table_resolve(const uint8_t* pks, size_t n, uint32_t* idx_out) {
  calls++;
  last_n = n;
  if (next_rc) return next_rc;
  for (size_t i = 0; i < n; i++) {  /* touch every byte of every key */
    uint32_t acc = 0;
    for (int k = 0; k < 48; k++) acc += pks[48 * i + k];
    idx_out[i] = (i & 1) ? 0xffffffffu : 1000u + acc;
  }
  if (n) {
    seen_first = pks[0];
    seen_last = pks[48 * n - 1];
  }
  return TBLS_SUCCESS;
}
int tbls_pk_table_clear(void) {
  clears++;
  return TBLS_SUCCESS;
}

/* ---- the glue's entry points under test ----------------------------------- */
#define J(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipPkIndex_##n
jint J(pkTableResolve)(JNIEnv*, jclass, jbyteArray, jintArray);
jint J(pkTableClear)(JNIEnv*, jclass);

static int failures;
#define CHECK(cond, what)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("FAIL %s (line %d)\n", what, __LINE__);       \
      failures++;                                          \
    }                                                      \
  } while (0)

int main(void) {
  /* well-formed: 3 keys, an output array with room to spare */
  jobject pks = arr(3 * 48, 1), out = arr(5, 4);
  uint8_t* p = (uint8_t*)pks->data;
  for (int i = 0; i < 3 * 48; i++) p[i] = (uint8_t)(i + 1);
  ((jint*)out->data)[3] = 77;
  CHECK(J(pkTableResolve)(&ENV, NULL, pks, out) == TBLS_SUCCESS && calls == 1 && last_n == 3, "resolve reaches the library");
  CHECK(seen_first == 1 && seen_last == 144, "the keys as passed");
  uint32_t acc0 = 0, acc2 = 0;
  for (int k = 0; k < 48; k++) acc0 += p[k], acc2 += p[96 + k];
  const jint* o = (const jint*)out->data;
  CHECK((uint32_t)o[0] == 1000u + acc0 && o[1] == -1 && (uint32_t)o[2] == 1000u + acc2, "the indices, a miss as -1");
  CHECK(o[3] == 77, "nothing written past n answers");

  /* an output array of exactly n */
  jobject out3 = arr(3, 4);
  CHECK(J(pkTableResolve)(&ENV, NULL, pks, out3) == TBLS_SUCCESS && calls == 2, "output of exactly n");

  /* no keys: reaches the library with n = 0 and writes nothing */
  jobject none = arr(0, 1), out0 = arr(0, 4);
  CHECK(J(pkTableResolve)(&ENV, NULL, none, out0) == TBLS_SUCCESS && calls == 3 && last_n == 0, "no keys");

  /* malformed: NULL arrays, a partial key, a short output array */
  jobject partial = arr(3 * 48 - 1, 1), out2 = arr(2, 4);
  const int before = calls;
  CHECK(J(pkTableResolve)(&ENV, NULL, NULL, out) == TBLS_BAD_ARGUMENT, "NULL keys");
  CHECK(J(pkTableResolve)(&ENV, NULL, pks, NULL) == TBLS_BAD_ARGUMENT, "NULL output");
  CHECK(J(pkTableResolve)(&ENV, NULL, partial, out) == TBLS_BAD_ARGUMENT, "a partial key");
  CHECK(J(pkTableResolve)(&ENV, NULL, pks, out2) == TBLS_BAD_ARGUMENT, "a short output array");
  CHECK(calls == before && !pending, "malformed arguments do not reach the library");

  /* the library's status comes back, and the output stays as it was */
  next_rc = TBLS_BAD_ARGUMENT; /* no table */
  ((jint*)out->data)[0] = 5;
  CHECK(J(pkTableResolve)(&ENV, NULL, pks, out) == TBLS_BAD_ARGUMENT && ((jint*)out->data)[0] == 5, "the library's status");
  next_rc = 0;

  CHECK(J(pkTableClear)(&ENV, NULL) == TBLS_SUCCESS && clears == 1, "clear");

  arr_free(pks), arr_free(out), arr_free(out3), arr_free(none), arr_free(out0), arr_free(partial), arr_free(out2);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
