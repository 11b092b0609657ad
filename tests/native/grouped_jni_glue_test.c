/* Unit test of the grouped batch's JNI glue (integration/native/
 * tekubls_grouped_jni.c) against a recording fake of tbls_batch_verify_grouped
 * and the stub JNI environment of jni_stub/jni.h: malformed Java arguments
 * must return TBLS_BAD_ARGUMENT without reaching the library (no read past a
 * copied array: built with ASan/UBSan), well-formed ones must reach it with
 * the sets as the Java side passed them, and the verdict must land in the
 * caller's array.  Prints "ok" and exits 0 on success.  Test infrastructure only. */
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
static int calls, next_rc, last_gpus;
static size_t last_n;
static uint32_t last_flags, sum_keys, sum_msgs, sum_sigs;
static uint64_t sum_rand;

int tbls_batch_verify_grouped(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, uint32_t flags, int* ok, tbls_timing* t) {
  (void)t;
  calls++;
  last_n = n;
  last_gpus = n_gpus;
  last_flags = flags;
  sum_keys = sum_msgs = sum_sigs = 0;
  sum_rand = 0;
  for (size_t i = 0; i < n; i++) {  /* touch every byte of every set */
    for (uint32_t k = 0; k < 48 * sets[i].n_pks; k++) sum_keys += sets[i].pks[k];
    for (uint32_t k = 0; k < sets[i].msg_len; k++) sum_msgs += sets[i].msg[k];
    for (int k = 0; k < 96; k++) sum_sigs += sets[i].sig[k];
    sum_rand += rand[i];
  }
  *ok = 1;
  return next_rc;
}

/* ---- the glue's entry point under test ------------------------------------ */
#define J(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipGrouped_##n
jint J(batchVerifyGrouped)(JNIEnv*, jclass, jbyteArray, jintArray, jbyteArray, jintArray, jbyteArray, jlongArray, jint, jint, jintArray);

static int failures;
#define CHECK(cond, what)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("FAIL %s (line %d)\n", what, __LINE__);       \
      failures++;                                          \
    }                                                      \
  } while (0)

int main(void) {
  /* well-formed: 3 sets with 1 / 2 / 0 keys, messages of 2 / 0 / 3 bytes (sets 0 and 2 could share one) */
  jobject pks = arr(3 * 48, 1), npk = arr(3, 4), msgs = arr(5, 1), off = arr(4, 4), sigs = arr(3 * 96, 1), rnd = arr(3, 8), ok = arr(1, 4);
  uint32_t want_keys = 0, want_msgs = 0, want_sigs = 0;
  for (int i = 0; i < 3 * 48; i++) want_keys += ((uint8_t*)pks->data)[i] = (uint8_t)(i + 1);
  for (int i = 0; i < 5; i++) want_msgs += ((uint8_t*)msgs->data)[i] = (uint8_t)(200 + i);
  for (int i = 0; i < 3 * 96; i++) want_sigs += ((uint8_t*)sigs->data)[i] = (uint8_t)(3 * i);
  const jint np[3] = {1, 2, 0}, mo[4] = {0, 2, 2, 5};
  memcpy(npk->data, np, sizeof np);
  memcpy(off->data, mo, sizeof mo);
  const jlong rr[3] = {5, -1, 7};  /* an unsigned 64-bit randomizer with its top bit set */
  memcpy(rnd->data, rr, sizeof rr);
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, rnd, 1, 1, ok) == TBLS_SUCCESS && calls == 1, "reaches the library");
  CHECK(last_n == 3 && last_gpus == 1 && last_flags == TBLS_GROUP_FORCE, "n, nGpus and flags as passed");
  CHECK(sum_keys == want_keys && sum_msgs == want_msgs && sum_sigs == want_sigs && sum_rand == 5ull + 0xffffffffffffffffull + 7ull, "the sets as passed");
  CHECK(((jint*)ok->data)[0] == 1, "the verdict");

  /* no sets: reaches the library with n = 0 */
  jobject none1 = arr(0, 1), none4 = arr(0, 4), off1 = arr(1, 4), none8 = arr(0, 8);
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, none1, none4, none1, off1, none1, none8, 0, 0, ok) == TBLS_SUCCESS && calls == 2 && last_n == 0, "no sets");

  /* the library's status comes back */
  next_rc = TBLS_BAD_ARGUMENT;
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT && calls == 3, "the library's status");
  next_rc = 0;

  /* malformed arguments never reach the library */
  const int before = calls;
  jobject neg = arr(3, 4), many = arr(3, 4), off3 = arr(3, 4), down = arr(4, 4), past = arr(4, 4), first = arr(4, 4), sig2 = arr(2 * 96, 1), rnd2 = arr(2, 8),
          ok0 = arr(0, 4);
  const jint np_neg[3] = {1, -1, 0}, np_many[3] = {1, 2, 1}, mo_down[4] = {0, 2, 1, 5}, mo_past[4] = {0, 2, 2, 6}, mo_first[4] = {1, 2, 2, 5};
  memcpy(neg->data, np_neg, sizeof np_neg);
  memcpy(many->data, np_many, sizeof np_many);
  memcpy(off3->data, mo, 3 * sizeof(jint));
  memcpy(down->data, mo_down, sizeof mo_down);
  memcpy(past->data, mo_past, sizeof mo_past);
  memcpy(first->data, mo_first, sizeof mo_first);
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, NULL, npk, msgs, off, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "NULL keys");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, NULL, msgs, off, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "NULL key counts");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, NULL, off, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "NULL messages");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, NULL, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "NULL offsets");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off, NULL, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "NULL signatures");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, NULL, 0, 0, ok) == TBLS_BAD_ARGUMENT, "NULL randomizers");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, rnd, 0, 0, NULL) == TBLS_BAD_ARGUMENT, "NULL verdict");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, rnd, 0, 0, ok0) == TBLS_BAD_ARGUMENT, "an empty verdict array");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, neg, msgs, off, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "a negative key count");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, many, msgs, off, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "key counts past the key array");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off3, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "n offsets instead of n + 1");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, down, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "offsets that go down");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, past, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "an offset past the messages");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, first, sigs, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "a first offset that is not 0");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off, sig2, rnd, 0, 0, ok) == TBLS_BAD_ARGUMENT, "too few signatures");
  CHECK(J(batchVerifyGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, rnd2, 0, 0, ok) == TBLS_BAD_ARGUMENT, "too few randomizers");
  CHECK(calls == before && !pending, "malformed arguments do not reach the library");

  arr_free(pks), arr_free(npk), arr_free(msgs), arr_free(off), arr_free(sigs), arr_free(rnd), arr_free(ok), arr_free(none1), arr_free(none4);
  arr_free(off1), arr_free(none8), arr_free(neg), arr_free(many), arr_free(off3), arr_free(down), arr_free(past), arr_free(first), arr_free(sig2);
  arr_free(rnd2), arr_free(ok0);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
