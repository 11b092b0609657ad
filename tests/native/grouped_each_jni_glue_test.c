/* Unit test of the grouped batch-and-settle JNI glue (integration/native/
 * tekubls_grouped_each_jni.c) against a recording fake of
 * tbls_batch_verify_each_grouped and the stub JNI environment of
 * jni_stub/jni.h: malformed Java arguments must return TBLS_BAD_ARGUMENT
 * without reaching the library (no read past a copied array: built with
 * ASan/UBSan), well-formed ones must reach it with the sets as the Java side
 * passed them, and the batch verdict and the per-set verdicts must land in the
 * caller's arrays.  Prints "ok" and exits 0 on success.  Test infrastructure only. */
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

int tbls_batch_verify_each_grouped(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, uint32_t flags, int* ok, int* ok_per_set,
                                   tbls_timing* t) {
  (void)t;
  calls++;
  last_n = n;
  last_gpus = n_gpus;
  last_flags = flags;
  sum_keys = sum_msgs = sum_sigs = 0;
  sum_rand = 0;
  for (size_t i = 0; i < n; i++) {  /* touch every byte of every set; a set with keys is valid here */
    for (uint32_t k = 0; k < 48 * sets[i].n_pks; k++) sum_keys += sets[i].pks[k];
    for (uint32_t k = 0; k < sets[i].msg_len; k++) sum_msgs += sets[i].msg[k];
    for (int k = 0; k < 96; k++) sum_sigs += sets[i].sig[k];
    sum_rand += rand[i];
    ok_per_set[i] = sets[i].n_pks ? 1 : 0;
  }
  *ok = 0;
  return next_rc;
}

/* ---- the glue's entry point under test ------------------------------------ */
#define J(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipGroupedEach_##n
jint J(batchVerifyEachGrouped)(JNIEnv*, jclass, jbyteArray, jintArray, jbyteArray, jintArray, jbyteArray, jlongArray, jint, jint, jintArray, jintArray);

static int failures;
#define CHECK(cond, what)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("FAIL %s (line %d)\n", what, __LINE__);       \
      failures++;                                          \
    }                                                      \
  } while (0)

int main(void) {
  /* well-formed: 3 sets with 1 / 2 / 0 keys, messages of 2 / 0 / 3 bytes */
  jobject pks = arr(3 * 48, 1), npk = arr(3, 4), msgs = arr(5, 1), off = arr(4, 4), sigs = arr(3 * 96, 1), rnd = arr(3, 8), ok = arr(1, 4), each = arr(3, 4);
  uint32_t want_keys = 0, want_msgs = 0, want_sigs = 0;
  for (int i = 0; i < 3 * 48; i++) want_keys += ((uint8_t*)pks->data)[i] = (uint8_t)(i + 1);
  for (int i = 0; i < 5; i++) want_msgs += ((uint8_t*)msgs->data)[i] = (uint8_t)(200 + i);
  for (int i = 0; i < 3 * 96; i++) want_sigs += ((uint8_t*)sigs->data)[i] = (uint8_t)(3 * i);
  const jint np[3] = {1, 2, 0}, mo[4] = {0, 2, 2, 5}, sevens[3] = {7, 7, 7};
  memcpy(npk->data, np, sizeof np);
  memcpy(off->data, mo, sizeof mo);
  memcpy(each->data, sevens, sizeof sevens);
  ((jint*)ok->data)[0] = 7;
  const jlong rr[3] = {5, -1, 7};  /* an unsigned 64-bit randomizer with its top bit set */
  memcpy(rnd->data, rr, sizeof rr);
  CHECK(J(batchVerifyEachGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, rnd, 1, 1, ok, each) == TBLS_SUCCESS && calls == 1, "reaches the library");
  CHECK(last_n == 3 && last_gpus == 1 && last_flags == TBLS_GROUP_FORCE, "n, nGpus and flags as passed");
  CHECK(sum_keys == want_keys && sum_msgs == want_msgs && sum_sigs == want_sigs && sum_rand == 5ull + 0xffffffffffffffffull + 7ull, "the sets as passed");
  CHECK(((jint*)ok->data)[0] == 0, "the batch verdict");
  CHECK(((jint*)each->data)[0] == 1 && ((jint*)each->data)[1] == 1 && ((jint*)each->data)[2] == 0, "the per-set verdicts");

  /* a longer per-set array keeps its tail */
  jobject each5 = arr(5, 4);
  ((jint*)each5->data)[3] = ((jint*)each5->data)[4] = 9;
  CHECK(J(batchVerifyEachGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, rnd, 0, 0, ok, each5) == TBLS_SUCCESS && calls == 2 && last_flags == 0, "a longer verdict array");
  CHECK(((jint*)each5->data)[0] == 1 && ((jint*)each5->data)[2] == 0 && ((jint*)each5->data)[3] == 9 && ((jint*)each5->data)[4] == 9, "only n verdicts written");

  /* no sets: reaches the library with n = 0, an empty per-set array is enough */
  jobject none1 = arr(0, 1), none4 = arr(0, 4), off1 = arr(1, 4), none8 = arr(0, 8), each0 = arr(0, 4);
  CHECK(J(batchVerifyEachGrouped)(&ENV, NULL, none1, none4, none1, off1, none1, none8, 0, 0, ok, each0) == TBLS_SUCCESS && calls == 3 && last_n == 0, "no sets");

  /* the library's status comes back, and the per-set array is left alone */
  next_rc = TBLS_DEVICE_ERROR;
  memcpy(each->data, sevens, sizeof sevens);
  CHECK(J(batchVerifyEachGrouped)(&ENV, NULL, pks, npk, msgs, off, sigs, rnd, 0, 0, ok, each) == TBLS_DEVICE_ERROR && calls == 4, "the library's status");
  CHECK(((jint*)each->data)[0] == 7 && ((jint*)each->data)[2] == 7 && ((jint*)ok->data)[0] == 0, "no verdicts after an error");
  next_rc = 0;

  /* malformed arguments never reach the library */
  const int before = calls;
  jobject neg = arr(3, 4), many = arr(3, 4), off3 = arr(3, 4), down = arr(4, 4), past = arr(4, 4), first = arr(4, 4), sig2 = arr(2 * 96, 1), rnd2 = arr(2, 8),
          ok0 = arr(0, 4), each2 = arr(2, 4);
  const jint np_neg[3] = {1, -1, 0}, np_many[3] = {1, 2, 1}, mo_down[4] = {0, 2, 1, 5}, mo_past[4] = {0, 2, 2, 6}, mo_first[4] = {1, 2, 2, 5};
  memcpy(neg->data, np_neg, sizeof np_neg);
  memcpy(many->data, np_many, sizeof np_many);
  memcpy(off3->data, mo, 3 * sizeof(jint));
  memcpy(down->data, mo_down, sizeof mo_down);
  memcpy(past->data, mo_past, sizeof mo_past);
  memcpy(first->data, mo_first, sizeof mo_first);
#define CALL(a, b, c, d, e, f, g, h) J(batchVerifyEachGrouped)(&ENV, NULL, a, b, c, d, e, f, 0, 0, g, h)
  CHECK(CALL(NULL, npk, msgs, off, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "NULL keys");
  CHECK(CALL(pks, NULL, msgs, off, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "NULL key counts");
  CHECK(CALL(pks, npk, NULL, off, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "NULL messages");
  CHECK(CALL(pks, npk, msgs, NULL, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "NULL offsets");
  CHECK(CALL(pks, npk, msgs, off, NULL, rnd, ok, each) == TBLS_BAD_ARGUMENT, "NULL signatures");
  CHECK(CALL(pks, npk, msgs, off, sigs, NULL, ok, each) == TBLS_BAD_ARGUMENT, "NULL randomizers");
  CHECK(CALL(pks, npk, msgs, off, sigs, rnd, NULL, each) == TBLS_BAD_ARGUMENT, "NULL batch verdict");
  CHECK(CALL(pks, npk, msgs, off, sigs, rnd, ok0, each) == TBLS_BAD_ARGUMENT, "an empty batch verdict array");
  CHECK(CALL(pks, npk, msgs, off, sigs, rnd, ok, NULL) == TBLS_BAD_ARGUMENT, "NULL per-set verdicts");
  CHECK(CALL(pks, npk, msgs, off, sigs, rnd, ok, each2) == TBLS_BAD_ARGUMENT, "too few per-set verdicts");
  CHECK(CALL(pks, neg, msgs, off, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "a negative key count");
  CHECK(CALL(pks, many, msgs, off, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "key counts past the key array");
  CHECK(CALL(pks, npk, msgs, off3, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "n offsets instead of n + 1");
  CHECK(CALL(pks, npk, msgs, down, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "offsets that go down");
  CHECK(CALL(pks, npk, msgs, past, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "an offset past the messages");
  CHECK(CALL(pks, npk, msgs, first, sigs, rnd, ok, each) == TBLS_BAD_ARGUMENT, "a first offset that is not 0");
  CHECK(CALL(pks, npk, msgs, off, sig2, rnd, ok, each) == TBLS_BAD_ARGUMENT, "too few signatures");
  CHECK(CALL(pks, npk, msgs, off, sigs, rnd2, ok, each) == TBLS_BAD_ARGUMENT, "too few randomizers");
  CHECK(calls == before && !pending, "malformed arguments do not reach the library");

  arr_free(pks), arr_free(npk), arr_free(msgs), arr_free(off), arr_free(sigs), arr_free(rnd), arr_free(ok), arr_free(each), arr_free(each5);
  arr_free(none1), arr_free(none4), arr_free(off1), arr_free(none8), arr_free(each0), arr_free(neg), arr_free(many), arr_free(off3), arr_free(down);
  arr_free(past), arr_free(first), arr_free(sig2), arr_free(rnd2), arr_free(ok0), arr_free(each2);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
