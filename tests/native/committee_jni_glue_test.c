/* Unit test of the sync-committee JNI glue
 * (integration/native/tekubls_committee_jni.c) against a recording fake of
 * the C ABI entries it calls and the stub JNI environment of jni_stub/jni.h:
 * malformed Java arguments must return TBLS_BAD_ARGUMENT without reaching the
 * library (no read past a copied array: built with ASan/UBSan), well-formed
 * ones must reach it with the sets laid out as the Java side flattened them.
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
static int calls;
static size_t last_n;
static uint32_t last_slot, last_size, slot_size[TBLS_COMMITTEE_SLOTS];
static tbls_set_bits last_bits[8];
static tbls_set_idx last_idx[8];
static uint32_t last_members[8], seen_idx; /* contents are recorded inside the fake: the glue frees its copies on return */
static uint8_t seen_bit;

int tbls_fast_aggregate_verify_many_idx(const tbls_set_idx* sets, size_t n, int* ok) {
  size_t acc = 0;
  for (size_t i = 0; i < n; i++) {  /* touch every byte the sets name */
    if (i < 8) last_idx[i] = sets[i];
    if (i == 2 && sets[i].n_pks > 3) seen_idx = sets[i].key_idx[3];
    for (uint32_t k = 0; k < sets[i].n_pks; k++) acc += sets[i].key_idx[k];
    for (uint32_t k = 0; k < sets[i].msg_len; k++) acc += sets[i].msg[k];
    for (int k = 0; k < 96; k++) acc += sets[i].sig[k];
    ok[i] = (int)(i & 1) + (int)(acc & 0);
  }
  last_n = n;
  calls++;
  return TBLS_SUCCESS;
}
int tbls_committee_load(uint32_t slot, const uint32_t* key_idx, uint32_t size) {
  for (uint32_t k = 0; k < size; k++)
    if (k < 8) last_members[k] = key_idx[k];
  (void)key_idx[size - 1];
  last_slot = slot;
  last_size = size;
  slot_size[slot] = size;
  calls++;
  return TBLS_SUCCESS;
}
uint32_t tbls_committee_size(uint32_t slot) { return slot < TBLS_COMMITTEE_SLOTS ? slot_size[slot] : 0; }  /* a query: not counted */
int tbls_fast_aggregate_verify_many_bits(uint32_t slot, const tbls_set_bits* sets, size_t n, int* ok) {
  const uint32_t nb = (slot_size[slot] + 7u) / 8u;
  size_t acc = 0;
  for (size_t i = 0; i < n; i++) {
    if (i < 8) last_bits[i] = sets[i];
    if (i == 3 && nb > 1) seen_bit = sets[i].bits[1];
    for (uint32_t k = 0; k < nb; k++) acc += sets[i].bits[k];
    for (uint32_t k = 0; k < sets[i].msg_len; k++) acc += sets[i].msg[k];
    for (int k = 0; k < 96; k++) acc += sets[i].sig[k];
    ok[i] = (int)(i != 1) + (int)(acc & 0);
  }
  last_slot = slot;
  last_n = n;
  calls++;
  return TBLS_SUCCESS;
}

/* ---- the glue's entry points under test ----------------------------------- */
#define J(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipCommittee_##n
jint J(fastAggregateVerifyManyIdx)(JNIEnv*, jclass, jintArray, jintArray, jbyteArray, jintArray, jbyteArray, jintArray);
jint J(committeeLoad)(JNIEnv*, jclass, jint, jintArray);
jint J(fastAggregateVerifyManyBits)(JNIEnv*, jclass, jint, jint, jbyteArray, jbyteArray, jintArray, jbyteArray, jintArray);

static int failures;
#define CHECK(cond, what)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("FAIL %s (line %d)\n", what, __LINE__);       \
      failures++;                                          \
    }                                                      \
  } while (0)

/* n flattened sets over a committee of `size` members, ml-byte messages, nk indices each */
typedef struct {
  jobject bits, idx, npk, msgs, moff, sigs, ok;
} batch;
static batch mk(int n, int size, int ml, int nk) {
  batch b;
  b.bits = arr(n * ((size + 7) / 8), 1);
  b.idx = arr(n * nk, 4);
  b.npk = arr(n, 4);
  b.msgs = arr(n * ml, 1);
  b.moff = arr(n + 1, 4);
  b.sigs = arr(96 * n, 1);
  b.ok = arr(n ? n : 1, 4);
  for (int i = 0; i < n; i++) ((jint*)b.npk->data)[i] = nk;
  for (int i = 0; i <= n; i++) ((jint*)b.moff->data)[i] = i * ml;
  return b;
}
static void bfree(batch* b) {
  arr_free(b->bits), arr_free(b->idx), arr_free(b->npk), arr_free(b->msgs), arr_free(b->moff), arr_free(b->sigs), arr_free(b->ok);
}
static jint run_bits(batch* b, int slot, int size) {
  pending = 0;
  return J(fastAggregateVerifyManyBits)(&ENV, NULL, slot, size, b->bits, b->msgs, b->moff, b->sigs, b->ok);
}
static jint run_idx(batch* b) {
  pending = 0;
  return J(fastAggregateVerifyManyIdx)(&ENV, NULL, b->idx, b->npk, b->msgs, b->moff, b->sigs, b->ok);
}

int main(void) {
  /* committeeLoad: slot and size checked, members arrive as given */
  {
    jobject idx = arr(13, 4);
    for (int i = 0; i < 13; i++) ((jint*)idx->data)[i] = 1000 + i;
    calls = 0;
    pending = 0;
    CHECK(J(committeeLoad)(&ENV, NULL, 2, idx) == TBLS_SUCCESS && calls == 1 && last_slot == 2 && last_size == 13 && last_members[5] == 1005,
          "committeeLoad valid");
    calls = 0;
    CHECK(J(committeeLoad)(&ENV, NULL, 4, idx) == TBLS_BAD_ARGUMENT && J(committeeLoad)(&ENV, NULL, -1, idx) == TBLS_BAD_ARGUMENT && calls == 0,
          "committeeLoad slot");
    CHECK(J(committeeLoad)(&ENV, NULL, 0, NULL) == TBLS_BAD_ARGUMENT && calls == 0, "committeeLoad null");
    idx->len = 0;
    CHECK(J(committeeLoad)(&ENV, NULL, 0, idx) == TBLS_BAD_ARGUMENT && calls == 0, "committeeLoad empty");
    idx->len = 13;
    arr_free(idx);
    jobject big = arr(TBLS_COMMITTEE_MAX + 1, 4);
    CHECK(J(committeeLoad)(&ENV, NULL, 0, big) == TBLS_BAD_ARGUMENT && calls == 0, "committeeLoad too large");
    arr_free(big);
  }
  /* by bits, well-formed: reaches the library with the sets as flattened (slot 2 holds 13 members: 2-byte rows) */
  {
    batch b = mk(5, 13, 32, 1);
    ((jbyte*)b.bits->data)[2 * 3 + 1] = 0x11;
    calls = 0;
    CHECK(run_bits(&b, 2, 13) == TBLS_SUCCESS && calls == 1 && last_n == 5 && last_slot == 2, "valid bits call reaches the library");
    CHECK(last_bits[3].bits == last_bits[0].bits + 2 * 3 && seen_bit == 0x11 && last_bits[3].msg_len == 32 &&
              last_bits[3].msg == last_bits[0].msg + 96 && last_bits[3].sig == last_bits[0].sig + 96 * 3,
          "bits set layout");
    const jint* ok = (const jint*)b.ok->data;
    CHECK(ok[0] == 1 && ok[1] == 0 && ok[2] == 1 && ok[4] == 1, "bits verdicts copied out");
    bfree(&b);
  }
  /* by bits, malformed: BAD_ARGUMENT, library not called */
  const char* bad[] = {"bits short", "bits long", "msgOff not monotone", "msgOff past msgs", "msgOff[0] != 0", "sigs short",
                       "ok array small", "size not the slot's", "slot out of range", "size 0", "empty slot", "msgOff empty", "bits null"};
  for (int k = 0; k < (int)(sizeof bad / sizeof bad[0]); k++) {
    batch b = mk(4, 13, 32, 1);
    jint* mo = (jint*)b.moff->data;
    int slot = 2, size = 13;
    jobject keep_bits = b.bits;
    switch (k) {
      case 0: b.bits->len = 2 * 4 - 1; break;
      case 1: arr_free(b.bits); b.bits = keep_bits = arr(2 * 4 + 1, 1); break;
      case 2: mo[2] = 10; mo[1] = 40; break;
      case 3: mo[4] = 32 * 4 + 1; break;
      case 4: mo[0] = 1; break;
      case 5: b.sigs->len = 96 * 3 + 95; break;
      case 6: b.ok->len = 3; break;
      case 7: size = 16; break; /* same row length, another committee */
      case 8: slot = 4; break;
      case 9: size = 0; break;
      case 10: slot = 1; break;
      case 11: b.moff->len = 0; break;
      case 12: b.bits = NULL; break;
    }
    calls = 0;
    const jint rc = run_bits(&b, slot, size);
    CHECK(rc == TBLS_BAD_ARGUMENT && calls == 0, bad[k]);
    b.bits = keep_bits;
    bfree(&b);
  }
  /* by index: the same shape checks, and sum(nPks) indices */
  {
    batch b = mk(3, 8, 7, 4);
    for (int i = 0; i < 12; i++) ((jint*)b.idx->data)[i] = 50 + i;
    calls = 0;
    CHECK(run_idx(&b) == TBLS_SUCCESS && calls == 1 && last_n == 3, "valid idx call reaches the library");
    CHECK(last_idx[2].n_pks == 4 && last_idx[2].key_idx == last_idx[0].key_idx + 8 && seen_idx == 61 &&
              last_idx[2].msg == last_idx[0].msg + 14 && last_idx[2].msg_len == 7 && last_idx[2].sig == last_idx[0].sig + 192,
          "idx set layout");
    CHECK(((jint*)b.ok->data)[1] == 1 && ((jint*)b.ok->data)[2] == 0, "idx verdicts copied out");
    b.idx->len = 11;
    calls = 0;
    CHECK(run_idx(&b) == TBLS_BAD_ARGUMENT && calls == 0, "idx short");
    b.idx->len = 12;
    ((jint*)b.npk->data)[1] = -1;
    CHECK(run_idx(&b) == TBLS_BAD_ARGUMENT && calls == 0, "idx negative nPks");
    ((jint*)b.npk->data)[1] = 4;
    ((jint*)b.moff->data)[2] = 5;
    CHECK(run_idx(&b) == TBLS_BAD_ARGUMENT && calls == 0, "idx msgOff not monotone");
    ((jint*)b.moff->data)[2] = 14;
    b.sigs->len = 96 * 2;
    CHECK(run_idx(&b) == TBLS_BAD_ARGUMENT && calls == 0, "idx sigs short");
    b.sigs->len = 96 * 3;
    b.ok->len = 2;
    CHECK(run_idx(&b) == TBLS_BAD_ARGUMENT && calls == 0, "idx ok array small");
    b.ok->len = 3;
    b.moff->len = 3;
    CHECK(run_idx(&b) == TBLS_BAD_ARGUMENT && calls == 0, "idx msgOff short");
    b.moff->len = 4;
    CHECK(run_idx(&b) == TBLS_SUCCESS && calls == 1, "idx valid again");
    bfree(&b);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
