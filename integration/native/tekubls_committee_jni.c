/*
 * JNI glue of TekuBlsHipCommittee (integration/java/.../hip/
 * TekuBlsHipCommittee.java) onto the sync-committee entries of
 * include/tekubls.h: fastAggregateVerify with keys by table index, resident
 * committees, and sets given as participation bitvectors.  Same conventions
 * as tekubls_jni.c: arrays are copied in with Get*ArrayRegion, and every
 * argument is validated before the library sees a pointer into a copy --
 * NULL arrays, n + 1 monotone message offsets inside the message bytes,
 * sum(nPks) indices, n bit rows of (size + 7) / 8 bytes, n signatures, an
 * output array of n verdicts; a failed check returns TBLS_BAD_ARGUMENT (a
 * failed allocation TBLS_DEVICE_ERROR) without calling the library.
 *
 * Build beside tekubls_jni.c, into the same libtekubls_jni.so.
 */
#include <jni.h>
#include <stdlib.h>
#include <string.h>
#include "tekubls.h"

#define JNAME(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipCommittee_##n

static jsize alen(JNIEnv* env, jarray a) { return a ? (*env)->GetArrayLength(env, a) : -1; }

/* byte[] / int[] -> malloc'd copy; NULL on a NULL array, a failed allocation
 * or a failed copy (*rc says which); *len = its length */
static uint8_t* bytes_in(JNIEnv* env, jbyteArray a, jsize* len, int* rc) {
  const jsize n = alen(env, a);
  *len = n < 0 ? 0 : n;
  if (n < 0) {
    *rc = TBLS_BAD_ARGUMENT;
    return NULL;
  }
  uint8_t* p = (uint8_t*)malloc(n ? (size_t)n : 1);
  if (!p) {
    *rc = TBLS_DEVICE_ERROR;
    return NULL;
  }
  if (n) (*env)->GetByteArrayRegion(env, a, 0, n, (jbyte*)p);
  if ((*env)->ExceptionCheck(env)) {
    free(p);
    *rc = TBLS_BAD_ARGUMENT;
    return NULL;
  }
  return p;
}

static int32_t* ints_in(JNIEnv* env, jintArray a, jsize* len, int* rc) {
  const jsize n = alen(env, a);
  *len = n < 0 ? 0 : n;
  if (n < 0) {
    *rc = TBLS_BAD_ARGUMENT;
    return NULL;
  }
  int32_t* p = (int32_t*)malloc(sizeof(int32_t) * (n ? (size_t)n : 1));
  if (!p) {
    *rc = TBLS_DEVICE_ERROR;
    return NULL;
  }
  if (n) (*env)->GetIntArrayRegion(env, a, 0, n, (jint*)p);
  if ((*env)->ExceptionCheck(env)) {
    free(p);
    *rc = TBLS_BAD_ARGUMENT;
    return NULL;
  }
  return p;
}

/* n + 1 monotone offsets from 0 inside msgs_len bytes */
static int offsets_ok(const int32_t* mo, jsize n_off, jsize n, jsize msgs_len) {
  if (n < 0 || n_off != n + 1 || mo[0] != 0) return 0;
  for (jsize i = 0; i < n; i++)
    if (mo[i + 1] < mo[i] || mo[i + 1] > msgs_len) return 0;
  return 1;
}

static void verdicts_out(JNIEnv* env, jintArray okPerSet, const int* ok, jsize n) {
  if (n) (*env)->SetIntArrayRegion(env, okPerSet, 0, n, (const jint*)ok);
}

/* tbls_fast_aggregate_verify_many_idx: set i has nPks[i] table indices (keyIdx,
 * concatenated), message msgs[msgOff[i], msgOff[i + 1]) and signature sigs[96 i ..] */
JNIEXPORT jint JNICALL JNAME(fastAggregateVerifyManyIdx)(JNIEnv* env, jclass c, jintArray keyIdx, jintArray nPks, jbyteArray msgs,
                                                         jintArray msgOff, jbyteArray sigs, jintArray okPerSet) {
  (void)c;
  jsize n = 0, ni = 0, no = 0, ml = 0, sl = 0;
  int rc = TBLS_SUCCESS;
  int32_t* np = ints_in(env, nPks, &n, &rc);
  int32_t* ki = np ? ints_in(env, keyIdx, &ni, &rc) : NULL;
  int32_t* mo = ki ? ints_in(env, msgOff, &no, &rc) : NULL;
  uint8_t* m = mo ? bytes_in(env, msgs, &ml, &rc) : NULL;
  uint8_t* sg = m ? bytes_in(env, sigs, &sl, &rc) : NULL;
  tbls_set_idx* sets = NULL;
  int* ok = NULL;
  if (sg) {
    size_t k = 0;
    int shape = offsets_ok(mo, no, n, ml) && (size_t)sl >= 96u * (size_t)n && alen(env, okPerSet) >= n;
    for (jsize i = 0; shape && i < n; i++) {
      shape = np[i] >= 0;
      k += shape ? (size_t)np[i] : 0;
    }
    if (!shape || k > (size_t)ni) {
      rc = TBLS_BAD_ARGUMENT;
    } else {
      sets = (tbls_set_idx*)malloc(sizeof(tbls_set_idx) * (n ? (size_t)n : 1));
      ok = (int*)calloc(n ? (size_t)n : 1, sizeof(int));
      if (!sets || !ok) {
        rc = TBLS_DEVICE_ERROR;
      } else {
        k = 0;
        for (jsize i = 0; i < n; i++) {
          sets[i].key_idx = (const uint32_t*)ki + k;
          sets[i].n_pks = (uint32_t)np[i];
          sets[i].msg = m + mo[i];
          sets[i].msg_len = (uint32_t)(mo[i + 1] - mo[i]);
          sets[i].sig = sg + 96 * (size_t)i;
          k += (size_t)np[i];
        }
        rc = tbls_fast_aggregate_verify_many_idx(sets, (size_t)n, ok);
        if (rc == TBLS_SUCCESS) verdicts_out(env, okPerSet, ok, n);
      }
    }
  }
  free(ok);
  free(sets);
  free(sg);
  free(m);
  free(mo);
  free(ki);
  free(np);
  return rc;
}

/* tbls_committee_load: the committee's validator indices into `slot` */
JNIEXPORT jint JNICALL JNAME(committeeLoad)(JNIEnv* env, jclass c, jint slot, jintArray keyIdx) {
  (void)c;
  jsize ni = 0;
  int rc = TBLS_SUCCESS;
  if (slot < 0 || slot >= TBLS_COMMITTEE_SLOTS) return TBLS_BAD_ARGUMENT;
  int32_t* ki = ints_in(env, keyIdx, &ni, &rc);
  if (!ki) return rc;
  if (ni < 1 || ni > TBLS_COMMITTEE_MAX)
    rc = TBLS_BAD_ARGUMENT;
  else
    rc = tbls_committee_load((uint32_t)slot, (const uint32_t*)ki, (uint32_t)ni);
  free(ki);
  return rc;
}

/* tbls_fast_aggregate_verify_many_bits: n sets over the committee of `size`
 * members in `slot`; bits holds n rows of (size + 7) / 8 bytes (the
 * SyncAggregate bitvectors), concatenated.  size is the caller's view of the
 * committee: it fixes the row length checked here, and the library rejects
 * the call when the slot holds another size. */
JNIEXPORT jint JNICALL JNAME(fastAggregateVerifyManyBits)(JNIEnv* env, jclass c, jint slot, jint size, jbyteArray bits, jbyteArray msgs,
                                                          jintArray msgOff, jbyteArray sigs, jintArray okPerSet) {
  (void)c;
  jsize bl = 0, no = 0, ml = 0, sl = 0;
  int rc = TBLS_SUCCESS;
  if (slot < 0 || slot >= TBLS_COMMITTEE_SLOTS || size < 1 || size > TBLS_COMMITTEE_MAX) return TBLS_BAD_ARGUMENT;
  const size_t row = ((size_t)size + 7u) / 8u;
  int32_t* mo = ints_in(env, msgOff, &no, &rc);
  uint8_t* b = mo ? bytes_in(env, bits, &bl, &rc) : NULL;
  uint8_t* m = b ? bytes_in(env, msgs, &ml, &rc) : NULL;
  uint8_t* sg = m ? bytes_in(env, sigs, &sl, &rc) : NULL;
  tbls_set_bits* sets = NULL;
  int* ok = NULL;
  if (sg) {
    const jsize n = no - 1;
    if (no < 1 || !offsets_ok(mo, no, n, ml) || (size_t)bl != row * (size_t)n || (size_t)sl < 96u * (size_t)n ||
        alen(env, okPerSet) < n) {
      rc = TBLS_BAD_ARGUMENT;
    } else if (tbls_committee_size((uint32_t)slot) != (uint32_t)size) {
      rc = TBLS_BAD_ARGUMENT; /* the slot was reloaded or emptied: the rows no longer fit it */
    } else {
      sets = (tbls_set_bits*)malloc(sizeof(tbls_set_bits) * (n ? (size_t)n : 1));
      ok = (int*)calloc(n ? (size_t)n : 1, sizeof(int));
      if (!sets || !ok) {
        rc = TBLS_DEVICE_ERROR;
      } else {
        for (jsize i = 0; i < n; i++) {
          sets[i].bits = b + row * (size_t)i;
          sets[i].msg = m + mo[i];
          sets[i].msg_len = (uint32_t)(mo[i + 1] - mo[i]);
          sets[i].sig = sg + 96 * (size_t)i;
        }
        rc = tbls_fast_aggregate_verify_many_bits((uint32_t)slot, sets, (size_t)n, ok);
        if (rc == TBLS_SUCCESS) verdicts_out(env, okPerSet, ok, n);
      }
    }
  }
  free(ok);
  free(sets);
  free(sg);
  free(m);
  free(b);
  free(mo);
  return rc;
}
