/*
 * JNI glue of TekuBlsHipGroupedEach (integration/java/.../hip/
 * TekuBlsHipGroupedEach.java) onto tbls_batch_verify_each_grouped of
 * include/tekubls.h: the batch over message groups and, when it fails, every
 * set's verdict settled from the grouped pass, in one call.  A file and a
 * class of its own beside tekubls_grouped_jni.c / TekuBlsHipGrouped, which
 * stay the binding of tbls_batch_verify_grouped alone.  Same conventions:
 * arrays are copied in with Get*ArrayRegion, and every argument is validated
 * before the library sees a pointer into a copy -- NULL arrays, nPks[i] < 0,
 * key counts past the key array, message offsets that are not n + 1 monotone
 * values inside the message array, signature or randomizer arrays shorter
 * than the sets, an empty batch-verdict array, a per-set verdict array shorter
 * than the sets; a failed check returns TBLS_BAD_ARGUMENT (a failed allocation
 * TBLS_DEVICE_ERROR) without calling the library.
 *
 * Build beside tekubls_jni.c, into the same libtekubls_jni.so.
 */
#include <jni.h>
#include <stdlib.h>
#include <string.h>
#include "tekubls.h"

#define JNAME(n) Java_tech_pegasys_teku_bls_impl_hip_TekuBlsHipGroupedEach_##n

static jsize alen(JNIEnv* env, jarray a) { return a ? (*env)->GetArrayLength(env, a) : -1; }

/* a copy of the whole array (1 byte when empty); NULL with *rc set */
static void* copy_in(JNIEnv* env, jarray a, size_t unit, jsize* n, int* rc) {
  *n = alen(env, a);
  if (*n < 0) {
    *rc = TBLS_BAD_ARGUMENT;
    return NULL;
  }
  void* p = malloc(*n ? (size_t)*n * unit : 1);
  if (!p) {
    *rc = TBLS_DEVICE_ERROR;
    return NULL;
  }
  if (*n) {
    if (unit == 1) (*env)->GetByteArrayRegion(env, (jbyteArray)a, 0, *n, (jbyte*)p);
    else if (unit == 4) (*env)->GetIntArrayRegion(env, (jintArray)a, 0, *n, (jint*)p);
    else (*env)->GetLongArrayRegion(env, (jlongArray)a, 0, *n, (jlong*)p);
  }
  if ((*env)->ExceptionCheck(env)) {
    free(p);
    *rc = TBLS_BAD_ARGUMENT;
    return NULL;
  }
  return p;
}

/* tbls_batch_verify_each_grouped over flattened sets: pks (sum nPks * 48
 * bytes), nPks[n], messages concatenated with msgOff[n + 1], sigs (n * 96),
 * rand[n]; okOut[0] the batch verdict, okPerSet[0..n) the sets' (written only
 * when the library returns TBLS_SUCCESS) */
JNIEXPORT jint JNICALL JNAME(batchVerifyEachGrouped)(JNIEnv* env, jclass c, jbyteArray pks, jintArray nPks, jbyteArray msgs,
                                                     jintArray msgOff, jbyteArray sigs, jlongArray rand, jint nGpus, jint flags,
                                                     jintArray okOut, jintArray okPerSet) {
  (void)c;
  if (alen(env, okOut) < 1) return TBLS_BAD_ARGUMENT;
  int rc = TBLS_SUCCESS, ok = 0;
  jsize n = 0, n_off = 0, pl = 0, ml = 0, sl = 0, rl = 0;
  int32_t* np = (int32_t*)copy_in(env, nPks, 4, &n, &rc);
  int32_t* mo = np ? (int32_t*)copy_in(env, msgOff, 4, &n_off, &rc) : NULL;
  uint8_t* pk = mo ? (uint8_t*)copy_in(env, pks, 1, &pl, &rc) : NULL;
  uint8_t* m = pk ? (uint8_t*)copy_in(env, msgs, 1, &ml, &rc) : NULL;
  uint8_t* sg = m ? (uint8_t*)copy_in(env, sigs, 1, &sl, &rc) : NULL;
  uint64_t* r = sg ? (uint64_t*)copy_in(env, rand, 8, &rl, &rc) : NULL;
  tbls_set* sets = NULL;
  int* each = NULL;
  int done = 0;
  if (r) {
    int shape = n_off == n + 1 && mo[0] == 0 && (size_t)sl >= 96u * (size_t)n && rl >= n && alen(env, okPerSet) >= n;
    size_t k = 0;
    for (jsize i = 0; shape && i < n; i++) {
      if (np[i] < 0 || mo[i + 1] < mo[i] || mo[i + 1] > ml) shape = 0;
      else k += (size_t)np[i];
    }
    if (!shape || k > (size_t)pl / 48) {
      rc = TBLS_BAD_ARGUMENT;
    } else if (!(sets = (tbls_set*)malloc(sizeof(tbls_set) * (n ? (size_t)n : 1))) || !(each = (int*)calloc(n ? (size_t)n : 1, sizeof(int)))) {
      rc = TBLS_DEVICE_ERROR;
    } else {
      k = 0;
      for (jsize i = 0; i < n; i++) {
        sets[i].pks = pk + 48 * k;
        sets[i].n_pks = (uint32_t)np[i];
        sets[i].msg = m + mo[i];
        sets[i].msg_len = (uint32_t)(mo[i + 1] - mo[i]);
        sets[i].sig = sg + 96 * (size_t)i;
        k += (size_t)np[i];
      }
      rc = tbls_batch_verify_each_grouped(sets, (size_t)n, r, nGpus, (uint32_t)flags, &ok, each, NULL);
      done = rc == TBLS_SUCCESS;
    }
  }
  if (done && n) {
    jint* v = (jint*)each;  /* jint and int are both 32 bits here (checked below) */
    (*env)->SetIntArrayRegion(env, okPerSet, 0, n, v);
  }
  free(each);
  free(sets);
  free(r);
  free(sg);
  free(m);
  free(pk);
  free(mo);
  free(np);
  jint x = ok;
  (*env)->SetIntArrayRegion(env, okOut, 0, 1, &x);
  return rc;
}

typedef char jint_is_int[sizeof(jint) == sizeof(int) ? 1 : -1];
