// libtekubls_hip.so: host side of the C ABI (include/tekubls.h).
//
// One HIP stream + workspace per device, guarded by a per-device mutex so the
// library is thread-safe and re-entrant (prepareBatchVerify is called from
// many ForkJoin / service threads in the reference: BLS.java:297-331,
// AggregatingSignatureVerificationService.java:122-129).  Inputs are copied
// into pinned staging on entry.  There is no CPU fallback.
#include <chrono>
#include <cstdlib>
#include <functional>
#include <cstring>
#include <mutex>
#include <algorithm>
#include <dlfcn.h>
#include <map>
#include <sys/random.h>
#include <rccl/rccl.h>  // types and prototypes only: RCCL is resolved with dlopen (gather_partials)
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/tekubls.h"
#include "tb_kdecl.h"
#include "tb_hrow.h"
#include "tb_host.h"
#include "tb_pkindex.h"  // the key table's index over its key bytes: hash, probe step, probe bound
#include "tb_pkcomb.h"   // the per-key comb rows: row size, reference words
#include "tb_plan.h"  // every host-side decision: kernel choice, pair split, product levels, workspace layout, placement
#include "tb_settle.h"  // the group-test descent of settling a failed batch
#include "tb_pack.h"  // the staging image of a host batch: set kinds, layout, fill
#include "tb_group.h"  // the sets of a batch grouped by message, and the grouped staging image
#include "tb_msgmemo.h"  // the hash-point memo: the host index over a device's resident rows, and the image's regions of a launch that resolved

static_assert(TB_PARTIAL_BYTES == TBLS_PARTIAL_BYTES, "partial record size");
static_assert(tb::plan::LINE_BYTES_PER_PAIR == TB_LINE_BYTES_PER_PAIR, "tb_plan.h: line bytes per pair");
static_assert(tb::plan::HROW_SET_BYTES == sizeof(tb::hrow_set), "tb_plan.h: row-hash workspace per set");
static_assert(tb::memo::SRC_ROW == TB_MEMO_SRC_ROW && tb::memo::LEARN_NONE == TB_MEMO_NONE, "tb_msgmemo.h: the words k_msgmemo.hip reads");

using tb::caller_device;
using namespace tb::plan;
using namespace tb::pack;
using namespace tb::group;

namespace {

#define HIPCHK(x)                      \
  do {                                 \
    hipError_t e_ = (x);               \
    if (e_ != hipSuccess) {            \
      last_hip_error() = e_;           \
      return TBLS_DEVICE_ERROR;        \
    }                                  \
  } while (0)

hipError_t& last_hip_error() {
  static thread_local hipError_t e = hipSuccess;
  return e;
}

// A growable buffer in device memory (HOST false) or pinned host memory, freed
// with its owner.  Growing frees the old block: the caller has drained its users.
template <bool HOST>
struct gbuf {
  void* p = nullptr;
  size_t cap = 0;
  gbuf() = default;
  gbuf(const gbuf&) = delete;
  gbuf& operator=(const gbuf&) = delete;
  ~gbuf() { release(); }
  // exact: a buffer of a fixed size gets no headroom for growing
  int ensure(size_t bytes, bool exact = false) {
    if (bytes <= cap) return 0;
    release();
    const size_t nb = bytes < 4096 ? 4096 : exact ? bytes : bytes + bytes / 4;
    if ((HOST ? hipHostMalloc(&p, nb, hipHostMallocDefault) : hipMalloc(&p, nb)) != hipSuccess) {
      p = nullptr;
      return -1;
    }
    cap = nb;
    return 0;
  }
  void release() {
    if (p) (void)(HOST ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as(size_t off = 0) const {
    return reinterpret_cast<T*>(static_cast<uint8_t*>(p) + off);
  }
};
using dbuf = gbuf<false>;
using hbuf = gbuf<true>;

// One library device: its streams, events and buffers, all owned -- created by
// init() or on first use, released by the destructor.
struct dev_ctx {
  int dev = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  dbuf in, ws;  // device input staging, pipeline workspace
  dbuf fin;     // the synchronous final verification's verdict word (under the device lock)
  dbuf dstb;    // default DST for the device-resident API
  hipStream_t aux[3] = {nullptr, nullptr, nullptr};  // concurrent per-set stages (aux[1] signatures + bucket sums, aux[2] hash_to_G2: high priority)
  dbuf tab_aff, tab_code;                    // device-resident public-key table (tbls_pk_table_load)
  uint32_t tab_n = 0;
  // The table's index over its compressed key bytes (tb_pkindex.h, built by
  // tbls_pk_table_load unless TBLS_PK_LOOKUP=0): the K keys as loaded, the
  // slots (pkx_cap of them, 0: no index) and the load's hash seed.  pkx_stat:
  // hits and misses of the batch key stages (two 64-bit words).  pkx_miss:
  // the key stage's miss list, count first (K + 1 words for a batch of K
  // keys); used between ws_acquire and ws_release like `ws`, and grown like it.
  dbuf tab_keys, pkx_slots, pkx_stat, pkx_miss;
  uint32_t pkx_cap = 0;
  uint64_t pkx_seed = 0;
  // The learned key cache (tb_pkindex.h pkx_cache): byte keys
  // that a key stage decompressed and found valid, kept with their points for
  // the next batches' lookups.  pkc_rows: its fixed capacity (0: off --
  // TBLS_PK_CACHE=0, TBLS_PK_LOOKUP=0 or TBLS_PK_CACHE_KEYS=0, read by
  // tbls_init, which also draws pkc_seed).  pkc: allocated by the first key
  // stage that looks up (pk_lookup_reserve) -- a head (PKC_HEAD bytes: the row
  // counter, then at byte 8 the TB_PKC_STATS counters), the slots, the rows'
  // keys, the rows' points.  Read and written by key stages only, between
  // ws_acquire and ws_release like `ws`.
  dbuf pkc;
  uint32_t pkc_rows = 0;
  uint64_t pkc_seed = 0;
  // The miss count of the device's latest key stage that looked keys up, as
  // far as it has arrived: k_pk_decompress_list stores its list's count into
  // this pinned word (pk_seen_dev: the word's device address), and nothing
  // waits for it.  pk_seen_K: the keys of the latest stage queued (0: none
  // yet).  launch_partial predicts from the two whether the next batch's keys
  // are known (pk_keys_known); a late or mismatched count only costs a stage
  // order.
  hbuf pk_seen;
  uint32_t* pk_seen_dev = nullptr;
  uint32_t pk_seen_K = 0;
  // The per-key comb rows (tb_pkcomb.h), unless TBLS_PK_COMB=0
  // (pkcomb_on, read by tbls_init).  pkcomb: the learned cache's region --
  // pkcomb_cap ready bytes (one per cache row below the cap: TBLS_PK_COMB_KEYS,
  // at most pkc_rows), then at a multiple of 256 bytes pkcomb_cap rows of
  // TB_PKCOMB_ROW_BYTES -- allocated with the cache (pk_lookup_reserve), its
  // ready bytes zeroed wherever the cache's slots are.  tab_comb: the loaded
  // table's region, a row per table key (tbls_pk_table_load).  A region that
  // cannot be allocated is given up (pkcomb_cap = 0 for the process; the table's
  // until the next load) and the device verifies as without it.  pk_ref: the
  // batch keys' reference words (k_pk_lookup_ref), a word per key, used and
  // grown like pkx_miss.  pkcomb_stat: four 64-bit counters (tbls_pk_comb_stats).
  bool pkcomb_on = false;
  uint32_t pkcomb_cap = 0;
  dbuf pkcomb, tab_comb, pk_ref, pkcomb_stat;
  // resident committees (tbls_committee_load): per slot TB_CM_STRIDE bytes of
  // cmt (members, bad-member mask, valid-member row, the valid members' sum,
  // the load pass's code and failure count); size 0: empty slot
  dbuf cmt;
  uint32_t cm_size[TBLS_COMMITTEE_SLOTS] = {0, 0, 0, 0}, cm_sum_ok[TBLS_COMMITTEE_SLOTS] = {0, 0, 0, 0};
  hipEvent_t e_fork = nullptr, e_join[3] = {nullptr, nullptr, nullptr}, e_sig = nullptr;
  hipEvent_t e_learn = nullptr;  // k_pk_learn has ended, on the key stream behind e_join[0] (launch_partial)
  // The hash-point memo (tb_msgmemo.h): the host index, read and
  // written under `mu` only, and the rows it speaks of -- memo.rows affine G2
  // points, then (at a multiple of 256 bytes) their skip bytes -- allocated by
  // the first shard that resolves (memo_reserve).  The rows are read by
  // k_memo_fill and written by k_memo_learn only, between ws_acquire and
  // ws_release like `ws`.  e_mlearn: k_memo_learn has ended, on the hash
  // stream behind e_join[2] (launch_partial).
  tb::memo::index memo;
  dbuf memo_rows;
  hipEvent_t e_mlearn = nullptr;
  hipEvent_t e_t0 = nullptr, e_t1 = nullptr;  // per-call device timing (shard_launch), created once
  // Last use of `ws` on any stream.  The device-resident API queues work on the
  // caller's stream and returns; every later user of `ws` (on whatever stream)
  // first waits for this event, then records it after its own work.
  hipEvent_t e_ws = nullptr;
  dbuf recs;  // partial records gathered for the final exponentiation (gather_partials, device 0)
  dbuf sws;   // settling a failed batch (settle_sets): per-set Miller values, group levels, test lists
  dbuf comb;  // (d 2^(8w)) g1 for w < 8, d < 256 (k_g1_comb_init): the signature pairs' G1 side
  hbuf hin, hout;
  int load = 0;  // batches placed on this device and not yet finished (g_place_mu)

  dev_ctx() = default;
  dev_ctx(const dev_ctx&) = delete;
  dev_ctx& operator=(const dev_ctx&) = delete;
  // The streams (signatures and hash at high priority), the events and the
  // comb table on hardware device hw; false: the context is to be deleted.
  bool init(int hw) {
    const auto ok = [](hipError_t e) { return e == hipSuccess; };
    const auto event = [&](hipEvent_t* e) { return ok(hipEventCreateWithFlags(e, hipEventDisableTiming)); };
    dev = hw;
    int prio_lo = 0, prio_hi = 0;
    if (!(ok(hipSetDevice(dev)) && ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) &&
          ok(hipStreamCreateWithFlags(&aux[0], hipStreamNonBlocking)) && ok(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi)) &&
          ok(hipStreamCreateWithPriority(&aux[1], hipStreamNonBlocking, prio_hi)) &&
          ok(hipStreamCreateWithPriority(&aux[2], hipStreamNonBlocking, prio_hi)) && event(&e_join[2]) && event(&e_fork) && event(&e_join[0]) &&
          event(&e_join[1]) && event(&e_sig) && event(&e_learn) && event(&e_mlearn) && event(&e_ws) && ok(hipEventCreate(&e_t0)) && ok(hipEventCreate(&e_t1)) &&
          !comb.ensure(TB_MSM_BUCKETS * sizeof(g1a))))
      return false;
    hipLaunchKernelGGL(k_g1_comb_init, dim3(TB_MSM_BUCKETS / TB_BLOCK), dim3(TB_BLOCK), 0, stream, comb.as<g1a>());
    return ok(hipGetLastError()) && ok(hipStreamSynchronize(stream));
  }
  // With the context's device current: the handles init() got as far as, then
  // (as members) every buffer.
  ~dev_ctx() {
    (void)hipSetDevice(dev);
    for (hipStream_t s : {stream, aux[0], aux[1], aux[2]})
      if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : {e_fork, e_join[0], e_join[1], e_join[2], e_sig, e_learn, e_mlearn, e_t0, e_t1, e_ws})
      if (e) (void)hipEventDestroy(e);
  }
};

// Order a new user of c.ws (on stream s) after the previous one; call
// ws_release after queueing the new work.
inline hipError_t ws_acquire(dev_ctx& c, hipStream_t s) { return hipStreamWaitEvent(s, c.e_ws, 0); }
inline hipError_t ws_release(dev_ctx& c, hipStream_t s) { return hipEventRecord(c.e_ws, s); }

std::mutex g_mu;
std::vector<dev_ctx*> g_ctx;
bool g_inited = false;
bool g_pk_lookup = true;  // TBLS_PK_LOOKUP=0 (read by tbls_init): no index, byte keys are always decompressed (A/B, parity tests)

uint32_t shard_min() { return plan_env::get().shard_min; }
uint32_t shard_knee() { return plan_env::get().shard_knee; }

// The live placement (tb_plan.h place_plan): plan under g_place_mu and count the batch on its
// devices until the guard ends.
std::mutex g_place_mu;
uint32_t g_place_rr = 0;
struct placed {
  int G = 0;
  std::vector<int> dev;
  std::vector<size_t> cut;
  placed() = default;
  placed(const placed&) = delete;
  placed& operator=(const placed&) = delete;
  ~placed() {
    std::lock_guard<std::mutex> lk(g_place_mu);
    for (int k = 0; k < G; k++) g_ctx[dev[k]]->load--;
  }
};
template <class KEYS>
void place_batch(placed& pl, size_t n, const KEYS& keys, int n_gpus, uint32_t smin, uint32_t knee) {
  std::lock_guard<std::mutex> lk(g_place_mu);
  const int D = (int)g_ctx.size();
  std::vector<int> load(D);
  for (int d = 0; d < D; d++) load[d] = g_ctx[d]->load;
  pl.dev.assign(D, 0);
  pl.cut.assign(D + 1, 0);
  pl.G = place_plan(n, keys, D, n_gpus, load.data(), g_place_rr++, smin, knee, pl.dev.data(), pl.cut.data());
  for (int k = 0; k < pl.G; k++) g_ctx[pl.dev[k]]->load++;
}
// one device for a whole call (single verifications, helpers)
void place_one(placed& pl) {
  place_batch(pl, 1, [](size_t) { return 1u; }, 0, 1, 0);
}


// Launch the partial pipeline for one device.  All pointers in `b` are
// device pointers.  Writes the 580-byte partial record at `partial_out`.
// Leaves per-set codes in the workspace (set_code/sig_code).
// Per-stage timing (optional): ev[2*i] / ev[2*i+1] bracket stage i on the
// stream that runs it.  Stages: 0 pk decompress, 1 set pk (+ -[r] g1), 2
// signature decode + G2 check, 3 hash, 4 bucket sums (large batches), 5
// Miller, 6 Fp12 product.
#define TB_NSTAGE 7
#define TB_NSTAGE_EV (2 * TB_NSTAGE)
// Streams: keys on aux[0], signatures (+ bucket sums) on aux[1], hash_to_G2
// on aux[2]; aux[1] and aux[2] at high priority; all three join the
// caller's stream before the Miller loops (the bucket-sum chain before the
// accumulator, acc_lds).  `serial`
// (the stage-profile API) runs everything on the caller's stream, for
// exclusive per-stage timings.
struct bits_src;
struct partial_opts {
  const uint8_t* dst;  // hash_to_G2 domain separation tag, device memory
  uint32_t dlen;
  hipEvent_t* ev = nullptr;
  bool serial = false;
  const uint32_t* key_idx = nullptr;  // keys = indices into the resident table: no decompression
  bool settle = false;                // the settle layout: per-set stages and the line kernel only (pair_plan)
  const bits_src* cm = nullptr;       // the sets are bit rows over a resident committee (key_idx: the rows)
  // A grouped launch (n_msgs < b.n; tb_group.h): b.msgs / b.msg_off hold the
  // n_msgs distinct messages, and the CSR (device memory) lists each one's sets.
  uint32_t n_msgs = 0;
  const uint32_t *grp_off = nullptr, *grp_sets = nullptr;
  // A launch that resolved its messages against the device's hash-point memo
  // (shard_launch, run_each): b.msgs / b.msg_off hold the m_hash messages left
  // to hash; src (a word per distinct message), learn (a word per hashed
  // message) and, for an ungrouped pass, set_grp (a word per set) are device
  // memory (tb_msgmemo.h).
  bool memo = false;
  uint32_t m_hash = 0;
  const uint32_t *memo_src = nullptr, *memo_learn = nullptr, *memo_setgrp = nullptr;
};

// The regions of a ws_layout as typed pointers into the workspace at w.
struct ws_ptrs {
  g1a *pk_aff, *P, *set_P, *grp_part;
  g2a *Q, *sig_aff, *Qh;
  uint8_t *pk_code, *skip, *set_code, *sig_code, *sig_use, *pair_code, *grp_pskip, *skiph;
  uint32_t *msm_cnt, *msm_off, *msm_cur, *msm_idx, *mlist, *mcnt, *n_bad, *grp_item;
  g2j* msm_sum;
  hrow_set* hrow;
  uint4* lines;
  fp12 *f, *fpart, *fpart2, *segv;
  ws_ptrs(const ws_layout& L, uint8_t* w)
      : pk_aff((g1a*)(w + L.pk_aff)), P((g1a*)(w + L.P)), set_P((g1a*)(w + L.set_P)), grp_part((g1a*)(w + L.grp_part)), Q((g2a*)(w + L.Q)),
        sig_aff((g2a*)(w + L.sig_aff)), pk_code(w + L.pk_code), skip(w + L.skip), set_code(w + L.set_code), sig_code(w + L.sig_code),
        sig_use(w + L.sig_use), pair_code(w + L.pair_code), grp_pskip(w + L.grp_pskip), msm_cnt((uint32_t*)(w + L.msm_cnt)),
        msm_off((uint32_t*)(w + L.msm_off)), msm_cur((uint32_t*)(w + L.msm_cur)), msm_idx((uint32_t*)(w + L.msm_idx)),
        mlist((uint32_t*)(w + L.mlist)), mcnt((uint32_t*)(w + L.mcnt)), n_bad((uint32_t*)(w + L.n_bad)), grp_item((uint32_t*)(w + L.grp_item)),
        msm_sum((g2j*)(w + L.msm_sum)),
        hrow((hrow_set*)(w + L.hrow)), lines((uint4*)(w + L.lines)), f((fp12*)(w + L.f)), fpart((fp12*)(w + L.fpart)),
        fpart2((fp12*)(w + L.fpart2)), segv((fp12*)(w + L.segv)) {
    Qh = (g2a*)(w + L.Qh);
    skiph = w + L.skiph;
  }
};

// The affine keys a stage reads, with their validity codes: the call's own
// decompressed keys (idx == nullptr, tab_n 0), or the resident table through
// the indices idx (for a committee's sets: their bit rows).
struct key_src {
  const g1a* aff;
  const uint8_t* code;
  const uint32_t* idx;
  uint32_t tab_n;
};
inline key_src own_keys(const g1a* aff, const uint8_t* code) { return {aff, code, nullptr, 0u}; }
inline key_src table_keys(const dev_ctx& c, const uint32_t* idx) { return {c.tab_aff.as<const g1a>(), c.tab_code.as<const uint8_t>(), idx, c.tab_n}; }

// Per-set aggregate key and P_i = [r_i] apk_i on stream s.  Single-key sets:
// one thread per set (k_set_pk, or its two-wave twin with w2: tb_plan.h
// use_w2).  When some set has several keys (multi: tb_plan.h multi_key),
// those sets go to the wave-level aggregation
// through a device-built work list (mlist / mcnt: n + 1 words of workspace).
// P2 (nullable): signature-pair points -[r_i] g1 (comb: the device's table).
// rows (nullable; pk_comb_rows): the device keeps comb rows for this batch's
// key source, and the two-wave kernel's place is k_set_pk_comb_w2's.
struct comb_rows {
  const uint32_t* pk_ref;             // byte keys: the lookup's reference words (nullptr by index)
  const g1a *cache_comb, *tab_comb;   // the regions' rows (nullptr: none)
  unsigned long long* stat;
};
void launch_set_pk(hipStream_t s, uint32_t n, bool w2, uint32_t multi, const uint32_t* pk_off, const key_src& ks, const uint64_t* rand, g1a* P,
                   uint8_t* set_code, uint32_t* n_bad, uint32_t* mlist, uint32_t* mcnt, g1a* P2, const g1a* comb, const comb_rows* rows = nullptr) {
  if (!n) return;
  const dim3 blk(TB_BLOCK), g((n + TB_BLOCK - 1) / TB_BLOCK);
  if (w2 && rows)
    hipLaunchKernelGGL(k_set_pk_comb_w2, g, blk, 0, s, pk_off, ks.aff, ks.code, rand, n, P, set_code, n_bad, ks.idx, ks.tab_n, multi, P2, comb,
                       rows->pk_ref, rows->cache_comb, rows->tab_comb, rows->stat);
  else
    hipLaunchKernelGGL(w2 ? k_set_pk_w2 : k_set_pk, g, blk, 0, s, pk_off, ks.aff, ks.code, rand, n, P, set_code, n_bad, ks.idx, ks.tab_n, multi, P2,
                       comb);
  if (!multi) return;
  (void)hipMemsetAsync(mcnt, 0, 4, s);
  hipLaunchKernelGGL(k_multi_list, g, blk, 0, s, pk_off, n, mlist, mcnt);
  if (multi == 2)
    hipLaunchKernelGGL(k_set_pk_agg_coop, dim3(std::min<uint32_t>(n, 4096u)), dim3(512), 0, s, pk_off, ks.aff, ks.code, rand,
                       (const uint32_t*)mlist, (const uint32_t*)mcnt, P, set_code, n_bad, ks.idx, ks.tab_n, P2, comb, 0u);
  else
    hipLaunchKernelGGL(k_set_pk_wave, dim3(std::min<uint32_t>(n, 4096u)), dim3(64), 0, s, pk_off, ks.aff, ks.code, rand,
                       (const uint32_t*)mlist, (const uint32_t*)mcnt, P, set_code, n_bad, ks.idx, ks.tab_n);
}

// A resident committee on one device (dev_ctx::cmt) and the bit rows' stride.
#define TB_CM_WORDS (TBLS_COMMITTEE_MAX / 32)
#define TB_CM_OFF_BAD ((size_t)TBLS_COMMITTEE_MAX * 4)
#define TB_CM_OFF_VALID (TB_CM_OFF_BAD + 256)
#define TB_CM_OFF_SUM (TB_CM_OFF_VALID + 256)
#define TB_CM_OFF_CODE (TB_CM_OFF_SUM + 256)
#define TB_CM_STRIDE (TB_CM_OFF_CODE + 256)
struct bits_src {
  const uint32_t *members, *bad;
  const g1a* sum;
  uint32_t size, sum_ok, stride_w;
};
inline bits_src committee_src(const dev_ctx& c, uint32_t slot) {
  const uint8_t* m = c.cmt.as<const uint8_t>((size_t)slot * TB_CM_STRIDE);
  return {(const uint32_t*)m, (const uint32_t*)(m + TB_CM_OFF_BAD), (const g1a*)(m + TB_CM_OFF_SUM), c.cm_size[slot], c.cm_sum_ok[slot],
          bits_stride_w(c.cm_size[slot])};
}

// launch_set_pk for sets given as participation bit rows over a resident
// committee (ks.idx: n rows of cm.stride_w words): one kernel, every set on the
// lane-cooperative rows (k_set_pk_bits_coop), keys from the table.  unit_r: r = 1.
void launch_set_pk_bits(hipStream_t s, uint32_t n, const key_src& ks, const bits_src& cm, const uint64_t* rand, g1a* P, uint8_t* set_code,
                        uint32_t* n_bad, g1a* P2, const g1a* comb, uint32_t unit_r) {
  if (!n) return;
  hipLaunchKernelGGL(k_set_pk_bits_coop, dim3(std::min<uint32_t>(n, 4096u)), dim3(512), 0, s, ks.idx, cm.stride_w, cm.members, cm.size, cm.bad,
                     cm.sum, cm.sum_ok, ks.aff, ks.code, ks.tab_n, rand, n, P, set_code, n_bad, P2, comb, unit_r);
}

#define TB_PKX_BLOCK 256u  // threads per workgroup of the key index's kernels (k_pkindex.hip)

// The widest loads a key array at p allows (k_pkindex.hip pkx_load_key).
inline uint32_t pkx_align(const void* p) {
  const uintptr_t a = (uintptr_t)p;
  return !(a & 15u) ? 16u : !(a & 3u) ? 4u : 1u;
}

// True when byte keys on c resolve from the table's index.
inline bool pk_table_index_on(const dev_ctx& c) { return c.tab_n && c.pkx_cap; }
// True when byte keys on c are looked up before they are decompressed: in the
// table's index, in the learned cache, or in both.
inline bool pk_lookup_on(const dev_ctx& c) { return pk_table_index_on(c) || c.pkc_rows; }

// The learned cache's buffer (dev_ctx::pkc) and the view its kernels take
// (slots == nullptr: the device has no cache).
#define PKC_HEAD 64u
inline size_t pkc_zeroed_bytes(const dev_ctx& c) { return PKC_HEAD + (size_t)tb::pkx_capacity(c.pkc_rows) * 4; }  // the head and the slots
inline tb::pkx_cache pk_cache_view(const dev_ctx& c) {
  if (!c.pkc_rows || !c.pkc.p) return {nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0};
  const size_t o_keys = pkc_zeroed_bytes(c), o_points = o_keys + (size_t)c.pkc_rows * 48;
  return {c.pkc.as<uint32_t>(PKC_HEAD), tb::pkx_capacity(c.pkc_rows) - 1u, c.pkc.as<uint32_t>(o_keys), c.pkc.as<uint32_t>(o_points), c.pkc_rows,
          c.pkc.as<uint32_t>(0), c.pkc.as<unsigned long long>(8), c.pkc_seed};
}

// The comb regions (dev_ctx::pkcomb, tab_comb) as the kernels take them.
inline size_t pkcomb_rows_off(const dev_ctx& c) { return align_up((size_t)c.pkcomb_cap); }  // behind the ready bytes
inline bool pk_cache_comb_on(const dev_ctx& c) { return c.pkcomb_on && c.pkc_rows && c.pkc.p && c.pkcomb_cap && c.pkcomb.p; }
inline bool pk_table_comb_on(const dev_ctx& c) { return c.pkcomb_on && c.tab_n && c.tab_comb.p; }
// Byte keys on c get reference words from their lookup (k_pk_lookup_ref).
inline bool pk_refs_on(const dev_ctx& c) { return pk_cache_comb_on(c) || (pk_table_index_on(c) && pk_table_comb_on(c)); }
// The rows launch_set_pk reads for a batch whose keys are table indices
// (by_index) or bytes that were looked up; false: the device has none for it.
inline bool pk_comb_rows(const dev_ctx& c, bool by_index, comb_rows& r) {
  if (by_index ? !pk_table_comb_on(c) : !(pk_lookup_on(c) && pk_refs_on(c))) return false;
  r.pk_ref = by_index ? nullptr : c.pk_ref.as<const uint32_t>();
  r.cache_comb = pk_cache_comb_on(c) ? c.pkcomb.as<const g1a>(pkcomb_rows_off(c)) : nullptr;
  r.tab_comb = pk_table_comb_on(c) ? c.tab_comb.as<const g1a>() : nullptr;
  r.stat = c.pkcomb_stat.as<unsigned long long>();
  return true;
}

// Room for the miss list of a K-key stage, and the learned cache on its first
// use; the caller holds the workspace (ws_acquire) and `s` orders every
// earlier user of it, so growing drains s first, as the workspace does.  A
// cache that cannot be allocated is given up for the process (pkc_rows = 0):
// the device goes on as without one, it does not fail its batches.
int pk_lookup_reserve(dev_ctx& c, uint32_t K, hipStream_t s) {
  if (!K) return TBLS_SUCCESS;
  if (c.pkc_rows && !c.pkc.p) {  // an empty cache: the counters and every slot 0; the rows need no clearing
    if (c.pk_seen.ensure(64) || hipHostGetDevicePointer((void**)&c.pk_seen_dev, c.pk_seen.p, 0) != hipSuccess ||
        c.pkc.ensure(pkc_zeroed_bytes(c) + (size_t)c.pkc_rows * (48 + sizeof(g1a)), true)) {
      (void)hipGetLastError();
      c.pkc.release();
      c.pkc_rows = 0;
      c.pk_seen_dev = nullptr;
    } else {
      *c.pk_seen.as<uint32_t>() = 0xffffffffu;  // until the first count arrives: every key a miss
      HIPCHK(hipMemsetAsync(c.pkc.p, 0, pkc_zeroed_bytes(c), s));
    }
  }
  // the cache's comb region with it: no row ready.  One that cannot be
  // allocated is given up for the process too (TBLS_INIT_SHARE_DEVICES puts up
  // to 32 contexts on one GPU): the device verifies as without comb rows.
  if (c.pkcomb_on && c.pkcomb_cap && !c.pkcomb.p) {
    c.pkcomb_cap = std::min(c.pkcomb_cap, c.pkc_rows);
    if (!c.pkc.p || !c.pkcomb_cap || c.pkcomb.ensure(pkcomb_rows_off(c) + (size_t)c.pkcomb_cap * TB_PKCOMB_ROW_BYTES, true)) {
      (void)hipGetLastError();
      c.pkcomb.release();
      c.pkcomb_cap = 0;
    } else {
      HIPCHK(hipMemsetAsync(c.pkcomb.p, 0, c.pkcomb_cap, s));
    }
  }
  if (!pk_lookup_on(c)) return TBLS_SUCCESS;
  const size_t need = ((size_t)K + 1) * 4;
  if (need <= c.pkx_miss.cap && (!pk_refs_on(c) || need <= c.pk_ref.cap)) return TBLS_SUCCESS;
  HIPCHK(hipStreamSynchronize(s));
  if (c.pkx_miss.ensure(need)) return TBLS_DEVICE_ERROR;
  return pk_refs_on(c) && c.pk_ref.ensure(need) ? TBLS_DEVICE_ERROR : TBLS_SUCCESS;
}

// The key stage of K byte keys: affine points and validity codes into pk_aff /
// pk_code.  With a lookup on the device (pk_lookup_on, pk_lookup_reserve
// called) it is three steps: launch_pk_lookup -- k_pk_lookup copies the keys
// that the table's index or the learned cache knows and lists the others --
// then k_pk_decompress_list decompresses that list, and with a cache
// launch_pk_learn -- k_pk_learn appends the list's valid keys to it.  The same
// bytes give the same point and code either way, since the table's entries
// came from k_pk_decompress and the cache's rows from k_pk_decompress_list.
// Without a lookup: k_pk_decompress over all K.  launch_byte_keys queues the
// stage on s; looked_up: the caller has queued launch_pk_lookup already, on a
// stream s waits for; learn false: the caller queues launch_pk_learn itself,
// behind the kernels that wait for the keys (launch_partial).
int launch_pk_lookup(dev_ctx& c, hipStream_t s, const uint8_t* pks, uint32_t K, g1a* pk_aff, uint8_t* pk_code) {
  uint32_t* miss = c.pkx_miss.as<uint32_t>();
  HIPCHK(hipMemsetAsync(miss, 0, 4, s));
  const bool tab = pk_table_index_on(c);
  if (pk_refs_on(c)) {  // a device with comb rows: the keys' reference words too (k_set_pk_comb_w2 reads them)
    const bool cc = pk_cache_comb_on(c);
    hipLaunchKernelGGL(k_pk_lookup_ref, dim3((K + TB_PKX_BLOCK - 1) / TB_PKX_BLOCK), dim3(TB_PKX_BLOCK), 0, s, pks, K, pkx_align(pks),
                       tab ? c.pkx_slots.as<const uint32_t>() : nullptr, tab ? c.pkx_cap - 1u : 0u, c.pkx_seed, c.tab_keys.as<const uint32_t>(),
                       c.tab_aff.as<const g1a>(), c.tab_code.as<const uint8_t>(), pk_cache_view(c), pk_aff, pk_code, miss,
                       c.pkx_stat.as<unsigned long long>(), c.pk_ref.as<uint32_t>(), cc ? c.pkcomb.as<const uint8_t>() : nullptr,
                       cc ? c.pkcomb_cap : 0u, pk_table_comb_on(c) ? 1u : 0u);
    return TBLS_SUCCESS;
  }
  hipLaunchKernelGGL(k_pk_lookup, dim3((K + TB_PKX_BLOCK - 1) / TB_PKX_BLOCK), dim3(TB_PKX_BLOCK), 0, s, pks, K, pkx_align(pks),
                     tab ? c.pkx_slots.as<const uint32_t>() : nullptr, tab ? c.pkx_cap - 1u : 0u, c.pkx_seed, c.tab_keys.as<const uint32_t>(),
                     c.tab_aff.as<const g1a>(), c.tab_code.as<const uint8_t>(), pk_cache_view(c), pk_aff, pk_code, miss,
                     c.pkx_stat.as<unsigned long long>());
  return TBLS_SUCCESS;
}
// The comb builders' grid: workgroups of TB_PKCOMB_BLOCK threads that walk
// their list with the grid's stride, at most 1,024 of them (the list's length
// is only known on the device, and a batch without misses should launch little).
inline dim3 pkcomb_grid(uint32_t K) { return dim3(std::min<uint32_t>((K + TB_PKCOMB_BLOCK - 1) / TB_PKCOMB_BLOCK, 1024u)); }
void launch_pk_learn(dev_ctx& c, hipStream_t s, const uint8_t* pks, uint32_t K, const g1a* pk_aff, const uint8_t* pk_code) {
  if (!K || !c.pkc_rows) return;
  if (pk_cache_comb_on(c)) {  // the append, and the comb rows of the keys it publishes
    hipLaunchKernelGGL(k_pk_learn_comb, pkcomb_grid(K), dim3(TB_PKCOMB_BLOCK), 0, s, pks, pkx_align(pks), c.pkx_miss.as<const uint32_t>(), pk_aff,
                       pk_code, pk_cache_view(c), c.pkcomb.as<g1a>(pkcomb_rows_off(c)), c.pkcomb.as<uint8_t>(), c.pkcomb_cap,
                       c.pkcomb_stat.as<unsigned long long>());
    return;
  }
  hipLaunchKernelGGL(k_pk_learn, dim3((K + TB_PKX_BLOCK - 1) / TB_PKX_BLOCK), dim3(TB_PKX_BLOCK), 0, s, pks, pkx_align(pks),
                     c.pkx_miss.as<const uint32_t>(), pk_aff, pk_code, pk_cache_view(c));
}
int launch_byte_keys(dev_ctx& c, hipStream_t s, const uint8_t* pks, uint32_t K, g1a* pk_aff, uint8_t* pk_code, bool looked_up = false,
                     bool learn = true) {
  if (!K) return TBLS_SUCCESS;
  const dim3 blk(TB_BLOCK), g((K + TB_BLOCK - 1) / TB_BLOCK);
  if (!pk_lookup_on(c)) {
    hipLaunchKernelGGL(k_pk_decompress, g, blk, 0, s, pks, K, pk_aff, pk_code);
    return TBLS_SUCCESS;
  }
  if (!looked_up)
    if (const int rc = launch_pk_lookup(c, s, pks, K, pk_aff, pk_code)) return rc;
  // the grids cover K: the list's length is only known on the device
  hipLaunchKernelGGL(k_pk_decompress_list, g, blk, 0, s, pks, c.pkx_miss.as<const uint32_t>(), pk_aff, pk_code,
                     c.pkc_rows ? c.pk_seen_dev : nullptr);
  if (learn) launch_pk_learn(c, s, pks, K, pk_aff, pk_code);
  if (c.pkc_rows) c.pk_seen_K = K;
  return TBLS_SUCCESS;
}

// The prediction that a batch's byte keys are in the learned cache (taken from
// it, not decompressed): at most 1/8 of the latest key stage's keys were
// misses.  Validator keys are a stable registry, so the last batch is the
// best cheap predictor; below 1/8 the decompression beside the signature
// checks is under 0.4 ms of the 3.2 ms it takes for a whole 131,072-key batch
// (the shares in between are not measured).  Only with a cache: without one
// the launches and their order are the parent's.  TB_PK_KNOWN_ORDER=0 builds
// a library that never predicts, for the A/B of the two orders
// (tools/build_variant.py).
#ifndef TB_PK_KNOWN_ORDER
#define TB_PK_KNOWN_ORDER 1
#endif
inline bool pk_keys_known(const dev_ctx& c) {
  if (!TB_PK_KNOWN_ORDER || !c.pkc_rows || !c.pk_seen_K || !c.pk_seen.p) return false;
  const uint32_t miss = *static_cast<const volatile uint32_t*>(c.pk_seen.p);
  return (uint64_t)miss * 8 <= c.pk_seen_K;
}

// The memo's kernels: TB_MEMO_CHUNKS threads per point; the rows' skip bytes
// follow the memo.rows points of dev_ctx::memo_rows.
inline dim3 memo_grid(uint32_t points) { return dim3((uint32_t)(((uint64_t)points * TB_MEMO_CHUNKS + TB_MEMO_BLOCK - 1) / TB_MEMO_BLOCK)); }
inline size_t memo_skip_off(uint32_t rows) { return align_up((size_t)rows * sizeof(g2a)); }
inline uint8_t* memo_row_skip(const dev_ctx& c) { return c.memo_rows.as<uint8_t>(memo_skip_off(c.memo.rows)); }
static_assert(sizeof(g2a) % 16 == 0, "the rows are copied as 16-byte words: hipMalloc's base and every row are 16-byte aligned");

// The Miller line kernel of a line group (tb_plan.h line_group): a lane quad,
// a lane pair or one lane per pair.
inline auto line_kernel_of(int lg) { return lg == 4 ? k_miller_lines_quad : lg == 2 ? k_miller_lines_duo : k_miller_lines_w2; }

// One launch_partial call: the batch, its plan, the workspace and the streams
// of its chains.  Each chain queues on one stream, in order; launch_partial
// forks and joins them.
struct partial_run {
  dev_ctx& c;
  const tbls_dev_batch& b;
  const partial_opts& o;
  const batch_plan& bp;
  const ws_ptrs& W;
  const key_src& keys;
  hipStream_t s, sa, sb, sh;  // the caller's, keys, signatures + bucket sums, hash
  bool late_join;             // bp.late_join with the streams side by side
  // Byte keys on a device that looks them up (pk_lookup_on): launch_partial
  // has queued the lookup on the caller's stream ahead of the fork, and the
  // key stream starts at the misses.
  bool pre_lookup;
  const uint32_t n = b.n;
  const dim3 blk = dim3(TB_BLOCK), g = dim3((b.n + TB_BLOCK - 1) / TB_BLOCK);  // one thread per set
  g1a* sig_P() const { return bp.pp.msm ? nullptr : W.P + n; }                 // -[r_i] g1 of the sets' signature pairs
  // A grouped plan (tb_plan.h pair_plan): nh messages and main pairs, the
  // signature side from pair xo on, the sets' [r_i] apk_i in a region of their
  // own, and the pairs' own code rows (set_code / sig_code are per set there).
  const uint32_t nh = bp.pp.n_msgs, xo = bp.pp.x_first();
  const dim3 gh = dim3((bp.pp.n_msgs + TB_BLOCK - 1) / TB_BLOCK);  // one thread per message
  g1a* set_P() const { return bp.pp.grouped ? W.set_P : W.P; }
  uint8_t* code_a() const { return bp.pp.grouped ? W.pair_code : W.set_code; }
  uint8_t* code_b() const { return bp.pp.grouped ? W.pair_code + align_up(bp.pp.n_pairs) : W.sig_code; }

#define TB_EV(i, st) \
  if (o.ev) HIPCHK(hipEventRecord(o.ev[i], st))

  // --- stream b: signatures, then (large batches) the bucket sums -----------
  int sig_chain() const {
    const pair_plan& pp = bp.pp;
    if (pp.msm) {  // bucket sort by randomizer byte (randomizers only)
      HIPCHK(hipMemsetAsync(W.msm_cnt, 0, TB_MSM_BUCKETS * 4, sb));
      hipLaunchKernelGGL(k_msm_hist, g, blk, 0, sb, b.rand, n, W.msm_cnt);
      hipLaunchKernelGGL(k_msm_scan, dim3(1), dim3(256), 0, sb, (const uint32_t*)W.msm_cnt, W.msm_off, W.msm_cur);
      hipLaunchKernelGGL(k_msm_scatter, g, blk, 0, sb, b.rand, n, W.msm_cur, W.msm_idx);
    }
    TB_EV(4, sb);
    if (n) {
      const auto check = bp.w2 ? k_sig_check_w2 : k_sig_check;
      if (bp.sig == sig_kind::msm)
        hipLaunchKernelGGL(check, g, blk, 0, sb, b.sigs, n, W.sig_aff, W.sig_use, W.sig_code, W.n_bad, 0u);
      else if (bp.sig == sig_kind::coop)
        hipLaunchKernelGGL(k_sig_check_coop, dim3((n + 3) / 4), dim3(64), 0, sb, b.sigs, n, W.Q + n, W.skip + n, W.sig_code, W.n_bad);
      else
        hipLaunchKernelGGL(check, g, blk, 0, sb, b.sigs, n, W.Q + n, W.skip + n, W.sig_code, W.n_bad, 1u);
    }
    TB_EV(5, sb);
    if (late_join) HIPCHK(hipEventRecord(c.e_sig, sb));  // the signature codes are there (batch_plan::late_join)
    TB_EV(8, sb);
    if (pp.msm) {
      hipLaunchKernelGGL(k_msm_bucket_tree, dim3(TB_MSM_TREE_WG), dim3(64), 0, sb, (const g2a*)W.sig_aff, (const uint8_t*)W.sig_use,
                         (const uint32_t*)W.msm_off, (const uint32_t*)W.msm_idx, W.msm_sum);
      hipLaunchKernelGGL(k_msm_bitsum_pairs, dim3(TB_MSM_XPAIRS), dim3(64), 0, sb, (const g2j*)W.msm_sum, c.comb.as<const g1a>(), W.P + xo,
                         W.Q + xo, W.skip + xo);
      if (pp.n_xwave)  // their Miller loops, one wave each, on this stream: f[n_f_main ..)
        hipLaunchKernelGGL(k_miller_wave, dim3(pp.n_xwave), dim3(64), 0, sb, (const g1a*)W.P + xo, (const g2a*)W.Q + xo,
                           (const uint8_t*)W.skip + xo, (const uint8_t*)code_a() + xo, (const uint8_t*)code_b() + xo, pp.n_xwave,
                           W.f + pp.n_f_main());
    }
    TB_EV(9, sb);
    return TBLS_SUCCESS;
  }

  // --- stream a: public keys, [r] apk (+ -[r] g1 for the signature pairs) -----
  int key_chain() const {
    const g1a* comb = c.comb.as<const g1a>();
    if (!pre_lookup) TB_EV(0, sa);  // else recorded before the lookup (launch_partial)
    if (bp.key == key_kind::bits) {
      TB_EV(1, sa);
      TB_EV(2, sa);
      launch_set_pk_bits(sa, n, keys, *o.cm, b.rand, set_P(), W.set_code, W.n_bad, sig_P(), comb, 0u);
    } else if (bp.key == key_kind::keys_coop) {  // one kernel; its time shows as stage 0
      const bool tab = keys.idx != nullptr;
      hipLaunchKernelGGL(k_keys_coop, dim3((n + 3) / 4), dim3(128), 0, sa, tab ? nullptr : b.pks, b.pk_off, tab ? keys.aff : nullptr,
                         tab ? keys.code : nullptr, keys.idx, keys.tab_n, b.rand, n, set_P(), sig_P(), W.set_code, W.n_bad, comb);
      TB_EV(1, sa);
      TB_EV(2, sa);
    } else {
      if (const int rc = launch_byte_keys(c, sa, b.pks, bp.n_keys, W.pk_aff, W.pk_code, pre_lookup, false)) return rc;  // learnt behind the join (launch_partial)
      TB_EV(1, sa);
      TB_EV(2, sa);
      comb_rows rows;
      const bool has_rows = pk_comb_rows(c, keys.idx != nullptr, rows);  // byte keys: the lookup wrote their references
      launch_set_pk(sa, n, bp.w2, bp.multi, b.pk_off, keys, b.rand, set_P(), W.set_code, W.n_bad, W.mlist, W.mcnt, sig_P(), comb,
                    has_rows ? &rows : nullptr);
    }
    if (bp.pp.grouped) group_sums();
    TB_EV(3, sa);
    return TBLS_SUCCESS;
  }

  // --- grouped plans, on the key stream after the key stage: the main pairs'
  // G1 side, P[g] = sum of the group's [r_i] apk_i (k_group_pk_sum_coop).  An
  // infinite sum is flagged in the pair's first code byte, which the Miller
  // kernels read like skip: the hash stream owns skip[g] at this time.
  void group_sums() const {
    const uint32_t walk = group_walk(n), items_max = group_items_max(n, nh);
    const bool split = n > walk;  // else no group has more than one item
    const uint32_t* item_first = split ? W.grp_item : nullptr;
    if (split) hipLaunchKernelGGL(k_group_items, dim3(1), dim3(256), 0, sa, o.grp_off, nh, n, walk, W.grp_item);
    for (uint32_t pass = 0; pass < (split ? 2u : 1u); pass++)
      hipLaunchKernelGGL(k_group_pk_sum_coop, dim3(std::min<uint32_t>(pass ? nh : items_max, 4096u)), dim3(512), 0, sa, (const g1a*)W.set_P,
                         (const uint8_t*)W.set_code, n, o.grp_off, o.grp_sets, item_first, nh, walk, items_max, pass, W.P, code_a(), W.grp_part,
                         W.grp_pskip);
  }

  // --- high-priority stream: hash_to_G2 per set -------------------------------
  // The longest per-set stage (2 wave rounds at 131k sets): with queue
  // priority its waves are dispatched first and the shorter key / signature
  // stages fill the SIMDs around them, instead of its last waves running
  // alone after the others finish.
  // With the memo (bp.memo) the kernels hash the bp.n_hash messages the host
  // left into Qh / skiph, and k_memo_fill then gives every main pair its Q
  // and skip byte from there or from the device's rows: with nothing left to
  // hash it is the only kernel on this stream.
  int hash_chain() const {
    g2a* Q = bp.memo ? W.Qh : W.Q;
    uint8_t* skip = bp.memo ? W.skiph : W.skip;
    const uint32_t nh = bp.n_hash;
    const dim3 gh((nh + TB_BLOCK - 1) / TB_BLOCK);  // one thread per message to hash
    TB_EV(6, sh);
    switch (bp.hash) {
      case hash_kind::none:
        break;
      case hash_kind::coop:
        hipLaunchKernelGGL(k_set_hash_coop, dim3(nh), dim3(256), 0, sh, b.msgs, b.msg_off, o.dst, o.dlen, nh, Q, skip, (const uint64_t*)nullptr);
        break;
      case hash_kind::wave:
        hipLaunchKernelGGL(k_set_hash_wave, dim3(nh), dim3(128), 0, sh, b.msgs, b.msg_off, o.dst, o.dlen, nh, Q, skip);
        break;
      case hash_kind::row: {
        hrow_set* H = W.hrow;
        hipLaunchKernelGGL(k_hrow_field, gh, blk, 0, sh, b.msgs, b.msg_off, o.dst, o.dlen, nh, H);
        hipLaunchKernelGGL(k_hrow_sswu, dim3((2 * nh + 3) / 4), dim3(64), 0, sh, nh, H);
        hipLaunchKernelGGL(k_hrow_iso, gh, blk, 0, sh, nh, H);
        hipLaunchKernelGGL(k_hrow_cof, dim3((nh + 3) / 4), dim3(64), 0, sh, nh, (const hrow_set*)H, Q, skip, 0);
        hipLaunchKernelGGL(k_hrow_fix, gh, blk, 0, sh, nh, (const hrow_set*)H, Q, skip);
        break;
      }
      case hash_kind::quad:
        hipLaunchKernelGGL(k_set_hash_quad, dim3((4 * nh + TB_BLOCK - 1) / TB_BLOCK), blk, 0, sh, b.msgs, b.msg_off, o.dst, o.dlen, nh, Q, skip);
        break;
      case hash_kind::duo:
        hipLaunchKernelGGL(k_set_hash_duo, dim3((2 * nh + TB_BLOCK - 1) / TB_BLOCK), blk, 0, sh, b.msgs, b.msg_off, o.dst, o.dlen, nh, Q, skip);
        break;
      case hash_kind::w2:
        // the chains' affine addends wait in the line buffer (19,584 B per pair,
        // unused until the line kernel, which runs after this stream joins)
        hipLaunchKernelGGL(k_set_hash_w2, gh, blk, 0, sh, b.msgs, b.msg_off, o.dst, o.dlen, nh, Q, skip, (g2a*)W.lines);
        break;
      case hash_kind::lane:
        hipLaunchKernelGGL(k_set_hash, gh, blk, 0, sh, b.msgs, b.msg_off, o.dst, o.dlen, nh, Q, skip);
        break;
    }
    if (bp.hash == hash_kind::quad || bp.hash == hash_kind::duo || bp.hash == hash_kind::w2)  // the exact formulas for the sets it flags (skip == 2)
      hipLaunchKernelGGL(k_set_hash_fix, gh, blk, 0, sh, b.msgs, b.msg_off, o.dst, o.dlen, nh, Q, skip);
    if (bp.memo && bp.pp.n_msgs)
      hipLaunchKernelGGL(k_memo_fill, memo_grid(bp.pp.n_msgs), dim3(TB_MEMO_BLOCK), 0, sh, o.memo_src, o.memo_setgrp, bp.pp.n_msgs,
                         (const g2a*)W.Qh, (const uint8_t*)W.skiph, c.memo_rows.as<const g2a>(), memo_row_skip(c), W.Q, W.skip);
    TB_EV(7, sh);
    return TBLS_SUCCESS;
  }
  // the rows learn the hashed messages the host gave a row (launch_partial queues it behind the join)
  void memo_learn() const {
    hipLaunchKernelGGL(k_memo_learn, memo_grid(bp.n_hash), dim3(TB_MEMO_BLOCK), 0, sh, o.memo_learn, bp.n_hash, (const g2a*)W.Qh,
                       (const uint8_t*)W.skiph, c.memo_rows.as<g2a>(), memo_row_skip(c));
  }

  // --- Miller loops of all pairs (pairs of invalid sets contribute 1) ---------
  int miller() const {
    const pair_plan& pp = bp.pp;
    const uint32_t np = pp.n_pairs;
    const g1a* P = W.P;
    const g2a* Q = W.Q;
    const uint8_t *skip = W.skip, *ca = code_a(), *cb = code_b();
    TB_EV(10, s);
    if (!np) return TBLS_SUCCESS;
    if (pp.wave) {
      hipLaunchKernelGGL(k_miller_wave, dim3(np), dim3(64), 0, s, P, Q, skip, ca, cb, np, W.f);
      return TBLS_SUCCESS;
    }
    // chunks of the main pairs: G2 lines (P and T in LDS), then the Fp12
    // accumulator (segment-major values: segment j of group g at f[j * n_groups + g])
    const uint4* lines = W.lines;
    const auto line_kernel = line_kernel_of(bp.line_group);  // mid-size batches: a lane group per pair
    for (uint32_t lo = 0; lo < pp.n_main; lo += TB_LINE_CHUNK) {
      const uint32_t m = std::min(TB_LINE_CHUNK, pp.n_main - lo), mt = (m + pp.per - 1) / pp.per;
      hipLaunchKernelGGL(line_kernel, dim3((bp.line_group * m + TB_BLOCK - 1) / TB_BLOCK), blk, 0, s, P + lo, Q + lo, skip + lo, ca + lo, cb + lo, m,
                         W.lines);
      if (o.settle) continue;  // settle_sets accumulates per set from these lines
      if (late_join && lo == 0) HIPCHK(hipStreamWaitEvent(s, c.e_join[1], 0));  // the bucket-sum stream first (acc_lds)
      if (pp.seg()) {
        const uint32_t g_pad = (mt + TB_BLOCK - 1) / TB_BLOCK * TB_BLOCK;
        hipLaunchKernelGGL(k_miller_accs_lds, dim3(pp.nseg * g_pad / TB_BLOCK), blk, 0, s, lines, skip + lo, ca + lo, cb + lo, m, pp.per, pp.nseg,
                           g_pad, W.f + lo / pp.per, pp.n_groups());
      } else {
        hipLaunchKernelGGL(pp.per == 2 ? k_miller_acc2 : k_miller_acc1, dim3((mt + TB_BLOCK - 1) / TB_BLOCK), blk, 0, s, lines, skip + lo, ca + lo,
                           cb + lo, m, W.f + lo / pp.per);
      }
    }
    return TBLS_SUCCESS;
  }

  // --- the partial: the product of the Miller values, by the plan's levels ----
  int product_tree(void* partial_out) const {
    TB_EV(12, s);
    if (bp.pp.n_f() == 0) {  // no pairs at all: the partial product is 1
      HIPCHK(hipMemsetAsync(W.f, 0, sizeof(fp12), s));
      hipLaunchKernelGGL(k_fp12_one, dim3(1), dim3(64), 0, s, W.f);
    }
    const fp12* src = W.f;
    for (int i = 0; i < bp.n_levels; i++) {
      const prod_level& l = bp.levels[i];
      fp12* out = l.dst == prod_dst::partial ? (fp12*)partial_out : l.dst == prod_dst::segv ? W.segv : l.dst == prod_dst::fpart2 ? W.fpart2 : W.fpart;
      if (l.seg)
        hipLaunchKernelGGL(k_fp12_prod_wave_seg, dim3(l.n_out, bp.pp.nseg), dim3(64), 0, s, src, l.n_in, l.n_in_last, bp.pp.nseg, l.in_stride,
                           l.chunk, out, l.out_stride);
      else
        hipLaunchKernelGGL(k_fp12_prod_wave, dim3(l.n_out), dim3(64), 0, s, src, l.n_in, l.chunk, out);
      src = out;
    }
    if (bp.combine)  // the Horner combine of the segment products
      hipLaunchKernelGGL(k_fp12_seg_combine_coop, dim3(1), dim3(TB_CFE_THREADS), 0, s, (const fp12*)W.segv, bp.pp.nseg, 0u, (fp12*)partial_out);
    TB_EV(13, s);
    return TBLS_SUCCESS;
  }
};

int launch_partial(dev_ctx& c, const tbls_dev_batch& b, hipStream_t s, void* partial_out, ws_layout& L, const partial_opts& o) {
  const batch_plan bp(b.n, b.n_keys, o.cm ? key_source::bits : o.key_idx ? key_source::table : key_source::bytes, o.settle, plan_env::get(),
                      o.grp_off && o.grp_sets ? o.n_msgs : 0u, o.memo ? o.m_hash : HASH_ALL);
  L = ws_layout(bp);
  tb::stat_add(tb::TB_STAT_PARTIALS);
  HIPCHK(ws_acquire(c, s));
  if (L.total > c.ws.cap) {  // growing frees the old buffer: drain its users first
    HIPCHK(hipStreamSynchronize(s));
    if (c.ws.ensure(L.total)) return TBLS_DEVICE_ERROR;
  }
  if (bp.key == key_kind::decompress)
    if (const int rc = pk_lookup_reserve(c, bp.n_keys, s)) return rc;
  const ws_ptrs W(L, c.ws.as<uint8_t>());
  const key_src keys = o.key_idx ? table_keys(c, o.key_idx) : own_keys(W.pk_aff, W.pk_code);
  // `serial` (tbls_dev_batch_stage_profile): every stage on the caller's
  // stream, for exclusive per-stage timings.  Otherwise the three per-set
  // chains (keys, signatures + bucket sums, hash) run side by side on their
  // streams at every batch size.  (Rounds 2-3 ran large batches' per-set
  // stages in sequence on the caller's stream, 52.5 vs 53.3 ms per 131k step
  // then; with round 4's kernels side by side wins everywhere: 16,384-set
  // partial unchanged, 32,768 sets 14.16 -> 12.44 ms, 65,536 26.11 -> 22.23,
  // 131,072 37.73 -> 36.15, profiles/r04_stage_chain_ab.json.)
  const bool late_join = bp.late_join && !o.serial;
  // Whether byte keys are looked up is decided here, at launch, inside the
  // plan's decompress branch.  The lookup (k_pk_lookup, tens of microseconds)
  // is queued on the caller's stream ahead of the fork, and the key stream
  // starts at the decompression of the misses, as it starts at the
  // decompression of all keys without a table.  Queued as the first kernel of
  // the key stream instead, a 16,384-set batch through tbls_batch_verify took
  // 10.5 ms with every key in the table and 12.2 ms with none, against 8.9 ms
  // without a table, although no stage's own time grew; ahead of the fork: 8.9,
  // 9.0, 8.8.  `serial` keeps the lookup inside the key stage's
  // bracket, for the exclusive stage times.
  const bool pre_lookup = bp.key == key_kind::decompress && bp.n_keys && pk_lookup_on(c) && !o.serial;
  const partial_run run{c, b, o, bp, W, keys, s, o.serial ? s : c.aux[0], o.serial ? s : c.aux[1], o.serial ? s : c.aux[2], late_join, pre_lookup};
  // byte keys that are looked up, and the last key stage found (nearly) all of its own: no decompression to speak of in this batch
  const bool keys_known = bp.key == key_kind::decompress && bp.n_keys && pk_keys_known(c);
  HIPCHK(hipMemsetAsync(W.set_code, 0, L.code_bytes, s));  // set_code and sig_code (adjacent; a grouped plan's pair codes after them)
  HIPCHK(hipMemsetAsync(W.n_bad, 0, 4, s));
  if (run.pre_lookup) {
    if (o.ev) HIPCHK(hipEventRecord(o.ev[0], s));  // stage 0 starts here
    if (const int rc = launch_pk_lookup(c, s, b.pks, bp.n_keys, W.pk_aff, W.pk_code)) return rc;
  }
  if (!o.serial) {
    HIPCHK(hipEventRecord(c.e_fork, s));
    HIPCHK(hipStreamWaitEvent(run.sa, c.e_fork, 0));
    HIPCHK(hipStreamWaitEvent(run.sb, c.e_fork, 0));
    HIPCHK(hipStreamWaitEvent(run.sh, c.e_fork, 0));
  }
  if (const int rc = run.sig_chain()) return rc;
  HIPCHK(hipEventRecord(c.e_join[1], run.sb));
  if (const int rc = run.key_chain()) return rc;
  HIPCHK(hipEventRecord(c.e_join[0], run.sa));
  // The cache learns behind the join: nothing in this batch reads what
  // k_pk_learn writes, and a kernel of the key stream that is dispatched once
  // the hash and signature kernels hold the chip ends only when a round of
  // their waves has retired, however little it does.  Ahead of k_set_pk it
  // held back the join: a 16,384-set tbls_batch_verify_each took 10.4 ms with
  // every key cached and 11.0 ms with none, against 9.4-9.5 ms without a cache
  // (DESIGN.md 3l).  The caller's stream waits for e_learn before ws_release,
  // as for every stream: the kernel reads the workspace.  With comb rows
  //  the kernel here is k_pk_learn_comb, which also builds the
  // published rows' comb entries and sets their ready bytes ahead of e_learn:
  // nothing in this batch reads a comb row it builds (k_set_pk_comb_w2 goes by
  // the references this batch's lookup wrote before), and the lookups of
  // later launches start behind ws_acquire, so behind e_learn and the entries.
  const bool learns = bp.key == key_kind::decompress && bp.n_keys && c.pkc_rows;
  if (learns) {
    launch_pk_learn(c, run.sa, b.pks, bp.n_keys, W.pk_aff, W.pk_code);
    if (!o.serial) HIPCHK(hipEventRecord(c.e_learn, run.sa));
  }
  // Bucket-sum batches with the key table: the hash waits for the signature
  // checks (sig_first).  Every large per-set kernel is one round of
  // register-full waves, so whichever starts first holds the whole chip until
  // it ends: with the hash first, the signature checks and the bucket-sum
  // chain behind them ran after it, and the bit-sum pairs' 64 wave Miller
  // loops ended up after the line kernel, where the accumulator waited
  // ~1.4 ms for them with the chip nearly idle (rocprof trace of the 131k
  // step, profiles/r05_kernel_trace_step.txt).  With key decompression in
  // the batch the hash-first order still measured faster -- so byte keys take
  // the table's order only when the device is expected to know them
  // (keys_known): 131k step with every key in the learned cache 32.69-32.93 ms
  // hash first, 32.08-32.37 ms signature checks first
  // (profiles/pk_learn.json).
  if (late_join && (bp.sig_first || keys_known)) HIPCHK(hipStreamWaitEvent(run.sh, c.e_sig, 0));
  if (const int rc = run.hash_chain()) return rc;
  if (!o.serial) {
    HIPCHK(hipEventRecord(c.e_join[2], run.sh));
    HIPCHK(hipStreamWaitEvent(s, c.e_join[2], 0));
  }
  // The memo's rows learn behind the join, as the key cache does and for the
  // same reason: nothing in this batch reads what k_memo_learn writes.  The
  // caller's stream waits for e_mlearn before ws_release, so the rows of this
  // batch are complete before the next batch's k_memo_fill (which starts
  // behind ws_acquire), and a flush in the next batch -- whose learn kernel
  // overwrites rows -- cannot overtake this batch's fill.
  const bool mlearns = bp.memo && bp.n_hash;
  if (mlearns) {
    run.memo_learn();
    if (!o.serial) HIPCHK(hipEventRecord(c.e_mlearn, run.sh));
  }
  HIPCHK(hipStreamWaitEvent(s, c.e_join[0], 0));
  if (!late_join)
    HIPCHK(hipStreamWaitEvent(s, c.e_join[1], 0));
  else
    HIPCHK(hipStreamWaitEvent(s, c.e_sig, 0));  // the set pairs' lines read the signature codes; miller() waits for the rest
  if (const int rc = run.miller()) return rc;
  if (late_join) HIPCHK(hipStreamWaitEvent(s, c.e_join[1], 0));  // every stream joins before ws_release
  if (o.settle) {
    if (learns && !o.serial) HIPCHK(hipStreamWaitEvent(s, c.e_learn, 0));
    if (mlearns && !o.serial) HIPCHK(hipStreamWaitEvent(s, c.e_mlearn, 0));
    HIPCHK(hipGetLastError());
    HIPCHK(ws_release(c, s));
    return TBLS_SUCCESS;
  }
  TB_EV(11, s);
  if (const int rc = run.product_tree(partial_out)) return rc;
  HIPCHK(hipMemcpyAsync((uint8_t*)partial_out + sizeof(fp12), W.n_bad, 4, hipMemcpyDeviceToDevice, s));
  if (learns && !o.serial) HIPCHK(hipStreamWaitEvent(s, c.e_learn, 0));
  if (mlearns && !o.serial) HIPCHK(hipStreamWaitEvent(s, c.e_mlearn, 0));
  HIPCHK(hipGetLastError());
  HIPCHK(ws_release(c, s));
  return TBLS_SUCCESS;
}
#undef TB_EV

// final: product of g partial records -> final exponentiation, straight from
// the records (k_final_verify_recs reads them in place; the only device state
// it writes is the verdict word)
int launch_final(dev_ctx& c, const void* recs, uint32_t g, hipStream_t s, int* result_host) {
  if (c.fin.ensure(256)) return TBLS_DEVICE_ERROR;
  int* res = c.fin.as<int>();
  tb::stat_add(tb::TB_STAT_FINALS);
  tb_launch_final_recs((const uint8_t*)recs, g, s, res);
  HIPCHK(hipGetLastError());
  if (c.hout.ensure(16)) return TBLS_DEVICE_ERROR;
  HIPCHK(hipMemcpyAsync(c.hout.p, res, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *result_host = *(int*)c.hout.p;
  return TBLS_SUCCESS;
}

int ensure_init() {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_inited) return g_ctx.empty() ? TBLS_DEVICE_ERROR : TBLS_SUCCESS;
  return TBLS_DEVICE_ERROR;
}

dev_ctx* ctx_for(int d) {
  if (d < 0 || d >= (int)g_ctx.size()) return nullptr;
  return g_ctx[d];
}

// The keys of sets[lo, hi) against device c's state, under its lock (a reload
// cannot interleave): table indices below the table's size; bit rows over a
// loaded committee of the size the caller saw.
template <class SET>
int check_keys(const dev_ctx* c, const SET* sets, size_t lo, size_t hi) {
  if constexpr (std::is_same<SET, tbls_set_idx>::value) {
    if (!c->tab_n) return TBLS_BAD_ARGUMENT;
    for (size_t i = lo; i < hi; i++)
      for (uint32_t k = 0; k < sets[i].n_pks; k++)
        if (sets[i].key_idx[k] >= c->tab_n) return TBLS_BAD_ARGUMENT;
  } else if constexpr (std::is_same<SET, set_bits_i>::value) {
    if (!c->tab_n) return TBLS_BAD_ARGUMENT;
    for (size_t i = lo; i < hi; i++)
      if (sets[i].slot >= TBLS_COMMITTEE_SLOTS || sets[i].slot != sets[lo].slot || !sets[i].size ||
          sets[i].size != c->cm_size[sets[i].slot] || sets[i].n_pks != bits_stride_w(sets[i].size))
        return TBLS_BAD_ARGUMENT;
  }
  return TBLS_SUCCESS;
}

const uint8_t ETH2_DST[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";

// How shard_launch runs a shard.  gm: the grouped entries group the shard's
// own sets by message (tb_group.h) and launch the grouped plan when it pays
// (tb_plan.h group_pays), with GROUP_FORCE whenever a message repeats; a
// message that straddles a shard cut simply appears in both shards.
enum group_mode { GROUP_OFF, GROUP_AUTO, GROUP_FORCE };
inline group_mode group_mode_of(uint32_t flags) { return (flags & TBLS_GROUP_FORCE) ? GROUP_FORCE : GROUP_AUTO; }
struct shard_opts {
  const uint8_t* dst = ETH2_DST;  // hash_to_G2 domain separation tag, host memory
  uint32_t dlen = 43;
  bool settle = false;  // the settle layout (partial_opts::settle): no partial record
  group_mode gm = GROUP_OFF;
  // The batch entries (their DST is ETH2_DST, which the memo is keyed for):
  // resolve the shard's messages against the device's hash-point memo when it
  // is on.  Calls with a DST of their own leave it false.
  bool memo = false;
};

// The memo's rows on c for a shard about to resolve (lock held): allocated on
// first use; true when the device has a memo.  A device where the allocation
// fails goes on without one (memo.rows = 0), as with the key cache.
bool memo_reserve(dev_ctx& c) {
  if (!c.memo.rows) return false;
  if (c.memo_rows.p) return true;
  if (c.memo_rows.ensure(memo_skip_off(c.memo.rows) + c.memo.rows, true)) {
    (void)hipGetLastError();
    c.memo.configure(0);
    return false;
  }
  return true;
}
// What shard_launch leaves behind: the workspace layout of the pipeline that
// ran, the partial record (device memory, the shard's c->in) and the sets
// staged; when the grouped plan ran, its messages and the byte offsets of the
// CSR (tb_group.h grp_off, grp_sets) and of the randomizers in the staging
// image (c->in, and c->hin on the host side), for settle_grouped.
struct shard_run {
  ws_layout L;
  uint8_t* dpart = nullptr;
  uint32_t n = 0;
  uint32_t n_msgs = 0;  // 0: the shard ran ungrouped
  size_t in_grpoff = 0, in_grpsets = 0, in_rand = 0;
};

// Stage sets[lo, hi) on device c (its lock held) and queue the partial
// pipeline on c->stream, filling R: the 580-byte partial record lands at
// R.dpart -- nothing is synchronized.  e_t0/e_t1 bracket the kernels.
// With so.memo on a device that has a memo, the shard's messages are first
// resolved against its index (tb_msgmemo.h): the image then carries only the
// messages left to hash, with src, learn and -- for an ungrouped pass --
// set_grp in regions after the usual ones.
template <class SET>
int shard_launch_resolved(dev_ctx* c, const SET* sets, size_t lo, size_t hi, const uint64_t* rand, const shard_opts& so, shard_run& R,
                          bool& resolved);
// A shard that resolved and then failed invalidates the index: the rows it
// promised may never have been written.
template <class SET>
int shard_launch(dev_ctx* c, const SET* sets, size_t lo, size_t hi, const uint64_t* rand, const shard_opts& so, shard_run& R) {
  bool resolved = false;
  const int rc = shard_launch_resolved(c, sets, lo, hi, rand, so, R, resolved);
  if (rc && resolved) c->memo.invalidate();
  return rc;
}
template <class SET>
int shard_launch_resolved(dev_ctx* c, const SET* sets, size_t lo, size_t hi, const uint64_t* rand, const shard_opts& so, shard_run& R,
                          bool& resolved) {
  constexpr bool idx_mode = !std::is_same<SET, tbls_set>::value;  // keys from the table: indices, or committee bit rows
  constexpr bool bits_mode = std::is_same<SET, set_bits_i>::value;
  R = shard_run();
  HIPCHK(hipSetDevice(c->dev));
  if (const int rc = check_keys(c, sets, lo, hi)) return rc;
  bits_src cm{};
  if constexpr (bits_mode)
    if (hi > lo) cm = committee_src(*c, sets[lo].slot);
  groups G;
  bool grouped = false;
  const bool group_try = so.gm != GROUP_OFF && !so.settle && !bits_mode;
  const bool use_memo = so.memo && hi > lo && hi - lo <= TB_MEMO_SETS_MAX && memo_reserve(*c);
  if (group_try || use_memo) G = group_messages(sets, lo, hi);
  if (group_try) grouped = group_pays((uint32_t)(hi - lo), G.m, so.gm == GROUP_FORCE);
  tb::memo::resolved MR;
  if (use_memo) {
    MR = c->memo.resolve(G, !grouped);
    resolved = true;
  }
  tb::memo::packed_memo p;
  if (grouped)
    static_cast<packed_grouped&>(p) = pack_layout_grouped(sets, lo, hi, so.dlen, G);
  else
    static_cast<packed&>(p) = pack_layout(sets, lo, hi, so.dlen);
  if (use_memo) p = tb::memo::pack_layout_memo(p, grouped, G, MR);
  const size_t in_total = p.total + TBLS_PARTIAL_BYTES + 256;
  hipStream_t s = c->stream;
  if (in_total > c->in.cap || in_total > c->hin.cap) HIPCHK(hipStreamSynchronize(s));  // buffers may still be read
  if (c->hin.ensure(in_total) || c->in.ensure(in_total)) return TBLS_DEVICE_ERROR;
  if (grouped)
    pack_fill_grouped(c->hin.as<uint8_t>(), p, sets, lo, rand, so.dst, so.dlen, G);
  else
    pack_fill(c->hin.as<uint8_t>(), p, sets, lo, rand, so.dst, so.dlen);
  if (use_memo) tb::memo::pack_fill_memo(c->hin.as<uint8_t>(), p, G, MR);
  HIPCHK(hipMemcpyAsync(c->in.p, c->hin.p, p.total, hipMemcpyHostToDevice, s));
  uint8_t* di = c->in.as<uint8_t>();
  tbls_dev_batch b;
  b.pks = di + p.off_pks;
  b.pk_off = (const uint32_t*)(di + p.off_pkoff);
  b.n_keys = p.K;
  b.msgs = di + p.off_msgs;
  b.msg_off = (const uint32_t*)(di + p.off_msgoff);
  b.sigs = di + p.off_sigs;
  b.rand = (const uint64_t*)(di + p.off_rand);
  b.n = p.n;
  R.dpart = di + align_up(p.total);
  R.n = p.n;
  HIPCHK(hipEventRecord(c->e_t0, s));
  partial_opts o{di + p.off_dst, so.dlen};
  o.key_idx = idx_mode ? (const uint32_t*)(di + p.off_pks) : nullptr;
  o.settle = so.settle;
  o.cm = bits_mode ? &cm : nullptr;
  if (grouped) {
    o.n_msgs = p.m;
    o.grp_off = (const uint32_t*)(di + p.off_grpoff);
    o.grp_sets = (const uint32_t*)(di + p.off_grpsets);
    R.n_msgs = p.m;
    R.in_grpoff = p.off_grpoff;
    R.in_grpsets = p.off_grpsets;
    R.in_rand = p.off_rand;
  }
  if (use_memo) {
    b.msgs = di + p.off_hmsgs;
    b.msg_off = (const uint32_t*)(di + p.off_hmsgoff);
    o.memo = true;
    o.m_hash = p.m_hash;
    o.memo_src = (const uint32_t*)(di + p.off_src);
    o.memo_learn = (const uint32_t*)(di + p.off_learn);
    o.memo_setgrp = grouped ? nullptr : (const uint32_t*)(di + p.off_setgrp);
  }
  if (const int rc = launch_partial(*c, b, s, R.dpart, R.L, o)) return rc;
  HIPCHK(hipEventRecord(c->e_t1, s));
  return TBLS_SUCCESS;
}

// Per-set verdict codes of the shard that R records (set_code | sig_code; signature
// errors first: decode failures surface as BlsException), after the stream is idle.
int shard_codes(dev_ctx* c, const shard_run& R, uint8_t* codes_host) {
  const uint32_t n = R.n;
  if (!n) return TBLS_SUCCESS;
  if (c->hout.ensure(2 * (size_t)n)) return TBLS_DEVICE_ERROR;
  const ws_ptrs W(R.L, c->ws.as<uint8_t>());
  HIPCHK(hipMemcpyAsync(c->hout.p, W.set_code, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(c->hout.as<uint8_t>() + n, W.sig_code, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t a = c->hout.as<uint8_t>()[i], bb = c->hout.as<uint8_t>()[n + i];
    codes_host[i] = bb ? bb : a;
  }
  return TBLS_SUCCESS;
}

// One device: shard -> final exponentiation straight from the device-resident
// partial record (no host round trip), for the calls with a DST of their own
// or per-set codes (codes_host, nullable); batches go through batch_pass.
int verify_on_device(int d, const tbls_set* sets, size_t n, const uint64_t* rand, const uint8_t* dst, uint32_t dlen, int* ok,
                     uint8_t* codes_host) {
  dev_ctx* c = ctx_for(d);
  if (!c) return TBLS_DEVICE_ERROR;
  std::lock_guard<std::mutex> lk(c->mu);
  const shard_opts so{dst, dlen};
  shard_run R;
  int rc = shard_launch(c, sets, 0, n, rand, so, R);
  if (rc) return rc;
  rc = launch_final(*c, R.dpart, 1, c->stream, ok);  // synchronizes c->stream
  if (rc) return rc;
  return codes_host ? shard_codes(c, R, codes_host) : TBLS_SUCCESS;
}

// ---------------------------------------------------------------------------
// Per-set verdicts of a failed batch from the batch's own work (SURVEY.md
// 8(f) rank 2).  The reference settles a failed batch by recursive halving,
// one full batchVerify per half (AggregatingSignatureVerificationService.java:
// 206-233); round 4 ran every set again from its bytes with its own final
// exponentiation (tbls_verify_each: 75 ms for a failed 16,384-set batch whose
// batch pass takes 9.8).  Here, on the device that ran the batch and with its
// workspace intact:
//  * per-set Miller values from the batch's own G2 lines: the segmented
//    accumulator with two pairs per thread, where thread g owns pairs g and
//    g + n -- set g's (r apk, H(m)) and (-r g1, sig) -- so each thread's
//    value is that set's randomized Miller value, in nseg segments;
//  * two levels of wave products (16 sets per group, then 256), the same
//    kernels as the batch's product tree;
//  * group tests, top level first: one coop workgroup per group runs the
//    segments' Horner combine and the final exponentiation
//    (k_group_test_coop); a group whose product is 1 holds only valid sets
//    (its sets' randomizers make a false pass as unlikely as the batch's own,
//    2^-64 per forged set); failing groups are opened one level down, to
//    single sets, whose test is exact.  A set with a failed decode / group /
//    key check is invalid from its per-set code alone.
// Batches that ran the bucket-sum signature side (>= 20,480 sets) or the
// wave Miller loops (<= 2,048 pairs, a set's two pairs among them: 1,024
// sets) have no per-set signature pairs or no lines (tb_plan.h
// settle_ready): their sets are re-staged in chunks of TB_SETTLE_MAX in the
// settle layout (pair_plan settle: one signature pair per set, split
// kernels), which runs the per-set stages and the line kernel only.
// ---------------------------------------------------------------------------
// Group tests of the listed groups (at least one) of a segmented value array
// on c's stream: pass[k] = 1 iff group list[k] tests 1.
static int group_tests(dev_ctx* c, const fp12* vals, uint32_t stride, uint32_t nseg, const std::vector<uint32_t>& list, uint32_t* dlist,
                       uint8_t* dout, std::vector<uint8_t>& pass) {
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(dlist, list.data(), 4 * list.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_group_test_coop, dim3((uint32_t)list.size()), dim3(TB_CFE_THREADS), 0, s, vals, stride, nseg, (const uint32_t*)dlist, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(pass.data(), dout, list.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TBLS_SUCCESS;
}

// The tail of a settle, from the S.n per-set Miller values at S.V of c->sws
// (nseg segment rows, queued on c's stream): two levels of wave products
// (TB_SETTLE_FAN values per group, then groups of groups) into A and B, then
// the group tests top-down to single sets (tb_settle.h settle_descent).
// codes[i] != 0: value i's set is invalid by its code alone.
static int settle_tail(dev_ctx* c, const settle_layout& S, const std::vector<uint8_t>& codes, uint8_t* ok) {
  const uint32_t F = TB_SETTLE_FAN, n = S.n, nseg = S.nseg, nA = S.nA, nB = S.nB;
  fp12 *V = c->sws.as<fp12>(S.V), *A = c->sws.as<fp12>(S.A), *B = c->sws.as<fp12>(S.B);
  uint32_t* dlist = c->sws.as<uint32_t>(S.list);
  uint8_t* dout = c->sws.as<uint8_t>(S.out);
  hipStream_t s = c->stream;
  hipLaunchKernelGGL(k_fp12_prod_wave_seg, dim3(nA, nseg), dim3(64), 0, s, (const fp12*)V, n, n, nseg, n, F, A, nA);
  hipLaunchKernelGGL(k_fp12_prod_wave_seg, dim3(nB, nseg), dim3(64), 0, s, (const fp12*)A, nA, nA, nseg, nA, F, B, nB);
  HIPCHK(hipGetLastError());
  return settle_descent(S, codes, ok, [&](settle_level level, const std::vector<uint32_t>& list, std::vector<uint8_t>& pass) {
    return level == SETTLE_B   ? group_tests(c, B, nB, nseg, list, dlist, dout, pass)
           : level == SETTLE_A ? group_tests(c, A, nA, nseg, list, dlist, dout, pass)
                               : group_tests(c, V, n, nseg, list, dlist, dout, pass);
  });
}

// ok[0..R.n) for the sets whose pipeline (normal and settle_ready, or the
// settle layout) just ran on c as R records; lock held, workspace R.L intact.
static int settle_sets(dev_ctx* c, const shard_run& R, uint8_t* ok) {
  const uint32_t n = R.n;
  if (!n) return TBLS_SUCCESS;
  tb::stat_add(tb::TB_STAT_SETTLE);
  std::vector<uint8_t> codes(n);
  int rc = shard_codes(c, R, codes.data());  // synchronizes the stream
  if (rc) return rc;
  const settle_layout S(n);
  if (c->sws.ensure(S.total)) return TBLS_DEVICE_ERROR;
  const ws_ptrs W(R.L, c->ws.as<uint8_t>());
  hipStream_t s = c->stream;
  const uint32_t g_pad = (n + TB_BLOCK - 1) / TB_BLOCK * TB_BLOCK;
  hipLaunchKernelGGL(k_settle_mask, dim3((n + 255) / 256), dim3(256), 0, s, (const uint8_t*)W.set_code, n, W.skip);
  hipLaunchKernelGGL(k_miller_accs_lds, dim3(S.nseg * g_pad / TB_BLOCK), dim3(TB_BLOCK), 0, s, (const uint4*)W.lines, (const uint8_t*)W.skip,
                     (const uint8_t*)W.set_code, (const uint8_t*)W.sig_code, 2u * n, 2u, S.nseg, g_pad, c->sws.as<fp12>(S.V), n);
  return settle_tail(c, S, codes, ok);
}

// ok[0..R.n) for the sets whose GROUPED pipeline just ran on c as R records
// (R.n_msgs messages; lock held, stream idle, workspace R.L and the staging
// image in c->in / c->hin intact).  The grouped pass leaves no per-set Miller lines --
// one pair per message, the signature side as bucket sums -- but everything a
// per-set value needs: set_P, the codes, sig_aff / sig_use, the messages' hash
// points and the CSR.  So nothing is staged, decoded or hashed again
// (k_gsettle.hip): the messages' line tables once, then per chunk of
// gsettle_layout positions the signature pairs' lines (the line kernel a
// batch of that many pairs takes) and the accumulator into V; then
// settle_sets's tail over positions, and position t's verdict is set
// grp_sets[t]'s.
static int settle_grouped(dev_ctx* c, const shard_run& R, uint8_t* ok) {
  const uint32_t n = R.n, m = R.n_msgs;
  if (!n) return TBLS_SUCCESS;
  if (!m || m >= n) return TBLS_BAD_ARGUMENT;
  tb::stat_add(tb::TB_STAT_SETTLE);
  std::vector<uint8_t> codes(n);
  int rc = shard_codes(c, R, codes.data());  // per set; synchronizes the stream
  if (rc) return rc;
  const plan_env& env = plan_env::get();
  const gsettle_layout S(n, m, env);
  if (c->sws.ensure(S.total)) return TBLS_DEVICE_ERROR;
  const ws_ptrs W(R.L, c->ws.as<uint8_t>());
  const uint8_t* di = c->in.as<uint8_t>();
  const uint32_t *grp_off = (const uint32_t*)(di + R.in_grpoff), *grp_sets = (const uint32_t*)(di + R.in_grpsets);
  const uint32_t* pos_set = c->hin.as<uint32_t>(R.in_grpsets);  // the same CSR, host side
  const uint64_t* rand = (const uint64_t*)(di + R.in_rand);
  const g1a* set_P = W.set_P;
  const g2a *Q = W.Q, *sig_aff = W.sig_aff;
  const uint8_t *msg_skip = W.skip, *set_code = W.set_code, *sig_code = W.sig_code, *sig_use = W.sig_use;
  uint4 *mlines = c->sws.as<uint4>(S.mlines), *slines = c->sws.as<uint4>(S.slines);
  uint32_t* msg_of_pos = c->sws.as<uint32_t>(S.msg_of_pos);
  g1a* negr = c->sws.as<g1a>(S.negr);
  g2a* sigq = c->sws.as<g2a>(S.sigq);
  uint8_t* sskip = c->sws.as<uint8_t>(S.sskip);
  fp12* V = c->sws.as<fp12>(S.tail.V);
  const uint32_t nseg = S.tail.nseg;
  hipStream_t s = c->stream;
  const dim3 blk(TB_BLOCK);
  hipLaunchKernelGGL(k_gsettle_msg_lines, dim3((m + TB_BLOCK - 1) / TB_BLOCK), blk, 0, s, Q, msg_skip, m, mlines);
  for (uint32_t k = 0; k < S.n_chunks; k++) {
    const uint32_t lo = S.lo(k), cn = S.hi(k) - lo;
    const uint32_t g_pad = (cn + TB_BLOCK - 1) / TB_BLOCK * TB_BLOCK;
    const int lg = line_group(cn, env);
    hipLaunchKernelGGL(k_gsettle_prep, dim3(g_pad / TB_BLOCK), blk, 0, s, grp_off, grp_sets, m, n, lo, cn, rand, c->comb.as<const g1a>(), sig_aff,
                       sig_use, set_code, sig_code, msg_skip, msg_of_pos, negr, sigq, sskip);
    // the skip flag carries the codes: the same row for all three
    hipLaunchKernelGGL(line_kernel_of(lg), dim3((lg * cn + TB_BLOCK - 1) / TB_BLOCK), blk, 0, s, (const g1a*)negr, (const g2a*)sigq,
                       (const uint8_t*)sskip, (const uint8_t*)sskip, (const uint8_t*)sskip, cn, slines);
    hipLaunchKernelGGL(k_miller_accs_gsettle, dim3(nseg * g_pad / TB_BLOCK), blk, 0, s, (const uint4*)mlines, m, (const uint32_t*)msg_of_pos,
                       grp_sets, set_P, set_code, sig_code, msg_skip, (const uint4*)slines, (const uint8_t*)sskip, lo, cn, n, nseg, g_pad, V);
  }
  HIPCHK(hipGetLastError());
  std::vector<uint8_t> pos_code(n), pos_ok(n, 0);
  for (uint32_t t = 0; t < n; t++) {
    if (pos_set[t] >= n) return TBLS_DEVICE_ERROR;
    pos_code[t] = codes[pos_set[t]];
  }
  rc = settle_tail(c, S.tail, pos_code, pos_ok.data());
  if (rc) return rc;
  for (uint32_t t = 0; t < n; t++) ok[pos_set[t]] = pos_ok[t];
  return TBLS_SUCCESS;
}

// settle sets [lo, hi) of `sets` on c (lock held) after their batch failed
// (ran: the record of the batch's shard over exactly these sets): from the
// batch's workspace when it is settle_ready, else re-staged in the settle
// layout chunk by chunk
template <class SET>
static int settle_range(dev_ctx* c, const SET* sets, size_t lo, size_t hi, const uint64_t* rand, const shard_run& ran, uint8_t* ok) {
  if (settle_ready(ran.n)) return settle_sets(c, ran, ok);
  shard_opts so;
  so.settle = true;
  so.memo = true;  // the second staging of a failed batch finds its messages resident
  for (size_t a = lo; a < hi; a += TB_SETTLE_MAX) {
    const size_t b = std::min(hi, a + (size_t)TB_SETTLE_MAX);
    shard_run R;
    int rc = shard_launch(c, sets, a, b, rand, so, R);
    if (!rc) rc = settle_sets(c, R, ok + (a - lo));
    if (rc) return rc;
  }
  return TBLS_SUCCESS;
}

// ---------------------------------------------------------------------------
// Multi-GPU gather of the partial records: one 580-byte record
// per device to device 0, then one final exponentiation there.
//  * rccl (default): ncclGather over a single-process communicator
//    (ncclCommInitAll over the library's devices, created on first use),
//    every device's call inside one ncclGroupStart/End, on its own stream --
//    the records move over xGMI;
//  * peer: hipMemcpyPeerAsync of each record into device 0's buffer;
//  * host: each record through pinned host memory (no peer access needed).
// All three give the same bytes in device 0's buffer (TBLS_GATHER selects).
// ---------------------------------------------------------------------------
enum gather_mode { GATHER_RCCL, GATHER_PEER, GATHER_HOST };
gather_mode gather_sel() {
  const char* v = getenv("TBLS_GATHER");
  if (v && !strcmp(v, "peer")) return GATHER_PEER;
  if (v && !strcmp(v, "host")) return GATHER_HOST;
  return GATHER_RCCL;
}
bool gather_forced() { return getenv("TBLS_GATHER") != nullptr; }  // also for one device (tests)

struct rccl_api {
  bool tried = false, ok = false;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGather) Gather = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  // One single-process communicator per participating device set (a bit
  // mask over the library's devices): a batch placed on G of the initialised
  // devices gathers on a G-rank communicator over exactly those, so no rank
  // of the collective is left waiting.
  std::map<uint32_t, std::vector<ncclComm_t>> comms;
};
rccl_api g_rccl;

// RCCL resolved at run time (an already-loaded librccl.so.1 -- e.g. torch's --
// is reused by its soname); g_mu held.
bool rccl_load_locked() {
  if (g_rccl.tried) return g_rccl.ok;
  g_rccl.tried = true;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return false;
  g_rccl.CommInitAll = (decltype(g_rccl.CommInitAll))dlsym(h, "ncclCommInitAll");
  g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
  g_rccl.Gather = (decltype(g_rccl.Gather))dlsym(h, "ncclGather");
  g_rccl.GroupStart = (decltype(g_rccl.GroupStart))dlsym(h, "ncclGroupStart");
  g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))dlsym(h, "ncclGroupEnd");
  g_rccl.ok = g_rccl.CommInitAll && g_rccl.CommDestroy && g_rccl.Gather && g_rccl.GroupStart && g_rccl.GroupEnd;
  return g_rccl.ok;
}

// The communicator over devices devs[0..G) (created on first use); nullptr
// if RCCL is absent.
const std::vector<ncclComm_t>* rccl_comms_locked(const std::vector<int>& devs, int G) {
  if (!rccl_load_locked() || G < 1 || G > (int)g_ctx.size()) return nullptr;
  uint32_t mask = 0;
  for (int k = 0; k < G; k++) mask |= 1u << devs[k];
  auto it = g_rccl.comms.find(mask);
  if (it != g_rccl.comms.end()) return &it->second;
  std::vector<int> hw;
  for (int k = 0; k < G; k++) hw.push_back(g_ctx[devs[k]]->dev);
  std::vector<ncclComm_t> cm(G, nullptr);
  if (g_rccl.CommInitAll(cm.data(), G, hw.data()) != ncclSuccess) return nullptr;
  return &(g_rccl.comms[mask] = cm);
}

// Device records runs[k].dpart (on device devs[k]'s stream, k < G) -> the root's
// recs buffer (root = devs[0]).  Leaves the calling thread on the root device
// (the caller's caller_device restores).
int gather_partials(gather_mode mode, const std::vector<int>& devs, int G, const std::vector<shard_run>& runs) {
  dev_ctx* c0 = ctx_for(devs[0]);
  if (mode == GATHER_RCCL) {  // an RCCL communicator needs G distinct hardware devices (TBLS_INIT_SHARE_DEVICES)
    uint64_t seen = 0;
    for (int g = 0; g < G; g++) {
      const int d = ctx_for(devs[g])->dev;
      if (d < 64 && ((seen >> d) & 1)) mode = GATHER_PEER;
      if (d < 64) seen |= 1ull << d;
    }
  }
  HIPCHK(hipSetDevice(c0->dev));
  if (c0->recs.ensure((size_t)G * TBLS_PARTIAL_BYTES)) return TBLS_DEVICE_ERROR;
  uint8_t* recv = c0->recs.as<uint8_t>();
  if (mode == GATHER_RCCL) {
    const std::vector<ncclComm_t>* cm = nullptr;
    {
      std::lock_guard<std::mutex> lk(g_mu);
      cm = rccl_comms_locked(devs, G);
    }
    // ncclGather writes comm_size * 580 bytes at the root: recv holds G records
    if (!cm || (int)cm->size() != G) return TBLS_DEVICE_ERROR;
    for (int g = 0; g < G; g++) HIPCHK(hipSetDevice(ctx_for(devs[g])->dev));  // every device reachable before the group opens
    if (g_rccl.GroupStart() != ncclSuccess) return TBLS_DEVICE_ERROR;
    int bad = 0;
    for (int g = 0; g < G; g++) {
      dev_ctx* c = ctx_for(devs[g]);
      if (hipSetDevice(c->dev) != hipSuccess) {  // every rank must still join: the group ends below
        bad = 1;
        continue;
      }
      bad |= g_rccl.Gather(runs[g].dpart, g == 0 ? recv : nullptr, TBLS_PARTIAL_BYTES, ncclUint8, 0, (*cm)[g], c->stream) != ncclSuccess;
    }
    bad |= g_rccl.GroupEnd() != ncclSuccess;
    if (bad) return TBLS_DEVICE_ERROR;
    // the root's stream holds the gather; the others' sends complete on theirs
    for (int g = 1; g < G; g++) {
      dev_ctx* c = ctx_for(devs[g]);
      HIPCHK(hipSetDevice(c->dev));
      HIPCHK(hipEventRecord(c->e_join[0], c->stream));
      HIPCHK(hipSetDevice(c0->dev));
      HIPCHK(hipStreamWaitEvent(c0->stream, c->e_join[0], 0));
    }
    HIPCHK(hipSetDevice(c0->dev));
    return TBLS_SUCCESS;
  }
  if (mode == GATHER_PEER) {
    for (int g = 0; g < G; g++) {
      dev_ctx* c = ctx_for(devs[g]);
      HIPCHK(hipSetDevice(c->dev));
      HIPCHK(hipMemcpyPeerAsync(recv + (size_t)g * TBLS_PARTIAL_BYTES, c0->dev, runs[g].dpart, c->dev, TBLS_PARTIAL_BYTES, c->stream));
      if (g) {
        HIPCHK(hipEventRecord(c->e_join[0], c->stream));
        HIPCHK(hipSetDevice(c0->dev));
        HIPCHK(hipStreamWaitEvent(c0->stream, c->e_join[0], 0));
      }
    }
    HIPCHK(hipSetDevice(c0->dev));
    return TBLS_SUCCESS;
  }
  std::vector<uint8_t> host((size_t)G * TBLS_PARTIAL_BYTES);
  for (int g = 0; g < G; g++) {
    dev_ctx* c = ctx_for(devs[g]);
    HIPCHK(hipSetDevice(c->dev));
    if (c->hout.ensure(TBLS_PARTIAL_BYTES)) return TBLS_DEVICE_ERROR;
    HIPCHK(hipMemcpyAsync(c->hout.p, runs[g].dpart, TBLS_PARTIAL_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(host.data() + (size_t)g * TBLS_PARTIAL_BYTES, c->hout.p, TBLS_PARTIAL_BYTES);
  }
  HIPCHK(hipSetDevice(c0->dev));
  HIPCHK(hipMemcpyAsync(recv, host.data(), host.size(), hipMemcpyHostToDevice, c0->stream));
  HIPCHK(hipStreamSynchronize(c0->stream));
  return TBLS_SUCCESS;
}

// generic single-kernel helpers: upload bytes, run, download
struct upload {
  std::vector<uint8_t> h;
  size_t add(const void* src, size_t n) {
    size_t o = align_up(h.size());
    h.resize(o + (n ? n : 1));
    if (n) memcpy(h.data() + o, src, n);
    return o;
  }
};

// fn(g) for each of G shards: on the calling thread when G == 1, else one host
// thread per shard (host-side packing and launch queueing in parallel)
template <class FN>
void for_each_shard(int G, const FN& fn) {
  if (G == 1) {
    fn(0);
    return;
  }
  std::vector<std::thread> th;
  for (int g = 0; g < G; g++) th.emplace_back(fn, g);
  for (auto& x : th) x.join();
}

// The randomized batch over sets[0, n) (n > 0, every set with keys), the one
// pass behind tbls_batch_verify* and tbls_batch_verify_each: place the batch
// (place_plan), lock the placed devices in ascending order, stage and launch
// each shard (one host thread per shard when there are several), gather the
// partial records on the lowest device unless the one record is final as it
// lies, and run the final exponentiation there.  The locks and the placement
// last as long as the pass, so a caller can settle from the shards'
// workspaces (runs) under them.
template <class SET>
struct batch_pass {
  placed pl;  // declared first: the batch counts on its devices until the locks are gone
  std::vector<std::unique_lock<std::mutex>> locks;
  std::vector<shard_run> runs;  // per shard, what its launch left behind
  double device_ms = 0;         // the shards' e_t0 .. e_t1, summed
  dev_ctx* ctx(int g) const { return ctx_for(pl.dev[g]); }

  int run(const SET* sets, size_t n, const uint64_t* rand, int n_gpus, int* ok, group_mode gm = GROUP_OFF) {
    place_batch(pl, n, [&](size_t i) { return sets[i].n_pks; }, n_gpus, shard_min(), shard_knee());
    const int G = pl.G;
    for (int g = 0; g < G; g++) locks.emplace_back(ctx(g)->mu);  // only the placed devices, ascending: no deadlock
    runs.resize(G);
    shard_opts so;
    so.gm = gm;
    so.memo = true;
    std::vector<int> rcs(G, 0);
    for_each_shard(G, [&](int g) { rcs[g] = shard_launch(ctx(g), sets, pl.cut[g], pl.cut[g + 1], rand, so, runs[g]); });
    for (int g = 0; g < G; g++)
      if (rcs[g]) return rcs[g];
    dev_ctx* root = ctx(0);
    const void* recs = runs[0].dpart;
    if (G > 1 || gather_forced()) {
      if (const int rc = gather_partials(gather_sel(), pl.dev, G, runs)) return rc;
      recs = root->recs.p;
    }
    if (const int rc = launch_final(*root, recs, (uint32_t)G, root->stream, ok)) return rc;  // synchronizes the root's stream
    // the pipelines' device times, read here: a settle re-records the events
    // (its re-staged chunks run shard_launch again).  The root is current and idle.
    for (int g = 0; g < G; g++) {
      dev_ctx* c = ctx(g);
      if (g) {
        (void)hipSetDevice(c->dev);
        (void)hipStreamSynchronize(c->stream);
      }
      float ms = 0;
      (void)hipEventElapsedTime(&ms, c->e_t0, c->e_t1);
      device_ms += ms;
    }
    return TBLS_SUCCESS;
  }

  // total_ms since t0; device_ms is the batch pass only
  void timing(tbls_timing* t, std::chrono::steady_clock::time_point t0) const {
    if (!t) return;
    t->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    t->device_ms = device_ms;
    t->n_devices = (uint32_t)pl.G;
  }
};

// The device-resident API's way in: fn(c, s) with device `device` locked and
// current, s the caller's stream (or the device's own) and the default DST
// in c.dstb (uploaded on first use).
template <class FN>
int with_dev_stream(int device, void* stream, const FN& fn) {
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  dev_ctx* c = ctx_for(device);
  if (!c) return TBLS_DEVICE_ERROR;
  std::lock_guard<std::mutex> lk(c->mu);
  const caller_device keep;
  HIPCHK(hipSetDevice(c->dev));
  if (!c->dstb.p) {
    if (c->dstb.ensure(256)) return TBLS_DEVICE_ERROR;
    HIPCHK(hipMemcpy(c->dstb.p, ETH2_DST, 43, hipMemcpyHostToDevice));
  }
  return fn(*c, stream ? (hipStream_t)stream : c->stream);
}

// one-call helpers run on the least-loaded device (place_one)
int with_device(const std::function<int(dev_ctx&)>& fn) {
  const caller_device keep;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  placed pl;
  place_one(pl);
  tb::stat_add(tb::TB_STAT_HELPERS);
  dev_ctx* c = ctx_for(pl.dev[0]);
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->dev));
  // ws may still be in use by device-API work queued on a caller's stream
  HIPCHK(ws_acquire(*c, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int rc = fn(*c);
  (void)ws_release(*c, c->stream);
  return rc;
}

// The table and committee calls' way in: fn(c) for each device of the library
// in turn, locked and current.  after_ws: c.stream is first ordered after the
// workspace's last user (device-API partials queued on a caller's stream may
// still read the table); drain: and synchronized.  Stops at the first error.
template <class FN>
int each_device(bool after_ws, bool drain, const FN& fn) {
  std::vector<dev_ctx*> devs;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    devs = g_ctx;
  }
  for (dev_ctx* c : devs) {
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->dev));
    if (after_ws) HIPCHK(ws_acquire(*c, c->stream));
    if (drain) HIPCHK(hipStreamSynchronize(c->stream));
    if (const int rc = fn(c)) return rc;
  }
  return TBLS_SUCCESS;
}

int stage_in(dev_ctx& c, const upload& u, uint8_t** d) {
  if (c.in.ensure(u.h.size() + 4096)) return TBLS_DEVICE_ERROR;
  HIPCHK(hipMemcpyAsync(c.in.p, u.h.data(), u.h.size(), hipMemcpyHostToDevice, c.stream));
  *d = c.in.as<uint8_t>();
  return TBLS_SUCCESS;
}

int fetch(dev_ctx& c, void* dst, const void* src, size_t n) {
  HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipStreamSynchronize(c.stream));
  HIPCHK(hipGetLastError());
  return TBLS_SUCCESS;
}

void sk_to_words(const uint8_t sk[32], uint64_t w[4]) {
  for (int i = 0; i < 4; i++) {
    uint64_t v = 0;
    for (int j = 0; j < 8; j++) v = (v << 8) | sk[32 - 8 * (i + 1) + j];
    w[i] = v;
  }
}

// sk < r (BLSSecretKey.fromBytes range, BLSSecretKey.java:30-40)
// n randomizers in [1, 2^64) from the OS entropy source (one getrandom call
// per 32 MiB), as BlstBLS12381.nextBatchRandomMultiplier draws from
// SecureRandom (l.191-195); 0 is redrawn (2^64 itself does not fit a u64).
int fill_random(uint64_t* r, size_t n) {
  uint8_t* p = reinterpret_cast<uint8_t*>(r);
  size_t left = n * 8;
  while (left) {
    const ssize_t got = getrandom(p, left < (32u << 20) ? left : (32u << 20), 0);
    if (got <= 0) return TBLS_DEVICE_ERROR;
    p += got;
    left -= (size_t)got;
  }
  for (size_t i = 0; i < n; i++)
    while (r[i] == 0)
      if (getrandom(&r[i], 8, 0) != 8) return TBLS_DEVICE_ERROR;
  return TBLS_SUCCESS;
}

bool sk_in_range(const uint8_t sk[32]) {
  static const uint8_t R_BE[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                   0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
  return memcmp(sk, R_BE, 32) < 0;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" int tbls_init(int n_devices, uint32_t flags) {
  const caller_device keep;
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_inited) return g_ctx.empty() ? TBLS_DEVICE_ERROR : TBLS_SUCCESS;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    g_inited = true;
    return TBLS_DEVICE_ERROR;
  }
  const int hw = count;
  g_pk_lookup = !(getenv("TBLS_PK_LOOKUP") && getenv("TBLS_PK_LOOKUP")[0] == '0');
  // The learned key cache's rows per device: TBLS_PK_CACHE_KEYS (default
  // 2,097,152: about 320 MB with the slots); none with TBLS_PK_CACHE=0 or
  // without lookups.
  uint32_t cache_rows = 2097152u;
  if (const char* v = getenv("TBLS_PK_CACHE_KEYS")) cache_rows = (uint32_t)std::min<unsigned long long>(strtoull(v, nullptr, 10), 1ull << 28);
  if (!g_pk_lookup || (getenv("TBLS_PK_CACHE") && getenv("TBLS_PK_CACHE")[0] == '0')) cache_rows = 0;
  const bool comb_on = !(getenv("TBLS_PK_COMB") && getenv("TBLS_PK_COMB")[0] == '0');
  uint32_t comb_rows_cap = cache_rows;
  if (const char* v = getenv("TBLS_PK_COMB_KEYS")) comb_rows_cap = (uint32_t)std::min<unsigned long long>(strtoull(v, nullptr, 10), cache_rows);
  if ((flags & TBLS_INIT_SHARE_DEVICES) && n_devices > 0 && n_devices <= 32)
    count = n_devices;  // contexts over the hardware devices round-robin
  else if (n_devices > 0 && n_devices < count)
    count = n_devices;
  for (int d = 0; d < count; d++) {
    dev_ctx* c = new dev_ctx();
    // the cache's hash seed: from the OS entropy source, as the table index's
    if (!c->init(d % hw) || (cache_rows && fill_random(&c->pkc_seed, 1))) {
      delete c;
      break;
    }
    c->pkc_rows = cache_rows;
    // comb rows for the keys the device keeps, unless TBLS_PK_COMB=0; the
    // cache's region holds TBLS_PK_COMB_KEYS rows (default: every cache row,
    // 1,440 B each -- 3.0 GB at 2,097,152), allocated with the cache
    if (comb_on && !c->pkcomb_stat.ensure(32) && hipMemset(c->pkcomb_stat.p, 0, 32) == hipSuccess) {
      c->pkcomb_on = true;
      c->pkcomb_cap = std::min(comb_rows_cap, cache_rows);
    }
    // the hash-point memo's rows per device: TBLS_MSG_MEMO (default 0: off)
    if (const char* v = getenv("TBLS_MSG_MEMO")) c->memo.configure((uint32_t)std::min<unsigned long long>(strtoull(v, nullptr, 10), TB_MEMO_ROWS_MAX));
    g_ctx.push_back(c);
  }
  (void)hipGetLastError();  // a context that failed to set up leaves no sticky error for later calls' checks
  g_inited = true;
  return g_ctx.empty() ? TBLS_DEVICE_ERROR : TBLS_SUCCESS;
}

extern "C" void tbls_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  const caller_device keep;
  if (g_rccl.ok)
    for (auto& kv : g_rccl.comms)
      for (ncclComm_t cm : kv.second) (void)g_rccl.CommDestroy(cm);
  g_rccl.comms.clear();
  g_rccl.ok = g_rccl.tried = false;
  for (dev_ctx* c : g_ctx) delete c;
  g_ctx.clear();
  g_inited = false;
}

extern "C" int tbls_device_count(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return (int)g_ctx.size();
}

template <class SET>
int batch_verify_impl(const SET* sets, size_t n, const uint64_t* rand, int n_gpus, int* ok, tbls_timing* t, group_mode gm = GROUP_OFF) {
  auto t0 = std::chrono::steady_clock::now();
  const caller_device keep;
  *ok = 0;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  if (n == 0) return TBLS_SUCCESS;  // BLS.java:240-241
  for (size_t i = 0; i < n; i++)
    if (sets[i].n_pks == 0) return TBLS_BAD_ARGUMENT;
  batch_pass<SET> pass;
  if (const int rc = pass.run(sets, n, rand, n_gpus, ok, gm)) return rc;
  pass.timing(t, t0);
  return TBLS_SUCCESS;
}

extern "C" int tbls_batch_verify_grouped(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, uint32_t flags, int* ok,
                                         tbls_timing* t) {
  return batch_verify_impl(sets, n, rand, n_gpus, ok, t, group_mode_of(flags));
}

extern "C" int tbls_batch_verify_idx_grouped(const tbls_set_idx* sets, size_t n, const uint64_t* rand, int n_gpus, uint32_t flags, int* ok,
                                             tbls_timing* t) {
  return batch_verify_impl(sets, n, rand, n_gpus, ok, t, group_mode_of(flags));
}

extern "C" int tbls_group_plan(uint32_t n, uint32_t n_msgs, int* grouped, uint32_t* n_pairs) {
  int g = 0;
  uint32_t np = 0;
  group_plan(n, n_msgs, g, np);
  if (grouped) *grouped = g;
  if (n_pairs) *n_pairs = np;
  return TBLS_SUCCESS;
}

extern "C" int tbls_batch_verify(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, int* ok, tbls_timing* t) {
  return batch_verify_impl(sets, n, rand, n_gpus, ok, t);
}

// tbls_batch_verify_each: the randomized batch, and on failure each set's
// verdict settled from the batch's own work on the devices that ran it
// (settle_range), under the pass's locks.  Sets with no keys are false and
// left out of the batch.
// gm != GROUP_OFF (tbls_batch_verify_each_grouped): each shard groups its sets
// as tbls_batch_verify_grouped does.  When the batch fails, a pass of several
// shards first tests each shard's own partial record (one final
// exponentiation per shard, on its device) and settles only the shards that
// fail; a failed shard that ran grouped settles from the grouped pass's
// workspace (settle_grouped), one that ran ungrouped as above.
static int batch_verify_each_impl(const tbls_set* sets_in, size_t n_in, const uint64_t* rand_in, int n_gpus, group_mode gm, int* ok,
                                  int* ok_per_set, tbls_timing* t) {
  auto t0 = std::chrono::steady_clock::now();
  const caller_device keep;
  if (!ok || (n_in && (!sets_in || !rand_in || !ok_per_set))) return TBLS_BAD_ARGUMENT;
  *ok = 0;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  if (n_in == 0) return TBLS_SUCCESS;  // BLS.java:240-241
  std::vector<tbls_set> sets;
  std::vector<uint64_t> rand;
  std::vector<size_t> pos;
  for (size_t i = 0; i < n_in; i++) {
    ok_per_set[i] = 0;  // an empty key list: false (BLS.java:193-195)
    if (sets_in[i].n_pks) {
      sets.push_back(sets_in[i]);
      rand.push_back(rand_in[i]);
      pos.push_back(i);
    }
  }
  const size_t n = sets.size();
  if (n == 0) return TBLS_SUCCESS;
  batch_pass<tbls_set> pass;
  if (const int rc = pass.run(sets.data(), n, rand.data(), n_gpus, ok, gm)) return rc;
  std::vector<uint8_t> verdict(n, 1);
  if (!*ok) {
    const placed& pl = pass.pl;
    std::vector<int> rcs(pl.G, 0);
    for_each_shard(pl.G, [&](int g) {
      dev_ctx* c = pass.ctx(g);
      if (hipSetDevice(c->dev) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
        rcs[g] = TBLS_DEVICE_ERROR;
        return;
      }
      const shard_run& R = pass.runs[g];
      if (gm != GROUP_OFF && pl.G > 1) {  // this shard alone: a record that passes holds only valid sets
        int ok_g = 0;
        if ((rcs[g] = launch_final(*c, R.dpart, 1, c->stream, &ok_g)) || ok_g) return;
      }
      rcs[g] = R.n_msgs ? settle_grouped(c, R, verdict.data() + pl.cut[g])
                        : settle_range(c, sets.data(), pl.cut[g], pl.cut[g + 1], rand.data(), R, verdict.data() + pl.cut[g]);
    });
    for (int g = 0; g < pl.G; g++)
      if (rcs[g]) return rcs[g];
  }
  for (size_t k = 0; k < n; k++) ok_per_set[pos[k]] = verdict[k];
  if (n != n_in) *ok = 0;  // a set without keys fails the whole batch as well
  pass.timing(t, t0);       // settling is in total_ms
  return TBLS_SUCCESS;
}

extern "C" int tbls_batch_verify_each(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, int* ok, int* ok_per_set, tbls_timing* t) {
  return batch_verify_each_impl(sets, n, rand, n_gpus, GROUP_OFF, ok, ok_per_set, t);
}

extern "C" int tbls_batch_verify_each_grouped(const tbls_set* sets, size_t n, const uint64_t* rand, int n_gpus, uint32_t flags, int* ok,
                                              int* ok_per_set, tbls_timing* t) {
  return batch_verify_each_impl(sets, n, rand, n_gpus, group_mode_of(flags), ok, ok_per_set, t);
}

// --------------------------------------------------------------------------
// device-resident public-key table
// --------------------------------------------------------------------------
extern "C" int tbls_pk_table_load(const uint8_t* pks, size_t K, uint8_t* codes) {
  const caller_device keep;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  if (K == 0 || K > 0xffffffffu / 96) return TBLS_BAD_ARGUMENT;
  const bool index = [] {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_pk_lookup;
  }();
  uint64_t seed = 0;  // of this load's index: from the OS entropy source, as the randomizers
  if (index && fill_random(&seed, 1)) return TBLS_DEVICE_ERROR;
  const uint32_t cap = tb::pkx_capacity((uint32_t)K);
  return each_device(true, true, [&](dev_ctx* c) -> int {  // the old table's last readers have finished
    c->tab_n = 0;
    c->pkx_cap = 0;                          // and no index until this load's is complete
    for (uint32_t& sz : c->cm_size) sz = 0;  // the committees' indices meant the old table
    if (c->in.ensure(K * 48) || c->tab_aff.ensure(K * sizeof(g1a)) || c->tab_code.ensure(K)) return TBLS_DEVICE_ERROR;
    HIPCHK(hipMemcpyAsync(c->in.p, pks, K * 48, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pk_decompress, dim3((uint32_t)((K + TB_BLOCK - 1) / TB_BLOCK)), dim3(TB_BLOCK), 0, c->stream,
                       c->in.as<const uint8_t>(), (uint32_t)K, c->tab_aff.as<g1a>(), c->tab_code.as<uint8_t>());
    HIPCHK(hipGetLastError());
    if (codes) HIPCHK(hipMemcpyAsync(codes, c->tab_code.p, K, hipMemcpyDeviceToHost, c->stream));
    codes = nullptr;  // from the first device only
    if (index) {
      // the keys stay resident beside their points, and every slot is cleared:
      // nothing of an earlier table's index survives.  The stream is
      // synchronised below, under the lock, before any lookup can run.
      if (c->tab_keys.ensure(K * 48) || c->pkx_slots.ensure((size_t)cap * 4) || c->pkx_stat.ensure(16)) return TBLS_DEVICE_ERROR;
      HIPCHK(hipMemcpyAsync(c->tab_keys.p, c->in.p, K * 48, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemsetAsync(c->pkx_slots.p, 0, (size_t)cap * 4, c->stream));
      HIPCHK(hipMemsetAsync(c->pkx_stat.p, 0, 16, c->stream));
      hipLaunchKernelGGL(k_pkx_build, dim3((uint32_t)((K + TB_PKX_BLOCK - 1) / TB_PKX_BLOCK)), dim3(TB_PKX_BLOCK), 0, c->stream,
                         c->tab_keys.as<const uint32_t>(), (uint32_t)K, c->pkx_slots.as<uint32_t>(), cap - 1u, seed);
      HIPCHK(hipGetLastError());
    }
    // the table's comb region: a row per key, built from the points just
    // decompressed; without the memory for it the table works as before
    if (c->pkcomb_on) {
      if (c->tab_comb.ensure(K * TB_PKCOMB_ROW_BYTES, true)) {
        (void)hipGetLastError();
        c->tab_comb.release();
      } else {
        hipLaunchKernelGGL(k_pk_comb_build, pkcomb_grid((uint32_t)K), dim3(TB_PKCOMB_BLOCK), 0, c->stream, c->tab_aff.as<const g1a>(),
                           c->tab_code.as<const uint8_t>(), (uint32_t)K, c->tab_comb.as<g1a>(), c->pkcomb_stat.as<unsigned long long>());
        HIPCHK(hipGetLastError());
      }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->tab_n = (uint32_t)K;
    if (index) {
      c->pkx_seed = seed;
      c->pkx_cap = cap;
    }
    return TBLS_SUCCESS;
  });
}

// Drop the table, its index and the committees on every device.
extern "C" int tbls_pk_table_clear(void) {
  const caller_device keep;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  return each_device(true, true, [&](dev_ctx* c) -> int {
    c->tab_n = 0;
    c->pkx_cap = 0;
    for (uint32_t& sz : c->cm_size) sz = 0;
    for (dbuf* b : {&c->tab_aff, &c->tab_code, &c->tab_keys, &c->pkx_slots, &c->cmt, &c->tab_comb}) b->release();
    if (c->pkx_stat.p) HIPCHK(hipMemset(c->pkx_stat.p, 0, 16));
    return TBLS_SUCCESS;
  });
}

// One device pass over n keys: the table index of each key's bytes.
extern "C" int tbls_pk_table_resolve(const uint8_t* pks, size_t n, uint32_t* idx_out) {
  if (n && (!pks || !idx_out)) return TBLS_BAD_ARGUMENT;
  if (n > 0xffffffffu / 48) return TBLS_BAD_ARGUMENT;
  return with_device([&](dev_ctx& c) -> int {
    if (!pk_table_index_on(c)) return (int)TBLS_BAD_ARGUMENT;  // no table (or no index: TBLS_PK_LOOKUP=0)
    if (!n) return (int)TBLS_SUCCESS;
    const size_t o_idx = align_up(n * 48);
    if (c.in.ensure(o_idx + n * 4)) return (int)TBLS_DEVICE_ERROR;
    HIPCHK(hipMemcpyAsync(c.in.p, pks, n * 48, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(k_pk_resolve, dim3((uint32_t)((n + TB_PKX_BLOCK - 1) / TB_PKX_BLOCK)), dim3(TB_PKX_BLOCK), 0, c.stream,
                       c.in.as<const uint8_t>(), (uint32_t)n, pkx_align(c.in.p), c.pkx_slots.as<const uint32_t>(), c.pkx_cap - 1u, c.pkx_seed,
                       c.tab_keys.as<const uint32_t>(), c.in.as<uint32_t>(o_idx));
    return fetch(c, idx_out, c.in.as<uint8_t>(o_idx), n * 4);
  });
}

// Hits and misses of the batch key stages' lookups, summed over the devices.
extern "C" int tbls_pk_lookup_stats(uint64_t out[2], int reset) {
  const caller_device keep;
  if (!out) return TBLS_BAD_ARGUMENT;
  out[0] = out[1] = 0;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  return each_device(true, false, [&](dev_ctx* c) -> int {  // key stages queued on a caller's stream count too
    if (!c->pkx_stat.p) return TBLS_SUCCESS;
    uint64_t v[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(v, c->pkx_stat.p, 16, hipMemcpyDeviceToHost, c->stream));
    if (reset) HIPCHK(hipMemsetAsync(c->pkx_stat.p, 0, 16, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out[0] += v[0];
    out[1] += v[1];
    return TBLS_SUCCESS;
  });
}

// The learned key caches' counters, summed over the devices: lookups' hits,
// rows learned, keys refused by a full cache, rows in use.
extern "C" int tbls_pk_cache_stats(uint64_t out[4], int reset) {
  const caller_device keep;
  if (!out) return TBLS_BAD_ARGUMENT;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  return each_device(true, false, [&](dev_ctx* c) -> int {  // key stages queued on a caller's stream count too
    if (!c->pkc_rows || !c->pkc.p) return TBLS_SUCCESS;
    uint64_t v[1 + tb::TB_PKC_STATS] = {0, 0, 0, 0};  // the head: the row counter (a 32-bit word), the counters
    HIPCHK(hipMemcpyAsync(v, c->pkc.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    if (reset) HIPCHK(hipMemsetAsync(c->pkc.as<uint8_t>(8), 0, 8 * tb::TB_PKC_STATS, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < tb::TB_PKC_STATS; i++) out[i] += v[1 + i];
    out[3] += std::min<uint64_t>(v[0] & 0xffffffffu, c->pkc_rows);  // appenders racing for the last rows overshoot the counter
    return TBLS_SUCCESS;
  });
}

// Forget every learned key on every device (the counters too); the buffers stay.
extern "C" int tbls_pk_cache_clear(void) {
  const caller_device keep;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  return each_device(true, true, [&](dev_ctx* c) -> int {  // the last key stage has finished
    if (!c->pkc_rows || !c->pkc.p) return TBLS_SUCCESS;
    HIPCHK(hipMemsetAsync(c->pkc.p, 0, pkc_zeroed_bytes(*c), c->stream));
    if (pk_cache_comb_on(*c)) HIPCHK(hipMemsetAsync(c->pkcomb.p, 0, c->pkcomb_cap, c->stream));  // no row's comb is ready
    HIPCHK(hipStreamSynchronize(c->stream));
    c->pk_seen_K = 0;  // and nothing is expected of the next batch's keys (pk_keys_known)
    return TBLS_SUCCESS;
  });
}

// The comb rows' counters, summed over the devices: sets whose [r] pk came
// from a comb row, rows built for the learned caches, rows built for the
// loaded tables, and the caches' comb rows' capacity (0: no region).
extern "C" int tbls_pk_comb_stats(uint64_t out[4], int reset) {
  const caller_device keep;
  if (!out) return TBLS_BAD_ARGUMENT;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  return each_device(true, false, [&](dev_ctx* c) -> int {  // key stages queued on a caller's stream count too
    if (!c->pkcomb_on) return TBLS_SUCCESS;
    uint64_t v[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(v, c->pkcomb_stat.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    if (reset) HIPCHK(hipMemsetAsync(c->pkcomb_stat.p, 0, sizeof v, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; i++) out[i] += v[i];
    if (pk_cache_comb_on(*c)) out[3] += c->pkcomb_cap;
    return TBLS_SUCCESS;
  });
}

// --------------------------------------------------------------------------
// the hash-point memo (tb_msgmemo.h)
// --------------------------------------------------------------------------
// Rows per device (0: off), for batches staged afterwards; everything learned
// is forgotten and the row buffers are dropped (the next shard that resolves
// allocates its device's anew).
extern "C" int tbls_msg_memo_configure(uint32_t rows) {
  const caller_device keep;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  return each_device(true, true, [&](dev_ctx* c) -> int {  // the rows' last readers have finished
    c->memo.configure(rows);
    c->memo_rows.release();
    return TBLS_SUCCESS;
  });
}

// Pairs served from a row learned by an earlier call, messages hashed,
// flushes, rows in use (not reset), summed over the devices.
extern "C" int tbls_msg_memo_stats(uint64_t out[4], int reset) {
  const caller_device keep;
  if (!out) return TBLS_BAD_ARGUMENT;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  return each_device(false, false, [&](dev_ctx* c) -> int {  // the index is host state under the device's lock
    out[0] += c->memo.hits;
    out[1] += c->memo.hashed;
    out[2] += c->memo.flushes;
    out[3] += c->memo.used;
    if (reset) c->memo.reset_counters();
    return TBLS_SUCCESS;
  });
}

// Forget every learned hash point on every device; the buffers and the counters stay.
extern "C" int tbls_msg_memo_clear(void) {
  const caller_device keep;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  return each_device(false, false, [&](dev_ctx* c) -> int {  // rows are reassigned only by kernels queued behind ws_acquire
    c->memo.invalidate();
    return TBLS_SUCCESS;
  });
}

extern "C" size_t tbls_pk_table_size(void) {
  if (ensure_init()) return 0;
  dev_ctx* c = ctx_for(0);
  std::lock_guard<std::mutex> lk(c->mu);
  return c->tab_n;
}

extern "C" int tbls_batch_verify_idx(const tbls_set_idx* sets, size_t n, const uint64_t* rand, int n_gpus, int* ok, tbls_timing* t) {
  // indices are checked against each device's table under that device's lock (shard_launch)
  return batch_verify_impl(sets, n, rand, n_gpus, ok, t);
}

// core_verify through the same pipeline with r = 1 (one set, no randomizer)
static int verify_one(const uint8_t* pks, uint32_t n_pks, const uint8_t* msg, size_t len, const uint8_t sig[96], const uint8_t* dst,
                      size_t dlen, int* ok, uint8_t* code_out) {
  const caller_device keep;
  *ok = 0;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  if (dlen > 255) return TBLS_BAD_ARGUMENT;
  tbls_set s = {pks, n_pks, msg, (uint32_t)len, sig};
  uint8_t code = 0;
  uint64_t one = 1;
  placed pl;
  place_one(pl);
  int rc = verify_on_device(pl.dev[0], &s, 1, &one, dst, (uint32_t)dlen, ok, &code);
  if (code_out) *code_out = code;
  return rc;
}

extern "C" int tbls_verify(const uint8_t pk[48], const uint8_t* msg, size_t len, const uint8_t sig[96], const uint8_t* dst, size_t dlen,
                           int* ok) {
  uint8_t code = 0;
  int rc = verify_one(pk, 1, msg, len, sig, dst, dlen, ok, &code);
  if (rc) return rc;
  if (code == TB_BAD_ENCODING || code == TB_POINT_NOT_ON_CURVE) return code;  // decode failures are errors
  return TBLS_SUCCESS;
}

// Per-set fastAggregateVerify verdicts for sets[lo, hi) on device d in one
// pass (k_each.hip): shared per-set stages with r = 1, then one thread per set
// for its two-pair Miller loop and final exponentiation.
// Keys as bytes (decompressed here), table indices or committee bit rows.
// With a hash-point memo on the device the messages are resolved as
// shard_launch resolves them (one pair per set): the messages left are hashed
// into Qh / skiph behind the pass's workspace, k_memo_fill gives every set its
// Q, and k_memo_learn follows, all on the one stream.
template <class SET>
static int run_each_resolved(dev_ctx* c, const SET* sets, size_t lo, size_t hi, uint8_t* ok_host, bool& resolved);
template <class SET>
static int run_each(int d, const SET* sets, size_t lo, size_t hi, uint8_t* ok_host) {
  dev_ctx* c = ctx_for(d);
  if (!c) return TBLS_DEVICE_ERROR;
  std::lock_guard<std::mutex> lk(c->mu);
  bool resolved = false;
  const int rc = run_each_resolved(c, sets, lo, hi, ok_host, resolved);
  if (rc && resolved) c->memo.invalidate();  // the rows it promised may never have been written
  return rc;
}
template <class SET>
static int run_each_resolved(dev_ctx* c, const SET* sets, size_t lo, size_t hi, uint8_t* ok_host, bool& resolved) {
  constexpr bool bytes_mode = std::is_same<SET, tbls_set>::value, bits_mode = std::is_same<SET, set_bits_i>::value;
  tb::stat_add(tb::TB_STAT_EACH);
  HIPCHK(hipSetDevice(c->dev));
  if (const int rc = check_keys(c, sets, lo, hi)) return rc;
  tb::memo::packed_memo p;
  static_cast<packed&>(p) = pack_layout(sets, lo, hi, 43);
  const bool use_memo = hi > lo && hi - lo <= TB_MEMO_SETS_MAX && memo_reserve(*c);
  groups G;
  tb::memo::resolved MR;
  if (use_memo) {
    G = group_messages(sets, lo, hi);
    MR = c->memo.resolve(G, true);
    resolved = true;
    p = tb::memo::pack_layout_memo(p, false, G, MR);
  }
  if (c->hin.ensure(p.total + 256) || c->in.ensure(p.total + 256)) return TBLS_DEVICE_ERROR;
  pack_fill(c->hin.as<uint8_t>(), p, sets, lo, nullptr, ETH2_DST, 43);  // r = 1 for every set
  if (use_memo) tb::memo::pack_fill_memo(c->hin.as<uint8_t>(), p, G, MR);
  hipStream_t s = c->stream;
  HIPCHK(ws_acquire(*c, s));
  HIPCHK(hipStreamSynchronize(s));  // ws may be reallocated below
  HIPCHK(hipMemcpyAsync(c->in.p, c->hin.p, p.total, hipMemcpyHostToDevice, s));
  const uint8_t* di = c->in.as<uint8_t>();
  const uint32_t n = p.n, K = bytes_mode ? p.K : 0u;  // keys to decompress
  const each_layout E(n, K);
  const uint32_t m_hash = use_memo ? p.m_hash : 0u;
  const size_t o_qh = E.total, o_skiph = o_qh + align_up((size_t)m_hash * sizeof(g2a));  // the hashed points, behind the pass's regions
  if (c->ws.ensure(o_skiph + align_up(m_hash))) return TBLS_DEVICE_ERROR;
  if (const int rc = pk_lookup_reserve(*c, K, s)) return rc;
  uint8_t* w = c->ws.as<uint8_t>();
  g1a* P = (g1a*)(w + E.P);
  g2a *Q = (g2a*)(w + E.Q), *sig_aff = (g2a*)(w + E.sig_aff);
  uint8_t *skip = w + E.skip, *set_code = w + E.set_code, *sig_code = w + E.sig_code, *sig_use = w + E.sig_use, *okd = w + E.okd;
  uint32_t* n_bad = (uint32_t*)(w + E.n_bad);
  const uint64_t* rand = (const uint64_t*)(di + p.off_rand);
  const key_src keys = bytes_mode ? own_keys((const g1a*)(w + E.pk_aff), w + E.pk_code) : table_keys(*c, (const uint32_t*)(di + p.off_pks));
  const dim3 blk(TB_BLOCK), g((n + TB_BLOCK - 1) / TB_BLOCK);
  HIPCHK(hipMemsetAsync(n_bad, 0, 4, s));
  HIPCHK(hipMemsetAsync(set_code, 0, n, s));  // k_set_pk writes failures only
  // byte keys: from the table's index where it holds them, the others (or all) decompressed
  // a cache with comb rows learns behind k_set_pk (the rows' build is the longer kernel, and nothing here reads it)
  const bool learn_late = bytes_mode && pk_cache_comb_on(*c);
  if (const int rc = launch_byte_keys(*c, s, di + p.off_pks, K, (g1a*)(w + E.pk_aff), w + E.pk_code, false, !learn_late)) return rc;
  if constexpr (bits_mode) {
    if (n) launch_set_pk_bits(s, n, keys, committee_src(*c, sets[lo].slot), rand, P, set_code, n_bad, nullptr, nullptr, 1u);
  } else {
    comb_rows rows;
    const bool has_rows = pk_comb_rows(*c, !bytes_mode, rows);
    launch_set_pk(s, n, use_w2(n), multi_key(n, p.K), (const uint32_t*)(di + p.off_pkoff), keys, rand, P, set_code, n_bad, (uint32_t*)(w + E.mlist), (uint32_t*)(w + E.mcnt),
                  nullptr, nullptr, has_rows ? &rows : nullptr);
  }
  if (learn_late) launch_pk_learn(*c, s, di + p.off_pks, K, (const g1a*)(w + E.pk_aff), w + E.pk_code);
  hipLaunchKernelGGL(k_sig_check, g, blk, 0, s, di + p.off_sigs, n, sig_aff, sig_use, sig_code, n_bad, 0u);
  if (!use_memo) {
    hipLaunchKernelGGL(k_set_hash, g, blk, 0, s, di + p.off_msgs, (const uint32_t*)(di + p.off_msgoff), di + p.off_dst, 43u, n, Q, skip);
  } else {
    g2a* Qh = (g2a*)(w + o_qh);
    uint8_t* skiph = w + o_skiph;
    if (m_hash)
      hipLaunchKernelGGL(k_set_hash, dim3((m_hash + TB_BLOCK - 1) / TB_BLOCK), blk, 0, s, di + p.off_hmsgs, (const uint32_t*)(di + p.off_hmsgoff),
                         di + p.off_dst, 43u, m_hash, Qh, skiph);
    hipLaunchKernelGGL(k_memo_fill, memo_grid(n), dim3(TB_MEMO_BLOCK), 0, s, (const uint32_t*)(di + p.off_src), (const uint32_t*)(di + p.off_setgrp),
                       n, (const g2a*)Qh, (const uint8_t*)skiph, c->memo_rows.as<const g2a>(), memo_row_skip(*c), Q, skip);
    if (m_hash)
      hipLaunchKernelGGL(k_memo_learn, memo_grid(m_hash), dim3(TB_MEMO_BLOCK), 0, s, (const uint32_t*)(di + p.off_learn), m_hash, (const g2a*)Qh,
                         (const uint8_t*)skiph, c->memo_rows.as<g2a>(), memo_row_skip(*c));
  }
  hipLaunchKernelGGL(k_verify_each, g, blk, 0, s, (const g1a*)P, (const g2a*)Q, (const uint8_t*)skip, (const uint8_t*)set_code,
                     (const g2a*)sig_aff, (const uint8_t*)sig_use, (const uint8_t*)sig_code, n, okd);
  HIPCHK(hipGetLastError());
  if (c->hout.ensure(n)) return TBLS_DEVICE_ERROR;
  HIPCHK(hipMemcpyAsync(c->hout.p, okd, n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(ws_release(*c, s));
  memcpy(ok_host, c->hout.p, n);
  return TBLS_SUCCESS;
}

#define TB_EACH_CHUNK 65536u  // sets per device pass (bounds staging and workspace)

template <class SET>
static int verify_each_impl(const SET* sets, size_t n, int n_gpus, int* ok_per_set) {
  const caller_device keep;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  if (n == 0) return TBLS_SUCCESS;
  const size_t nchunks = (n + TB_EACH_CHUNK - 1) / TB_EACH_CHUNK;
  // one device per chunk, at most nchunks least-loaded devices (place_plan with
  // one-set "chunks"); chunk k runs on pl.dev[k % G], one host thread per device
  placed pl;
  place_batch(pl, nchunks, [](size_t) { return 0u; }, n_gpus, 1, 0);
  const int G = pl.G;
  std::vector<uint8_t> ok(n, 0);
  std::vector<int> rcs(G, 0);
  for_each_shard(G, [&](int k0) {
    for (size_t k = k0; k < nchunks && !rcs[k0]; k += G) {
      const size_t lo = k * TB_EACH_CHUNK, hi = std::min(n, lo + TB_EACH_CHUNK);
      rcs[k0] = run_each(pl.dev[k0], sets, lo, hi, ok.data() + lo);
    }
  });
  for (int k = 0; k < G; k++)
    if (rcs[k]) return rcs[k];
  for (size_t i = 0; i < n; i++) ok_per_set[i] = (sets[i].n_pks != 0 && ok[i]) ? 1 : 0;  // BLS.java:193-195
  return TBLS_SUCCESS;
}

extern "C" int tbls_verify_each(const tbls_set* sets, size_t n, int n_gpus, int* ok_per_set) {
  return verify_each_impl(sets, n, n_gpus, ok_per_set);
}

// fastAggregateVerify of every set (config 2: sync-committee sets of 512 keys).
// A randomized batch over the sets with keys settles the common all-valid
// case with one final exponentiation: it accepts iff every set verifies (with
// probability 1 - 2^-64 per forged set), and then every such set's verdict is
// 1.  Otherwise the per-set pass (tbls_verify_each) gives the verdicts.
template <class SET>
static int fast_aggregate_verify_many_impl(const SET* sets, size_t n, int* ok_per_set) {
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  if (n == 0) return TBLS_SUCCESS;
  std::vector<SET> keyed;
  std::vector<size_t> pos;
  for (size_t i = 0; i < n; i++) {
    ok_per_set[i] = 0;  // empty key list -> false (BLS.java:193-195)
    if (sets[i].n_pks) {
      keyed.push_back(sets[i]);
      pos.push_back(i);
    }
  }
  if (keyed.size() >= 2) {
    std::vector<uint64_t> rnd(keyed.size());
    if (fill_random(rnd.data(), rnd.size())) return TBLS_DEVICE_ERROR;
    int ok = 0;
    const int rc = batch_verify_impl(keyed.data(), keyed.size(), rnd.data(), 1, &ok, nullptr);
    if (rc != TBLS_SUCCESS) return rc;
    if (ok) {
      for (size_t p : pos) ok_per_set[p] = 1;
      return TBLS_SUCCESS;
    }
  }
  return verify_each_impl(sets, n, 1, ok_per_set);
}

extern "C" int tbls_fast_aggregate_verify_many(const tbls_set* sets, size_t n, int* ok_per_set) {
  return fast_aggregate_verify_many_impl(sets, n, ok_per_set);
}

// The same with keys by table index: the batch and the per-set pass read the
// resident table (no upload, decompression or subgroup check of keys); the
// table and every index are checked under the device lock (check_keys).
extern "C" int tbls_fast_aggregate_verify_many_idx(const tbls_set_idx* sets, size_t n, int* ok_per_set) {
  if (n && (!sets || !ok_per_set)) return TBLS_BAD_ARGUMENT;
  for (size_t i = 0; i < n; i++)
    if (sets[i].n_pks && !sets[i].key_idx) return TBLS_BAD_ARGUMENT;
  return fast_aggregate_verify_many_impl(sets, n, ok_per_set);
}

// --------------------------------------------------------------------------
// resident committees: the index list, the bad-member mask and the valid
// members' sum on every device, beside its key table
// --------------------------------------------------------------------------
extern "C" int tbls_committee_load(uint32_t slot, const uint32_t* key_idx, uint32_t size) {
  const caller_device keep;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  if (slot >= TBLS_COMMITTEE_SLOTS || !key_idx || size == 0 || size > TBLS_COMMITTEE_MAX) return TBLS_BAD_ARGUMENT;
  return each_device(false, true, [&](dev_ctx* c) -> int {
    if (!c->tab_n) return TBLS_BAD_ARGUMENT;
    for (uint32_t i = 0; i < size; i++)
      if (key_idx[i] >= c->tab_n) return TBLS_BAD_ARGUMENT;
    hipStream_t s = c->stream;
    c->cm_size[slot] = 0;
    if (c->cmt.ensure((size_t)TBLS_COMMITTEE_SLOTS * TB_CM_STRIDE)) return TBLS_DEVICE_ERROR;
    uint8_t* m = c->cmt.as<uint8_t>((size_t)slot * TB_CM_STRIDE);
    HIPCHK(hipMemsetAsync(m, 0, TB_CM_STRIDE, s));
    HIPCHK(hipMemcpyAsync(m, key_idx, (size_t)size * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_committee_mask, dim3(1), dim3(TB_CM_WORDS), 0, s, (const uint32_t*)m, size, c->tab_code.as<const uint8_t>(),
                       c->tab_n, (uint32_t*)(m + TB_CM_OFF_BAD), (uint32_t*)(m + TB_CM_OFF_VALID));
    // the committee sum: one set whose participants are the valid members,
    // on the direct side with r = 1; an exceptional addition is resolved by
    // the kernel's one-lane body, so only a sum at infinity leaves a code
    bits_src all = {(const uint32_t*)m, (const uint32_t*)(m + TB_CM_OFF_BAD), (const g1a*)(m + TB_CM_OFF_SUM), size, 0u, TB_CM_WORDS};
    launch_set_pk_bits(s, 1, table_keys(*c, (const uint32_t*)(m + TB_CM_OFF_VALID)), all, nullptr, (g1a*)(m + TB_CM_OFF_SUM), m + TB_CM_OFF_CODE,
                       (uint32_t*)(m + TB_CM_OFF_CODE + 4), nullptr, nullptr, 1u);
    HIPCHK(hipGetLastError());
    uint8_t code = 0xff;
    HIPCHK(hipMemcpyAsync(&code, m + TB_CM_OFF_CODE, 1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    c->cm_sum_ok[slot] = code == TB_SUCCESS ? 1u : 0u;
    c->cm_size[slot] = size;
    return TBLS_SUCCESS;
  });
}

extern "C" uint32_t tbls_committee_size(uint32_t slot) {
  if (slot >= TBLS_COMMITTEE_SLOTS || ensure_init()) return 0;
  dev_ctx* c = ctx_for(0);
  std::lock_guard<std::mutex> lk(c->mu);
  return c->cm_size[slot];
}

// fastAggregateVerify of sets given as participation bitvectors over the
// committee in `slot` (BlockProcessorAltair.java:234-267): the same two steps
// over the sets with a participant -- the randomized batch, then the per-set
// pass -- with the keys' stage on k_set_pk_bits_coop.
extern "C" int tbls_fast_aggregate_verify_many_bits(uint32_t slot, const tbls_set_bits* sets, size_t n, int* ok_per_set) {
  if (n && (!sets || !ok_per_set)) return TBLS_BAD_ARGUMENT;
  const uint32_t size = tbls_committee_size(slot);
  if (!size) return ensure_init() ? TBLS_DEVICE_ERROR : TBLS_BAD_ARGUMENT;
  const uint32_t nb = (size + 7u) / 8u;
  std::vector<set_bits_i> part;
  std::vector<size_t> pos;
  for (size_t i = 0; i < n; i++) {
    if (!sets[i].bits || !sets[i].sig) return TBLS_BAD_ARGUMENT;
    if ((size & 7u) && (sets[i].bits[nb - 1] >> (size & 7u))) return TBLS_BAD_ARGUMENT;  // a bit past the committee
    uint8_t any = 0;
    for (uint32_t k = 0; k < nb; k++) any |= sets[i].bits[k];
    ok_per_set[i] = 0;  // no participant: an empty key list (BLS.java:193-195)
    if (any) {
      part.push_back({sets[i].bits, bits_stride_w(size), sets[i].msg, sets[i].msg_len, sets[i].sig, slot, size});
      pos.push_back(i);
    }
  }
  if (part.empty()) return TBLS_SUCCESS;
  std::vector<int> ok(part.size(), 0);
  const int rc = fast_aggregate_verify_many_impl(part.data(), part.size(), ok.data());
  if (rc != TBLS_SUCCESS) return rc;
  for (size_t k = 0; k < part.size(); k++) ok_per_set[pos[k]] = ok[k];
  return TBLS_SUCCESS;
}

extern "C" int tbls_aggregate_verify(const uint8_t* pks, const uint8_t* const* msgs, const uint32_t* msg_lens, size_t n, const uint8_t sig[96],
                                     int* ok) {
  const caller_device keep;
  *ok = 0;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  if (n == 0) return TBLS_SUCCESS;
  static const uint8_t INF_SIG[96] = {0xc0};
  std::vector<tbls_set> sets(n);
  std::vector<uint64_t> ones(n, 1);
  for (size_t i = 0; i < n; i++) sets[i] = {pks + 48 * i, 1, msgs[i], msg_lens[i], i == 0 ? sig : INF_SIG};
  placed pl;
  place_one(pl);
  return verify_on_device(pl.dev[0], sets.data(), n, ones.data(), ETH2_DST, 43, ok, nullptr);
}

extern "C" int tbls_pk_validate(const uint8_t pk[48]) {
  tb::stat_add(tb::TB_STAT_ONE_VALIDATE);
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    size_t o = u.add(pk, 48);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(4096)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_pk_decompress, dim3(1), dim3(TB_BLOCK), 0, c.stream, d + o, 1u, c.ws.as<g1a>(0), c.ws.as<uint8_t>(1024));
    uint8_t code = 0;
    rc = fetch(c, &code, c.ws.as<uint8_t>(1024), 1);
    return rc ? rc : (int)code;
  });
}

extern "C" int tbls_sig_validate(const uint8_t sig[96], int* is_inf) {
  tb::stat_add(tb::TB_STAT_ONE_VALIDATE);
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    size_t o = u.add(sig, 96);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(4096)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_sig_validate, dim3(1), dim3(TB_BLOCK), 0, c.stream, d + o, 1u, c.ws.as<uint32_t>(0));
    uint32_t v = 0;
    rc = fetch(c, &v, c.ws.as<uint32_t>(0), 4);
    if (rc) return rc;
    if (is_inf) *is_inf = (v >> 8) & 1;
    return (int)(v & 0xff);
  });
}

// ---- batched deserialization / aggregation ----
extern "C" int tbls_pk_validate_many(const uint8_t* pks, size_t n, uint8_t* codes) {
  if (n == 0) return TBLS_SUCCESS;
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    size_t o = u.add(pks, 48 * n);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    const size_t aff = align_up(n * sizeof(g1a));
    if (c.ws.ensure(aff + align_up(n))) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_pk_decompress, dim3((uint32_t)((n + TB_BLOCK - 1) / TB_BLOCK)), dim3(TB_BLOCK), 0, c.stream, d + o, (uint32_t)n,
                       c.ws.as<g1a>(0), c.ws.as<uint8_t>(aff));
    return fetch(c, codes, c.ws.as<uint8_t>(aff), n);
  });
}

extern "C" int tbls_sig_validate_many(const uint8_t* sigs, size_t n, uint8_t* codes, uint8_t* is_inf) {
  if (n == 0) return TBLS_SUCCESS;
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    size_t o = u.add(sigs, 96 * n);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(4 * n)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_sig_validate, dim3((uint32_t)((n + TB_BLOCK - 1) / TB_BLOCK)), dim3(TB_BLOCK), 0, c.stream, d + o, (uint32_t)n,
                       c.ws.as<uint32_t>(0));
    std::vector<uint32_t> v(n);
    rc = fetch(c, v.data(), c.ws.as<uint32_t>(0), 4 * n);
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) {
      codes[i] = (uint8_t)(v[i] & 0xff);
      if (is_inf) is_inf[i] = (uint8_t)((v[i] >> 8) & 1);
    }
    return TBLS_SUCCESS;
  });
}

extern "C" int tbls_aggregate_sigs_many(const uint8_t* sigs, const uint32_t* off, size_t groups, uint8_t* out, int* status) {
  if (groups == 0) return TBLS_SUCCESS;
  for (size_t g = 0; g < groups; g++)
    if (off[g + 1] < off[g]) return TBLS_BAD_ARGUMENT;
  const size_t total = off[groups];
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    size_t os = u.add(sigs, 96 * total);
    size_t oo = u.add(off, 4 * (groups + 1));
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    const size_t ob = align_up(96 * groups);
    if (c.ws.ensure(ob + 4 * groups)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_aggregate_sigs_many, dim3((uint32_t)groups), dim3(TB_BLOCK), 0, c.stream, d + os, (const uint32_t*)(d + oo),
                       c.ws.as<uint8_t>(0), c.ws.as<int>(ob));
    rc = fetch(c, status, c.ws.as<int>(ob), 4 * groups);
    if (rc) return rc;
    return fetch(c, out, c.ws.as<uint8_t>(0), 96 * groups);
  });
}

extern "C" int tbls_aggregate_pks(const uint8_t* pks, size_t k, uint8_t out[48]) {
  if (k == 0) return TBLS_BAD_ARGUMENT;  // BlstPublicKey.java:56 checkArgument
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    size_t o = u.add(pks, 48 * k);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    const size_t aff = align_up(k * sizeof(g1a)), code = align_up(k);
    if (c.ws.ensure(aff + code + 256)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_pk_decompress, dim3((k + TB_BLOCK - 1) / TB_BLOCK), dim3(TB_BLOCK), 0, c.stream, d + o, (uint32_t)k, c.ws.as<g1a>(0),
                       c.ws.as<uint8_t>(aff));
    hipLaunchKernelGGL(k_aggregate_pks, dim3(1), dim3(TB_BLOCK), 0, c.stream, (const g1a*)c.ws.as<g1a>(0), (const uint8_t*)c.ws.as<uint8_t>(aff),
                       (uint32_t)k, c.ws.as<uint8_t>(aff + code));
    std::vector<uint8_t> codes(k);
    rc = fetch(c, codes.data(), c.ws.as<uint8_t>(aff), k);
    if (rc) return rc;
    // decode failures throw in BlstPublicKey.fromBytes (BlstPublicKey.java:39-44)
    for (size_t i = 0; i < k; i++)
      if (codes[i] == TB_BAD_ENCODING || codes[i] == TB_POINT_NOT_ON_CURVE) return (int)codes[i];
    return fetch(c, out, c.ws.as<uint8_t>(aff + code), 48);
  });
}

extern "C" int tbls_aggregate_sigs(const uint8_t* sigs, size_t k, uint8_t out[96]) {
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    size_t o = u.add(sigs, 96 * k);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(1024)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_aggregate_sigs, dim3(1), dim3(TB_BLOCK), 0, c.stream, d + o, (uint32_t)k, c.ws.as<uint8_t>(0), c.ws.as<int>(512));
    int status = 0;
    rc = fetch(c, &status, c.ws.as<int>(512), 4);
    if (rc) return rc;
    if (status) return status;
    return fetch(c, out, c.ws.as<uint8_t>(0), 96);
  });
}

extern "C" int tbls_hash_to_g2(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dlen, uint8_t out[96]) {
  if (dlen > 255) return TBLS_BAD_ARGUMENT;
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    uint32_t off[2] = {0, (uint32_t)len};
    size_t om = u.add(msg, len), oo = u.add(off, 8), od = u.add(dst, dlen);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(1024)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_hash_to_g2, dim3(1), dim3(TB_BLOCK), 0, c.stream, d + om, (const uint32_t*)(d + oo), d + od, (uint32_t)dlen, 1u,
                       c.ws.as<uint8_t>(0));
    return fetch(c, out, c.ws.as<uint8_t>(0), 96);
  });
}

extern "C" int tbls_sign(const uint8_t sk[32], const uint8_t* msg, size_t len, const uint8_t* dst, size_t dlen, uint8_t out[96]) {
  if (dlen > 255) return TBLS_BAD_ARGUMENT;
  if (!sk_in_range(sk)) return TBLS_BAD_SCALAR;
  bool zero = true;
  for (int i = 0; i < 32; i++) zero = zero && sk[i] == 0;
  if (zero) return TBLS_BAD_SCALAR;  // BlstBLS12381.java:54-56
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    uint64_t w[4];
    sk_to_words(sk, w);
    uint32_t off[2] = {0, (uint32_t)len};
    size_t ok_ = u.add(w, 32), om = u.add(msg, len), oo = u.add(off, 8), od = u.add(dst, dlen);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(1024)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_sign, dim3(1), dim3(TB_BLOCK), 0, c.stream, (const uint64_t*)(d + ok_), d + om, (const uint32_t*)(d + oo), d + od,
                       (uint32_t)dlen, 1u, c.ws.as<uint8_t>(0));
    return fetch(c, out, c.ws.as<uint8_t>(0), 96);
  });
}

extern "C" int tbls_sk_to_pk(const uint8_t sk[32], uint8_t out[48]) {
  if (!sk_in_range(sk)) return TBLS_BAD_SCALAR;
  return with_device([&](dev_ctx& c) -> int {
    upload u;
    uint64_t w[4];
    sk_to_words(sk, w);
    size_t ok_ = u.add(w, 32);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(1024)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_sk_to_pk, dim3(1), dim3(TB_BLOCK), 0, c.stream, (const uint64_t*)(d + ok_), 1u, c.ws.as<uint8_t>(0));
    return fetch(c, out, c.ws.as<uint8_t>(0), 48);
  });
}

extern "C" int tbls_dev_batch_partial(int device, const tbls_dev_batch* b, void* stream, void* partial_out) {
  return with_dev_stream(device, stream, [&](dev_ctx& c, hipStream_t s) {
    ws_layout L;
    return launch_partial(c, *b, s, partial_out, L, partial_opts{c.dstb.as<uint8_t>(), 43});
  });
}

extern "C" int tbls_dev_batch_partial_idx(int device, const tbls_dev_batch* b, const uint32_t* key_idx, void* stream, void* partial_out) {
  return with_dev_stream(device, stream, [&](dev_ctx& c, hipStream_t s) -> int {
    if (!c.tab_n || !key_idx) return TBLS_BAD_ARGUMENT;
    partial_opts o{c.dstb.as<uint8_t>(), 43};
    o.key_idx = key_idx;
    ws_layout L;
    return launch_partial(c, *b, s, partial_out, L, o);
  });
}

extern "C" int tbls_dev_batch_partial_grouped(int device, const tbls_dev_batch* b, const uint32_t* key_idx, uint32_t n_msgs,
                                              const uint32_t* grp_off, const uint32_t* grp_sets, void* stream, void* partial_out) {
  if (!b || !grp_off || !grp_sets || !n_msgs || n_msgs >= b->n) return TBLS_BAD_ARGUMENT;
  return with_dev_stream(device, stream, [&](dev_ctx& c, hipStream_t s) -> int {
    if (key_idx && !c.tab_n) return TBLS_BAD_ARGUMENT;
    partial_opts o{c.dstb.as<uint8_t>(), 43};
    o.key_idx = key_idx;
    o.n_msgs = n_msgs;
    o.grp_off = grp_off;
    o.grp_sets = grp_sets;
    ws_layout L;
    return launch_partial(c, *b, s, partial_out, L, o);
  });
}

static int partial_timed(int device, const tbls_dev_batch* b, void* stream, void* partial_out, float* stage_ms, bool serial) {
  return with_dev_stream(device, stream, [&](dev_ctx& c, hipStream_t s) -> int {
    hipEvent_t ev[TB_NSTAGE_EV];
    for (int i = 0; i < TB_NSTAGE_EV; i++) HIPCHK(hipEventCreate(&ev[i]));
    partial_opts o{c.dstb.as<uint8_t>(), 43};
    o.ev = ev;
    o.serial = serial;
    ws_layout L;
    int rc = launch_partial(c, *b, s, partial_out, L, o);
    if (!rc) {
      HIPCHK(hipEventSynchronize(ev[TB_NSTAGE_EV - 1]));
      static const int order[TB_NSTAGE] = {0, 1, 2, 3, 4, 5, 6};  // pk, set_pk, set_sig, set_hash, g2_sum, miller, prod
      const int evi[TB_NSTAGE] = {0, 2, 4, 6, 8, 10, 12};
      for (int i = 0; i < TB_NSTAGE; i++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev[evi[order[i]]], ev[evi[order[i]] + 1]);
        stage_ms[i] = ms;
      }
    }
    for (int i = 0; i < TB_NSTAGE_EV; i++) (void)hipEventDestroy(ev[i]);
    return rc;
  });
}

extern "C" int tbls_dev_batch_partial_timed(int device, const tbls_dev_batch* b, void* stream, void* partial_out, float* stage_ms) {
  return partial_timed(device, b, stream, partial_out, stage_ms, false);
}

extern "C" int tbls_dev_batch_stage_profile(int device, const tbls_dev_batch* b, void* stream, void* partial_out, float* stage_ms) {
  return partial_timed(device, b, stream, partial_out, stage_ms, true);
}

extern "C" int tbls_place_plan(size_t n, const uint32_t* n_pks, int n_devices, int n_gpus, const int* load, uint32_t rr,
                               uint32_t shard_min_sets, uint32_t shard_knee_sets, int* dev_out, size_t* cut_out) {
  if (n_devices < 1 || n_devices > 32 || !dev_out || !cut_out) return -TBLS_BAD_ARGUMENT;
  std::vector<int> dev(n_devices);
  std::vector<size_t> cut(n_devices + 1);
  const int G = place_plan(n, [&](size_t i) { return n_pks ? n_pks[i] : 1u; }, n_devices, n_gpus, load, rr, shard_min_sets, shard_knee_sets,
                           dev.data(), cut.data());
  for (int k = 0; k < G; k++) dev_out[k] = dev[k];
  for (int k = 0; k <= G; k++) cut_out[k] = cut[k];
  return G;
}

extern "C" uint32_t tbls_shard_min(void) { return shard_min(); }
extern "C" uint32_t tbls_shard_knee(void) { return shard_knee(); }

extern "C" int tbls_acc_plan(uint32_t n, uint32_t* per, uint32_t* nseg, int* split) {
  const pair_plan pp(n);
  if (per) *per = pp.per;
  if (nseg) *nseg = pp.nseg;
  if (split) *split = pp.split ? 1 : 0;
  return TBLS_SUCCESS;
}

// batched helpers for building synthetic workloads on the device
extern "C" int tbls_sk_to_pk_many(const uint8_t* sks, size_t n, uint8_t* out) {
  return with_device([&](dev_ctx& c) -> int {
    std::vector<uint64_t> w(4 * n);
    for (size_t i = 0; i < n; i++) sk_to_words(sks + 32 * i, &w[4 * i]);
    upload u;
    size_t o = u.add(w.data(), 32 * n);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(48 * n + 256)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_sk_to_pk, dim3((n + TB_BLOCK - 1) / TB_BLOCK), dim3(TB_BLOCK), 0, c.stream, (const uint64_t*)(d + o), (uint32_t)n,
                       c.ws.as<uint8_t>(0));
    return fetch(c, out, c.ws.p, 48 * n);
  });
}

extern "C" int tbls_sign_many(const uint8_t* sks, const uint8_t* msgs, const uint32_t* msg_off, size_t n, const uint8_t* dst, size_t dlen,
                              uint8_t* out) {
  if (dlen > 255) return TBLS_BAD_ARGUMENT;
  return with_device([&](dev_ctx& c) -> int {
    std::vector<uint64_t> w(4 * n);
    for (size_t i = 0; i < n; i++) sk_to_words(sks + 32 * i, &w[4 * i]);
    upload u;
    size_t ok_ = u.add(w.data(), 32 * n), om = u.add(msgs, msg_off[n]), oo = u.add(msg_off, 4 * (n + 1)), od = u.add(dst, dlen);
    uint8_t* d;
    int rc = stage_in(c, u, &d);
    if (rc) return rc;
    if (c.ws.ensure(96 * n + 256)) return (int)TBLS_DEVICE_ERROR;
    hipLaunchKernelGGL(k_sign, dim3((n + TB_BLOCK - 1) / TB_BLOCK), dim3(TB_BLOCK), 0, c.stream, (const uint64_t*)(d + ok_), d + om,
                       (const uint32_t*)(d + oo), d + od, (uint32_t)dlen, (uint32_t)n, c.ws.as<uint8_t>(0));
    return fetch(c, out, c.ws.p, 96 * n);
  });
}

// Asynchronous final verification (pipelined services): the product of the
// records and the final exponentiation queued on `s`, the verdict written to
// device memory.  k_final_verify_recs reads the records in place and writes
// only *ok_dev, so the call owns no device scratch: any number of calls may be
// in flight on any streams (round 2 kept the records' Fp12 copies and the
// invalid count in one per-device scratch buffer that two finals on different
// streams overwrote -- see DESIGN.md, "Asynchronous final verification").
int launch_final_async(const void* recs, uint32_t g, hipStream_t s, int* ok_dev) {
  tb_launch_final_recs((const uint8_t*)recs, g, s, ok_dev);
  HIPCHK(hipGetLastError());
  return TBLS_SUCCESS;
}

extern "C" int tbls_dev_final_verify_async(int device, const void* partials, uint32_t g, void* stream, int* ok_dev) {
  if (!partials || !ok_dev || g == 0) return TBLS_BAD_ARGUMENT;
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  dev_ctx* c = ctx_for(device);
  if (!c) return TBLS_DEVICE_ERROR;
  const caller_device keep;
  HIPCHK(hipSetDevice(c->dev));  // no device state is touched: no lock needed
  return launch_final_async(partials, g, stream ? (hipStream_t)stream : c->stream, ok_dev);
}

extern "C" int tbls_dev_final_verify(int device, const void* partials, uint32_t g, void* stream, int* ok) {
  if (ensure_init()) return TBLS_DEVICE_ERROR;
  dev_ctx* c = ctx_for(device);
  if (!c) return TBLS_DEVICE_ERROR;
  std::lock_guard<std::mutex> lk(c->mu);
  const caller_device keep;
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return launch_final(*c, partials, g, s, ok);
}
