// The batch plan: every host-side decision of the partial pipeline -- which
// kernel each stage runs, how the pairs are split over the Miller kernels,
// the product-tree schedule, the workspace layout and the placement of a
// batch on the devices -- as plain host code.  No HIP: tests/native/plan_check.cpp
// compiles this header with g++ and checks the plan on the CPU; tb_lib.hip
// builds one batch_plan per launch_partial call and launches from it.  Not
// included by any kernel translation unit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tb_curve.h"  // sizes of the workspace's point and field types

namespace tb {
namespace plan {

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Sizes of device types whose headers declare kernels (pinned by
// static_assert in tb_lib.hip).
constexpr size_t LINE_BYTES_PER_PAIR = 68u * 288u;  // TB_LINE_BYTES_PER_PAIR, tb_kdecl.h
constexpr size_t HROW_SET_BYTES = 864;              // sizeof(hrow_set), tb_hrow.h

// ---------------------------------------------------------------------------
// Tuning constants
// ---------------------------------------------------------------------------
// Placement (place_plan below): the shard size floor, and the floor on an idle node
#define TB_SHARD_MIN 32768u
#define TB_SHARD_KNEE 4096u
// Fp12 product levels: each wave multiplies TB_PROD_CHUNK values (k_fp12_prod_wave)
#define TB_PROD_CHUNK 16u
// From this many sets on, the signature side of the batch equation is a
// bucket sum by randomizer byte with 2040 bucket pairs (k_msm_*, k_sigs.hip);
// below it, one signature pair (-[r_i] g1, sig_i) per set.
// (Round 4: 32,768 -> 20,480 sets.  24,576-set batches gain -- device partial
// 13.65 -> 11.63 ms, host-API p50 15.7 -> 12.8 -- but at 12,288 and 16,384
// sets the host-API p50 turns bimodal, 9.6 -> 12.4 ms (best runs 9.1; most
// likely the bucket-sum kernels still resident when the one-round quad line
// kernel launches push some of its waves into a second round); profiles/r04_stage_msm_min.json,
// r04_cfg4_msm_ab.json.)  TBLS_MSM_MIN overrides (tuning).
#define TB_MSM_MIN 20480u
#define TB_HASH_WAVE_MAX 512u  // k_set_hash_wave (one workgroup per set) up to this many sets: at 1024 its waves fill every SIMD and the key / signature stages can no longer run beside it (measured 9.8 vs 8.8 ms partial)
#define TB_MSM_BUCKETS 2048u  // 8 windows x 256 digits (digit 0 unused)
#define TB_MSM_NSUM 2040u     // 8 x 255 bucket sums
#define TB_MSM_TREE_WG (TB_MSM_NSUM / 2u)  // k_msm_bucket_tree workgroups: two buckets of 32 lanes each (k_sigs.hip)
#define TB_MSM_XPAIRS 64u     // 8 windows x 8 digit bits: the signature side's pairs
// Split Miller loop (k_miller_lines + k_miller_acc*, k_lines.hip): pairs per
// line-buffer chunk (19,584 B of lines per pair: 5.1 GB per chunk), and the
// pair count from which two pairs share an accumulator (the GPU is full at one
// accumulator wave per SIMD: 1024 waves x 64 lanes x 2 pairs).
#define TB_LINE_CHUNK 262144u
#define TB_MILLER_PER2_MIN 131072u
// up to this many pairs, one pair per 64-lane workgroup (k_miller_wave);
// TBLS_MILLER_WAVE_MAX overrides (tuning).  (Round 6 measured the level
// program on 16 coop rows, k_miller_coop: one pair's loop 1.00 ms against
// the wave kernel's 0.84 at 128 sets, profiles/r06_latency_128_coop_vs_wave.json;
// not kept.)
#define TB_MILLER_WAVE_MAX 2048u
// Segmented accumulator (acc_plan below)
#define TB_ACC_FULL 65536u
#define TB_ACC_PER_MAX 16  // 32 x 16 measured slower than 16 x 8 at 131,072 pairs (13.9 vs 13.3 ms Miller stage)
#define TB_ACC_NSEG_MAX 16
// hash_to_G2 kernel by batch size (hash_kind below)
#define TB_HASH_ROW_MAX 1024u  // above, the quads win (4,096 sets: partial 6.98 -> 5.81 ms, profiles/r04_stage_row_vs_quad.json)
#define TB_HASH_QUAD_MAX 8192u
#define TB_HASH_DUO_MAX 32768u
#define TB_GROUP_LANES 65536u  // one wave per SIMD
// Values per wave of the unsegmented product levels (k_fp12_prod_wave): a
// wave multiplies its chunk one value after another, so small batches (the
// latency path) take 4 (256 pairs: 4 levels of 3 products, against 2 levels
// of 15 with 16); larger unsegmented batches keep TB_PROD_CHUNK.
#ifndef TB_PROD_SMALL_MAX
#define TB_PROD_SMALL_MAX 4096u
#endif
// The large-batch one-lane kernels (hash, signature check, [r] apk) as their
// two-waves-per-SIMD twins (k_w2_*.hip) from TB_W2_MIN sets, where each
// stage fills the GPU alone (throughput); TBLS_W2=0 selects the one-wave
// kernels (A/B).  Below it the stages run side by side and each is a
// latency chain: the one-wave kernels spill less, and a wave that holds the
// whole register file keeps its SIMD to itself instead of sharing it with
// another stage's two-wave waves (profiles/r04_stage16k_*).  (The Miller
// line and accumulator kernels measured slower at two waves -- 17.5 and 24.3
// vs 14.5 ms Miller stage at 131,072 sets, profiles/r04_bench_w2_masks.json
// -- and stay at one.)
#define TB_W2_MIN 32768u
// Grouped batches (tb_group.h, k_kcoop.hip): sets that sign the same message
// share one main pair.  The host entries group a batch of n sets with m
// distinct messages when n >= group_min and 100 m <= percent n
// (group_pays below); TBLS_GROUP_MIN = "min[,percent]" overrides (tuning).
// Measured with tools/bench_grouped.py on device-resident batches
// (profiles/grouped.json; ungrouped / grouped p50 of partial + final, ms):
//   n = 128     m = n/64 2.74 / 5.13    m = n/2 2.74 / 5.12   the bucket-sum chain's fixed cost
//   n = 512              5.36 / 5.26            5.37 / 5.31   parity
//   n = 2,048            5.93 / 5.41            5.89 / 6.20
//   n = 8,192            6.99 / 5.61            6.88 / 7.52
//   n = 16,384  m = 64   8.91 / 6.40   m = 2,048 (n/8) 8.84 / 6.92
//   n = 131,072 m = 64  35.01 / 14.03  m = 2,048 (n/64) 35.38 / 15.46
// So grouping pays from 2,048 sets at m = n / 64 and loses at m = n / 2 at
// every size of the sweep: the thresholds are the measured winning corner,
// 2,048 sets and 2 percent (n / 64 is 1.56 percent).  Ratios between n / 64
// and n / 2 are measured at 16,384 sets only (n / 8 wins there); the percent
// can rise once they are measured at the small sizes too.
#define TB_GROUP_MIN 2048u
#define TB_GROUP_PERCENT 2u
// k_group_pk_sum_coop: rows per workgroup, and the members one row walks at
// least before a group is split over several workgroups (group_walk below)
#define TB_GROUP_ROWS 32u
#define TB_GROUP_WALK_MIN 8u
#define TB_GROUP_CHIP_ROWS (256u * TB_GROUP_ROWS)  // one 512-thread workgroup per compute unit
// Settling a failed batch (tb_lib.hip settle_sets)
#define TB_SETTLE_FAN 16u                  // sets per group and groups per group of the next level (k_fp12_prod_wave_seg chunk)
#define TB_SETTLE_MAX (TB_LINE_CHUNK / 2u)  // sets per settle chunk: both pairs of every set in one line chunk

// ---------------------------------------------------------------------------
// Every environment override of the plan, parsed once per process (get()).
// Everything below takes a `const plan_env&`, so a CPU check can sweep
// overrides in one process.
// ---------------------------------------------------------------------------
struct plan_env {
  uint32_t msm_min = TB_MSM_MIN;                  // TBLS_MSM_MIN (tuning)
  uint32_t miller_wave_max = TB_MILLER_WAVE_MAX;  // TBLS_MILLER_WAVE_MAX (tuning)
  // TBLS_ACC_PLAN: -1 / -1 (unset), 0 / 0 ("0": unsegmented), or per / nseg
  int acc_per = -1, acc_seg = -1;
  // TBLS_HASH_PLAN = "row_max,quad_max,duo_max" (A/B; 0 disables a kernel)
  uint32_t row_max = TB_HASH_ROW_MAX, quad_max = TB_HASH_QUAD_MAX, duo_max = TB_HASH_DUO_MAX;
  bool w2 = true;  // TBLS_W2=0: the one-wave kernels at every size
  uint32_t w2_min = TB_W2_MIN;  // TBLS_W2_MIN: the two-wave kernels from this many sets (tuning; tests reach them at a few hundred sets)
  // Small batches (<= TB_HASH_WAVE_MAX sets) run the key, signature and hash
  // stages, and multi-key aggregation, on the lane-cooperative kernels
  // (k_kcoop.hip, k_hwave.hip k_set_hash_coop); TBLS_COOP=0 selects the
  // one-thread / one-wave kernels they replaced (A/B, fall-back).
  bool coop = true;
  // TBLS_SHARD_MIN = "min[,knee]" (min 0: every allowed idle device)
  uint32_t shard_min = TB_SHARD_MIN, shard_knee = TB_SHARD_KNEE;
  // TBLS_GROUP_MIN = "min[,percent]": the host entries' grouping thresholds
  uint32_t group_min = TB_GROUP_MIN, group_percent = TB_GROUP_PERCENT;
  // TBLS_GSETTLE_CHUNK: positions per chunk of settling a grouped batch (gsettle_layout; tuning)
  uint32_t gsettle_chunk = TB_SETTLE_MAX;

  // one parser per variable; v: the variable's value, nullptr when unset
  void parse_msm_min(const char* v) {
    if (v) msm_min = (uint32_t)atoi(v);
  }
  void parse_miller_wave_max(const char* v) {
    if (v) miller_wave_max = (uint32_t)atoi(v);
  }
  void parse_acc_plan(const char* v) {
    acc_per = acc_seg = -1;
    if (!v) return;
    if (v[0] == '0' && v[1] == 0) {
      acc_per = acc_seg = 0;
      return;
    }
    int p = 0, g = 0;
    if (sscanf(v, "%d,%d", &p, &g) == 2 && p >= 1 && p <= 32 && (p & (p - 1)) == 0 && g >= 1 && g <= TB_ACC_NSEG_MAX) {  // per <= 32: one mask bit per pair
      acc_per = p;
      acc_seg = g;
    }
  }
  void parse_hash_plan(const char* v) {
    unsigned r, q, d;
    if (v && sscanf(v, "%u,%u,%u", &r, &q, &d) == 3) {
      row_max = r;
      quad_max = q;
      duo_max = d;
    }
  }
  void parse_w2(const char* v) { w2 = !(v && v[0] == '0'); }
  void parse_w2_min(const char* v) {
    if (!v) return;
    const long m = atol(v);
    if (m >= 1) w2_min = (uint32_t)std::min<long>(m, 0x7fffffffL);
  }
  void parse_coop(const char* v) { coop = !(v && v[0] == '0'); }
  void parse_shard_min(const char* v) {
    if (!v) return;
    unsigned a = 0, b = 0;
    const int k = sscanf(v, "%u,%u", &a, &b);
    if (k >= 1) shard_min = a;
    shard_knee = k == 2 ? b : std::min(shard_min, (uint32_t)TB_SHARD_KNEE);
  }

  void parse_group_min(const char* v) {
    if (!v) return;
    unsigned a = 0, b = 0;
    const int k = sscanf(v, "%u,%u", &a, &b);
    if (k >= 1) group_min = a;
    if (k == 2 && b <= 100) group_percent = b;
  }

  void parse_gsettle_chunk(const char* v) {
    if (!v) return;
    const long c = atol(v);
    if (c >= 1 && c <= (long)TB_LINE_CHUNK) gsettle_chunk = (uint32_t)c;
  }

  static plan_env from_environment() {
    plan_env e;
    e.parse_msm_min(getenv("TBLS_MSM_MIN"));
    e.parse_miller_wave_max(getenv("TBLS_MILLER_WAVE_MAX"));
    e.parse_acc_plan(getenv("TBLS_ACC_PLAN"));
    e.parse_hash_plan(getenv("TBLS_HASH_PLAN"));
    e.parse_w2(getenv("TBLS_W2"));
    e.parse_w2_min(getenv("TBLS_W2_MIN"));
    e.parse_coop(getenv("TBLS_COOP"));
    e.parse_shard_min(getenv("TBLS_SHARD_MIN"));
    e.parse_group_min(getenv("TBLS_GROUP_MIN"));
    e.parse_gsettle_chunk(getenv("TBLS_GSETTLE_CHUNK"));
    return e;
  }
  // read once, thread-safe (C++11 magic static): concurrent batch callers plan at once
  static const plan_env& get() {
    static const plan_env v = from_environment();
    return v;
  }
};

// ---------------------------------------------------------------------------
// Placement of a batch on the devices.  The reference runs
// numThreads service workers side by side, each with its own batch
// (AggregatingSignatureVerificationService.java:121-132, 202-205), so a
// device should hold one caller's batch, not a slice of every caller's:
//  * a batch is sharded only over devices that are IDLE at placement time
//    (no batch in flight), and only into shards of at least shard_min sets:
//    G = min(idle devices, n_gpus cap, floor(n / shard_min)) >= 1.
//    shard_min = 32,768 sets, where one MI355X's partial stops being a
//    latency chain (profiles/r04_stage_sweep_final.json, device partial:
//    16,384 sets 8.6 ms = 1.9 M sets/s, 32,768 sets 12.5 ms = 2.6 M/s, 65,536
//    21.8 ms = 3.0 M/s, 131,072 37.4 ms = 3.5 M/s); below it a second device
//    buys a lone batch a few ms of latency and costs every concurrent caller a
//    whole device.  So a lone 131,072-set batch runs as 4 shards of 32,768,
//    1,048,576 sets over all 8 devices, and 8 workers with 16,384-set batches
//    (config 4) take 8 different devices, one each;
//  * with no idle device the batch goes whole to the least-loaded one;
//  * among equals, ties are broken round-robin from a counter; the chosen
//    devices are taken in ascending order (lock order; the lowest is the
//    gather root);
//  * shards are contiguous and balanced by key count, as teku_amd/dist.py
//    shard_bounds.
// (Round 4 sharded any batch of 2 x 2,048 sets over the least-loaded devices
// whatever their load: a 16,384-set batch took all 8 devices and concurrent
// workers serialized on them -- about 2.5 M sigs/s for the node where one
// batch per device gives about 13.9 M)
//  * on an IDLE NODE (no batch in flight on any device) a lone batch may
//    shard further, down to the latency knee of TB_SHARD_KNEE = 4,096 sets
//    per device (the same sweep: the device partial is 5.5 ms at 1,024 sets,
//    5.8 at 4,096, 6.5 at 8,192, 8.6 at 16,384), so a lone config-4 batch of
//    16,384 sets runs as 4 shards of 4,096: modelled latency 8.6 + 0.8 (final)
//    -> 5.8 + 0.8 ms plus the record gather.  Under load the rule above
//    holds: one device per batch.  A service that knows more batches are
//    waiting passes n_gpus = 1 (teku_amd/service.py, and the Java mirror
//    HipAggregatingSignatureVerificationService), so the first of several
//    queued batches does not take the whole idle node.
// TBLS_SHARD_MIN = "min[,knee]" overrides shard_min and the knee (min 0:
// every allowed idle device).  tbls_place_plan exposes the same function for
// CPU tests.
// ---------------------------------------------------------------------------
// n sets (keys(i) keys each) over D devices with loads load[0..D): returns G
// and fills dev[0..G) (ascending) and cut[0..G] (cut[0] = 0, cut[G] = n).
// knee (0: none): the shard size floor when every device is idle.
template <class KEYS>
int place_plan(size_t n, const KEYS& keys, int D, int n_gpus, const int* load, uint32_t rr, uint32_t smin, uint32_t knee, int* dev,
               size_t* cut) {
  if (D < 1) return 0;
  const int Gmax = (n_gpus > 0 && n_gpus < D) ? n_gpus : D;
  std::vector<int> order(D);
  for (int d = 0; d < D; d++) order[d] = d;
  // least loaded first, ties round-robin from rr
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    const int la = load ? load[a] : 0, lb = load ? load[b] : 0;
    if (la != lb) return la < lb;
    return (uint32_t)(a - (int)(rr % (uint32_t)D) + D) % (uint32_t)D < (uint32_t)(b - (int)(rr % (uint32_t)D) + D) % (uint32_t)D;
  });
  int idle = 0;
  while (idle < D && (!load || load[order[idle]] == 0)) idle++;
  if (idle == D && knee && smin && knee < smin) smin = knee;  // idle node: shard down to the latency knee
  const size_t g = smin ? n / smin : (size_t)Gmax;
  int G = (int)std::min<size_t>(std::max<size_t>(g, 1), (size_t)std::min(Gmax, std::max(idle, 1)));
  if ((size_t)G > n) G = n ? (int)n : 1;
  std::sort(order.begin(), order.begin() + G);
  for (int k = 0; k < G; k++) dev[k] = order[k];
  uint64_t totalK = 0;
  for (size_t i = 0; i < n; i++) totalK += keys(i) + 1;
  for (int k = 0; k <= G; k++) cut[k] = n;
  cut[0] = 0;
  uint64_t acc = 0;
  int k = 1;
  for (size_t i = 0; i < n && k < G; i++) {
    acc += keys(i) + 1;
    while (k < G && acc * G >= totalK * (uint64_t)k) cut[k++] = i + 1;
  }
  return G;
}

// ---------------------------------------------------------------------------
// Pairs of a batch of n sets: [0, n) the sets' (r_i apk_i, H(m_i)), then the
// signature side -- n pairs (-[r_i] g1, sig_i) below TB_MSM_MIN sets (ordinary
// pairs of the Miller kernels), else TB_MSM_XPAIRS bit-sum pairs.  With the
// split Miller loop the bit-sum pairs run one 64-lane wave each (k_miller_wave,
// n_xwave of them) on the bucket-sum stream, into the Miller values after the
// accumulators'.
// Segmented accumulator (k_lines.hip k_miller_accs_lds): `per` pairs per thread,
// the loop's 68 steps in `nseg` segments.  Chosen to minimize the modelled
// accumulator time: per-thread latency (68 / nseg) (12 + 13 per) Fp2
// products (one f^2, per sparse line products per step) times the wave rounds
// (TB_ACC_FULL threads = one 64-lane wave per SIMD fill the GPU once), plus
// the Horner tail of the segment products (k_fp12_seg_combine_coop: ~63 (1 -
// 1/nseg) Fp12 squarings, about one Fp2-product latency each); ties go to
// fewer segments (smaller product tree).  TBLS_ACC_PLAN="per,nseg" overrides
// it (tuning; per and nseg powers of two up to TB_ACC_PER_MAX /
// TB_ACC_NSEG_MAX; "0" selects the unsegmented k_miller_acc1/2).  Every per
// divides TB_LINE_CHUNK, so the chunks of a large batch fill contiguous group
// ranges (lo / per).  (Round 4: per up to 16 and nseg up to 16 -- 16 x 8 at
// 131,072 pairs, 8 x 16 at config 4's 32,768 -- where round 3 stopped at 8 x 4;
// profiles/r04_bench_accplans.json.)
// ---------------------------------------------------------------------------
inline void acc_plan(uint32_t n_main, uint32_t& per, uint32_t& nseg, const plan_env& env = plan_env::get()) {
  const int e_per = env.acc_per, e_seg = env.acc_seg;
  if (e_seg == 0) {  // the unsegmented kernels
    per = n_main >= TB_MILLER_PER2_MIN ? 2u : 1u;
    nseg = 1;
    return;
  }
  double best = 0;
  per = 1;
  nseg = 1;
  for (uint32_t p = 1; p <= (uint32_t)std::max(TB_ACC_PER_MAX, e_per); p *= 2) {
    if (e_per > 0 && (int)p != e_per) continue;
    for (uint32_t sg = 1; sg <= (uint32_t)TB_ACC_NSEG_MAX; sg++) {
      if (e_seg > 0 ? (int)sg != e_seg : (sg & (sg - 1)) != 0) continue;
      const double threads = (double)sg * ((n_main + p - 1) / p);
      const double rounds = std::max(1.0, std::ceil(threads / TB_ACC_FULL));
      const double cost = rounds * (68.0 / sg) * (12.0 + 13.0 * p) + (sg > 1 ? 63.0 * (1.0 - 1.0 / sg) : 0.0);
      if (best == 0 || cost < best * 0.999) {
        best = cost;
        per = p;
        nseg = sg;
      }
    }
  }
}
//
// Grouped plan (n_msgs < n: the sets share n_msgs distinct messages): the
// pairs are [0, n_msgs) the groups' (sum_{i in g} r_i apk_i, H(m_g)), then
// always the TB_MSM_XPAIRS bit-sum pairs, whatever n is -- per-set signature
// pairs would bring back n Miller loops.  x_first() is where the signature
// side starts in the pair arrays: n, or n_msgs when grouped.
struct pair_plan {
  uint32_t n, n_msgs, n_extra, n_pairs, n_main, n_xwave, per, nseg;
  bool grouped, msm, wave, split;
  // settle: the per-set layout a failed batch is settled on (settle_sets):
  // one signature pair per set (no bucket sums), split line / accumulator
  // kernels at every size
  // n_msgs_: the distinct messages (0 or >= n: n, every set its own pair)
  explicit pair_plan(uint32_t n_, bool settle = false, const plan_env& env = plan_env::get(), uint32_t n_msgs_ = 0) : n(n_) {
    n_msgs = n_msgs_ && n_msgs_ < n && !settle ? n_msgs_ : n;
    grouped = n_msgs < n;
    msm = !settle && (grouped || n >= env.msm_min);
    n_extra = msm ? TB_MSM_XPAIRS : n;
    n_pairs = n_msgs + n_extra;
    wave = !settle && n_pairs <= env.miller_wave_max;
    split = !wave;
    n_xwave = split && msm ? n_extra : 0u;  // bit-sum pairs on their own waves
    n_main = n_pairs - n_xwave;             // pairs owned by accumulator threads
    nseg = 1;
    per = 1;
    if (split) acc_plan(std::min(n_main, TB_LINE_CHUNK), per, nseg, env);  // the chunks launch one after another: plan one chunk's fill
  }
  bool seg() const { return split && (nseg > 1 || per > 2); }  // k_miller_accs_lds
  uint32_t n_groups() const { return (n_main + per - 1) / per; }
  uint32_t n_f_main() const { return nseg * n_groups(); }
  uint32_t n_f() const { return n_f_main() + n_xwave; }  // Miller values: accumulators (segment-major), then the wave pairs'
  uint32_t line_pairs() const { return split ? std::min(n_main, TB_LINE_CHUNK) : 0u; }
  uint32_t x_first() const { return n_msgs; }  // the first signature-side pair
};

// Whether a host entry groups a batch of n sets with n_msgs distinct messages
// (tbls_group_plan): never with every message distinct; with `force` whenever
// some message repeats; else from group_min sets on, when at most
// group_percent of n messages are distinct.
inline bool group_pays(uint32_t n, uint32_t n_msgs, bool force, const plan_env& env = plan_env::get()) {
  if (!n_msgs || n_msgs >= n) return false;
  if (force) return true;
  return n >= env.group_min && 100ull * n_msgs <= (uint64_t)env.group_percent * n;
}

// tbls_group_plan: grouped 0 never, 1 under `force` only, 2 without it as well;
// n_pairs of the grouped plan when grouped is not 0, else of the ungrouped one
inline void group_plan(uint32_t n, uint32_t n_msgs, int& grouped, uint32_t& n_pairs, const plan_env& env = plan_env::get()) {
  grouped = !group_pays(n, n_msgs, true, env) ? 0 : group_pays(n, n_msgs, false, env) ? 2 : 1;
  n_pairs = pair_plan(n, false, env, grouped ? n_msgs : 0u).n_pairs;
}

// k_group_pk_sum_coop: the members one workgroup sums (TB_GROUP_ROWS rows, each
// walking its share), by counting: a batch of n sets fills the chip's rows
// once when each row walks n / TB_GROUP_CHIP_ROWS members, and a walk shorter
// than TB_GROUP_WALK_MIN additions is not worth a row tree (5 additions) and
// an inversion of its own.  A group of more members is split into items of
// this many, summed by a second pass; items(n, m) bounds their number.
inline uint32_t group_walk(uint32_t n) {
  return TB_GROUP_ROWS * std::max<uint32_t>(TB_GROUP_WALK_MIN, (n + TB_GROUP_CHIP_ROWS - 1) / TB_GROUP_CHIP_ROWS);
}
inline uint32_t group_items_max(uint32_t n, uint32_t m) { return m + n / group_walk(n); }

// segments of the per-set accumulation of settle_sets: fill the GPU once (n threads per segment)
inline uint32_t settle_nseg(uint32_t n) {
  uint32_t sg = 1;
  while (sg < 16 && 2ull * sg * n <= TB_ACC_FULL) sg *= 2;
  return sg;
}

// true when the pipeline that just ran over n sets left what settle_sets needs:
// one signature pair per set and both pairs' lines in one chunk
inline bool settle_ready(uint32_t n, const plan_env& env = plan_env::get(), uint32_t n_msgs = 0) {
  const pair_plan pp(n, false, env, n_msgs);
  return pp.split && !pp.msm && 2ull * n <= TB_LINE_CHUNK;  // a grouped plan is msm: never
}

// ---------------------------------------------------------------------------
// The plan of one launch_partial call.
// ---------------------------------------------------------------------------
// hash_to_G2 kernel by batch size.  Up to TB_HASH_WAVE_MAX sets one workgroup
// per set: the lane-cooperative k_set_hash_coop (256 threads: coop SSWU chains
// and cofactor program), or k_set_hash_wave (the cofactor clearing
// lane-parallel) with TBLS_COOP=0.  Above: one 16-lane coop row per set
// (k_hrow.hip, five launches) up to row_max sets, one DPP quad per set
// (k_hquad.hip k_set_hash_quad) up to quad_max, one lane pair per set
// (k_set_hash_duo: an SSWU map per lane, the cofactor clearing dealt over the
// pair) up to duo_max, then the one-lane k_set_hash_w2 (two waves per SIMD,
// from TB_W2_MIN sets) or k_set_hash.  The quad, duo and w2 kernels are
// followed by the exact formulas for the sets they flag (k_set_hash_fix).  A
// lane group fills the GPU at 65,536 lanes: quads at 16,384
// sets leave no SIMD to the key and signature stages beside the hash
// (profiles/r04_stage16k_quad_vs_pair.json), so quads stop at 8,192.  The
// Miller lines use the same groups while they fit one wave per SIMD: quads
// up to 16,384 pairs, pairs up to 32,768 (k_miller_lines_quad / _duo),
// unless quad_max / duo_max is 0.  TBLS_HASH_PLAN = "row_max,quad_max,duo_max"
// overrides the defaults (A/B; 0 disables a kernel).  (Round 3's pair kernel,
// the SSWU maps on two lanes and the clearing on one, was removed once the
// duo kernel replaced it: 16,384-set hash stage 5.10 -> 3.65 ms.)
enum class hash_kind { none, coop, wave, row, quad, duo, w2, lane };
// Signature stage: decode + G2 check into sig_aff / sig_use for the bucket
// sums (msm), else the set's signature pair Q[n + i] = sig_i, skip[n + i] =
// infinite / invalid: 4 sets per wave, lane-cooperative (coop), or one thread
// per set (pair).  msm and pair take their two-wave twin with batch_plan::w2.
enum class sig_kind { msm, coop, pair };
// Where a batch's keys come from, and the key stage that follows:
//  bits        bit rows over a resident committee, keys from the table: every
//              set on the lane-cooperative rows (k_set_pk_bits_coop)
//  keys_coop   as many keys as sets, up to TB_HASH_WAVE_MAX sets: one kernel,
//              decode + G1 check (wave 0) beside -[r] g1, then [r] pk (wave 1)
//              (k_keys_coop; keys as bytes or from the table).  One key per
//              set in every real batch (a set of several keys beside empty
//              ones still verifies correctly, on one lane).
//  table       k_set_pk over the resident table: no decompression
//  decompress  k_pk_decompress, then k_set_pk
enum class key_source { bytes, table, bits };
enum class key_kind { bits, keys_coop, table, decompress };

// lanes per pair of the Miller line kernel: 4, 2 or 1
inline int line_group(uint32_t n_main, const plan_env& env = plan_env::get()) {
  if (env.quad_max && 4ull * n_main <= TB_GROUP_LANES) return 4;
  if (env.duo_max && 2ull * n_main <= TB_GROUP_LANES) return 2;
  return 1;
}
inline bool use_w2(uint32_t n, const plan_env& env = plan_env::get()) { return env.w2 && n >= env.w2_min; }
// Sets of several keys (n_keys > n: configs 2/3) go to a wave-level
// aggregation after the one-thread kernel: 2 the lane-cooperative one (32
// rows per set, k_kcoop.hip, with the set's -[r] g1), 1 the one-wave-per-set
// kernel (TBLS_COOP=0), 0 every set has one key
inline uint32_t multi_key(uint32_t n, uint32_t n_keys, const plan_env& env = plan_env::get()) { return n_keys > n ? (env.coop ? 2u : 1u) : 0u; }

// One level of the Fp12 product tree: k_fp12_prod_wave over n_in values in
// chunks of `chunk` (grid n_out), or with `seg` k_fp12_prod_wave_seg per
// segment (grid n_out x nseg): n_in values per segment, n_in_last in the
// last (the bit-sum pairs' values ride with it), rows in_stride apart, the
// products out_stride apart.
enum class prod_dst { fpart, fpart2, segv, partial };
struct prod_level {
  bool seg;
  uint32_t n_in, n_in_last, in_stride, chunk, n_out, out_stride;
  prod_dst dst;
};

constexpr uint32_t HASH_ALL = 0xffffffffu;  // batch_plan's m_hash without a memo: every main pair's message is hashed

struct batch_plan {
  pair_plan pp;
  uint32_t n_keys;  // keys to decompress (0 with a table source)
  // The messages to hash.  Without the hash-point memo (tb_msgmemo.h) these
  // are the main pairs' messages, pp.n_msgs, hashed straight into Q.  With it
  // (memo): the messages the host found neither resident nor repeated, hashed
  // into Qh / skiph (ws_layout), from where k_memo_fill gives every main pair
  // its Q.  The hash kernel, the row-hash workspace and the w2 kernel's park
  // area follow this count, not pp.n_msgs.
  uint32_t n_hash;
  bool memo;
  hash_kind hash = hash_kind::none;
  sig_kind sig;
  key_kind key;
  bool w2;            // the two-wave twins of the one-lane per-set kernels
  uint32_t multi;     // multi_key(n, the batch's keys)
  int line_group;     // lanes per pair of the line kernel (0: no line kernel, the wave Miller loops)
  // Large split batches: the main pairs' line kernel needs only the signature
  // codes from the signature stream, not the bucket sums and the extra
  // pairs' Miller loops (one 64-lane launch of ~2.5 ms): it waits on e_sig,
  // and only the accumulator and the product tree wait for the whole stream.
  // (Side-by-side streams only: not with launch_partial's `serial`.)
  bool late_join;
  // Bucket-sum batches: when the hash starts.  0: at once (beside the key
  // decompression and the signature checks); 1: after the signature checks;
  // 2: after the whole bucket-sum chain.  Measured at 131,072 sets
  // (profiles/r05_bench_sig_first.json): keys as bytes 36.4-36.7 ms (0) /
  // 37.8-37.9 (1) / 38.5-38.9 (2); keys from the device table 3.61-3.65 /
  // 3.87-3.90 / 3.70-3.74 M sigs/s.  So 1 with the key table (no key
  // decompression beside the signature checks), else 0.  (The A/B switch
  // TBLS_SIG_FIRST and order 2 were removed in round 6.)
  int sig_first;
  uint32_t prod_chunk;  // values per wave of the unsegmented product levels
  // The product tree: levels of chunked wave products f -> fpart -> fpart2 ->
  // fpart ...; the last writes the partial, or with `combine` the nseg
  // segment products (segv) that the Horner combine (k_fp12_seg_combine_coop)
  // turns into the partial.  Empty for a settle plan (no product).
  prod_level levels[10];  // >= log4(TB_PROD_SMALL_MAX) and log16(2^33)
  int n_levels = 0;
  bool combine = false;

  // n_msgs (0: n): a grouped plan when below n -- the hash kind, the line
  // group, the wave / split choice, the accumulator plan and the product
  // levels follow from n_msgs messages and n_msgs + 64 pairs; the per-set
  // kernels (key stage, signature check, w2) from n.
  // m_hash (HASH_ALL: no memo): the messages to hash of a launch that resolved.
  batch_plan(uint32_t n, uint32_t n_keys_in, key_source src, bool settle = false, const plan_env& env = plan_env::get(),
             uint32_t n_msgs = 0, uint32_t m_hash = HASH_ALL)
      : pp(n, settle, env, n_msgs), n_keys(src == key_source::bytes ? n_keys_in : 0u) {
    const bool small = n <= TB_HASH_WAVE_MAX && env.coop;
    w2 = use_w2(n, env);
    memo = m_hash != HASH_ALL;
    n_hash = memo ? std::min(m_hash, pp.n_msgs) : pp.n_msgs;
    const uint32_t nh = n_hash;  // messages to hash
    if (!nh) hash = hash_kind::none;
    else if (nh <= TB_HASH_WAVE_MAX) hash = env.coop ? hash_kind::coop : hash_kind::wave;
    else if (nh <= env.row_max) hash = hash_kind::row;
    else if (nh <= env.quad_max) hash = hash_kind::quad;
    else if (nh <= env.duo_max) hash = hash_kind::duo;
    else hash = use_w2(nh, env) ? hash_kind::w2 : hash_kind::lane;
    sig = pp.msm ? sig_kind::msm : small ? sig_kind::coop : sig_kind::pair;
    key = src == key_source::bits ? key_kind::bits
          : n_keys_in == n && n && small ? key_kind::keys_coop
          : src == key_source::table ? key_kind::table
                                     : key_kind::decompress;
    multi = multi_key(n, n_keys_in, env);
    line_group = pp.split ? plan::line_group(pp.n_main, env) : 0;
    late_join = pp.msm && pp.split;
    sig_first = src == key_source::bytes ? 0 : 1;
    prod_chunk = !pp.seg() && pp.n_f() <= TB_PROD_SMALL_MAX ? 4u : TB_PROD_CHUNK;
    if (settle) return;
    int lvl = 0;
    auto scratch = [&] { return (lvl++ & 1) ? prod_dst::fpart2 : prod_dst::fpart; };
    if (pp.seg() && pp.nseg > 1) {
      // per segment, the bit-sum pairs' values with the last, to the nseg
      // segment products, then the Horner combine into the partial
      combine = true;
      uint32_t cn = pp.n_groups(), cl = pp.n_groups() + pp.n_xwave, stride = pp.n_groups();
      for (;;) {
        const uint32_t no = (cn + TB_PROD_CHUNK - 1) / TB_PROD_CHUNK, nl = (cl + TB_PROD_CHUNK - 1) / TB_PROD_CHUNK;
        if (nl == 1) {
          levels[n_levels++] = {true, cn, cl, stride, TB_PROD_CHUNK, nl, 1u, prod_dst::segv};
          break;
        }
        levels[n_levels++] = {true, cn, cl, stride, TB_PROD_CHUNK, nl, nl, scratch()};
        cn = no;
        cl = stride = nl;
      }
    } else {
      uint32_t cnt = pp.n_f() ? pp.n_f() : 1;  // no pairs at all: the product of the one value 1 (k_fp12_one)
      for (;;) {
        const uint32_t nout = (cnt + prod_chunk - 1) / prod_chunk;
        if (nout == 1) {
          levels[n_levels++] = {false, cnt, cnt, 0u, prod_chunk, nout, 0u, prod_dst::partial};
          break;
        }
        levels[n_levels++] = {false, cnt, cnt, 0u, prod_chunk, nout, 0u, scratch()};
        cnt = nout;
      }
    }
  }
};

// --------------------------------------------------------------------------
// workspace layout for one device pipeline (byte offsets into dev_ctx::ws)
// --------------------------------------------------------------------------
struct ws_layout {
  size_t pk_aff, pk_code, P, Q, skip, set_code, sig_code, f, fpart, fpart2, segv, n_bad, result;
  size_t sig_aff, sig_use, msm_cnt, msm_off, msm_cur, msm_idx, msm_sum, mlist, mcnt, lines, hrow, total;
  // Grouped plans only (empty otherwise): set_code and sig_code hold one byte
  // per SET there, and the Miller kernels read a code per PAIR from pair_code
  // (two rows of n_pairs zero bytes after sig_code; the group sums flag an
  // infinite sum in the first row).  set_P: the sets' [r_i] apk_i; grp_item,
  // grp_part, grp_pskip: k_group_pk_sum_coop's first item per group and the
  // items' partial sums with their infinity flags.
  size_t pair_code, set_P, grp_item, grp_part, grp_pskip;
  // Memo plans only (empty otherwise, after every other region, so that no
  // offset moves without a memo): the n_hash hashed points and their skip
  // bytes, which k_memo_fill and k_memo_learn copy as 16-byte words.
  size_t Qh, skiph;
  size_t code_bytes;  // set_code .. the end of the last code row: zeroed by every launch
  uint32_t nb_f;
  // A function of the plan alone: what a host launch knows beyond it (where
  // the staging image holds a grouped shard's CSR and randomizers) is in the
  // launch's own record (tb_lib.hip shard_run).
  ws_layout() : total(0) {}
  explicit ws_layout(const batch_plan& bp) {
    const pair_plan& pp = bp.pp;
    const uint32_t n = pp.n, np = pp.n_pairs, nf = pp.n_f(), K = bp.n_keys;
    const bool msm = pp.msm;
    // first product level; segmented: nseg rows of the last segment's width
    const uint32_t pc = bp.prod_chunk;
    nb_f = (nf + pc - 1) / pc + pp.nseg * ((pp.n_groups() + pp.n_xwave + TB_PROD_CHUNK - 1) / TB_PROD_CHUNK);
    size_t o = 0;
    pk_aff = o;   o = align_up(o + (size_t)K * sizeof(g1a));
    pk_code = o;  o = align_up(o + K);
    const bool grouped = pp.grouped;
    const uint32_t nc = grouped ? n : np;  // code bytes per row
    P = o;        o = align_up(o + (size_t)np * sizeof(g1a));
    Q = o;        o = align_up(o + (size_t)np * sizeof(g2a));
    skip = o;     o = align_up(o + np);
    set_code = o; o = align_up(o + nc);  // extra pairs: zero codes
    sig_code = o; o = align_up(o + nc);
    pair_code = o; o = grouped ? o + 2 * align_up(np) : o;
    code_bytes = o - set_code;
    const size_t nm = msm ? n : 0;
    sig_aff = o;  o = align_up(o + nm * sizeof(g2a));
    sig_use = o;  o = align_up(o + nm);
    msm_cnt = o;  o = align_up(o + (msm ? TB_MSM_BUCKETS * 4 : 0));
    msm_off = o;  o = align_up(o + (msm ? (TB_MSM_BUCKETS + 1) * 4 : 0));
    msm_cur = o;  o = align_up(o + (msm ? TB_MSM_BUCKETS * 4 : 0));
    msm_idx = o;  o = align_up(o + nm * 8 * 4);
    msm_sum = o;  o = align_up(o + (msm ? (size_t)TB_MSM_BUCKETS * sizeof(g2j) : 0));
    mlist = o;    o = align_up(o + (size_t)n * 4);
    mcnt = o;     o = align_up(o + 4);
    const uint32_t nh = bp.n_hash;
    hrow = o;     o = align_up(o + (bp.hash == hash_kind::row ? (size_t)nh * HROW_SET_BYTES : 0));
    // the line buffer; before the line kernel runs, k_set_hash_w2 parks the
    // chains' affine addends in it (a g2a per set)
    lines = o;    o = align_up(o + std::max((size_t)pp.line_pairs() * LINE_BYTES_PER_PAIR, bp.hash == hash_kind::w2 ? (size_t)nh * sizeof(g2a) : 0));
    f = o;        o = align_up(o + (size_t)(nf ? nf : 1) * sizeof(fp12));
    fpart = o;    o = align_up(o + (size_t)nb_f * sizeof(fp12));
    fpart2 = o;   o = align_up(o + (size_t)((nb_f + pc - 1) / pc + pp.nseg) * sizeof(fp12));
    segv = o;     o = align_up(o + (size_t)pp.nseg * sizeof(fp12));
    n_bad = o;    o = align_up(o + 4);
    result = o;   o = align_up(o + 4);
    const uint32_t ni = grouped ? group_items_max(n, pp.n_msgs) : 0u;
    set_P = o;     o = align_up(o + (grouped ? (size_t)n * sizeof(g1a) : 0));
    grp_item = o;  o = align_up(o + (grouped ? ((size_t)pp.n_msgs + 1) * 4 : 0));
    grp_part = o;  o = align_up(o + (size_t)ni * sizeof(g1a));
    grp_pskip = o; o = align_up(o + ni);
    const size_t nq = bp.memo ? bp.n_hash : 0;
    Qh = o;        o = align_up(o + nq * sizeof(g2a));
    skiph = o;     o = align_up(o + nq);
    static_assert(sizeof(g2a) % 16 == 0, "k_memo_fill copies points as 16-byte words: Q, Qh (multiples of 256) and every entry are 16-byte aligned");
    total = o;
  }
};

// workspace of the per-set pass (tb_lib.hip run_each) over n sets with K keys
// to decompress; the multi-key work list's count follows its n entries
struct each_layout {
  size_t pk_aff, pk_code, P, Q, sig_aff, skip, set_code, sig_code, sig_use, okd, n_bad, mlist, mcnt, total;
  each_layout(uint32_t n, uint32_t K) {
    size_t o = 0;
    pk_aff = o;   o = align_up(o + (size_t)K * sizeof(g1a));
    pk_code = o;  o = align_up(o + (K ? K : 1));
    P = o;        o = align_up(o + (size_t)n * sizeof(g1a));
    Q = o;        o = align_up(o + (size_t)n * sizeof(g2a));
    sig_aff = o;  o = align_up(o + (size_t)n * sizeof(g2a));
    skip = o;     o = align_up(o + n);
    set_code = o; o = align_up(o + n);
    sig_code = o; o = align_up(o + n);
    sig_use = o;  o = align_up(o + n);
    okd = o;      o = align_up(o + n);
    n_bad = o;    o = align_up(o + 4);
    mlist = o;    mcnt = o + (size_t)n * 4;  o = align_up(o + (size_t)n * 4 + 4);
    total = o;
  }
};

// scratch of settling n sets (tb_lib.hip settle_sets, settle_tail; byte
// offsets into dev_ctx::sws, from `base` on, a multiple of 256): nseg segment
// rows of the n per-set Miller values, of their nA group products
// (TB_SETTLE_FAN sets each) and of the nB products of those groups; then the
// list of groups to test (at most n words) and the tests' verdicts (a byte
// each).  total: the end of the scratch, base included.
struct settle_layout {
  uint32_t n, nseg, nA, nB;
  size_t V, A, B, list, out, total;
  explicit settle_layout(uint32_t n_, size_t base = 0) : n(n_) {
    nseg = settle_nseg(n);
    nA = (n + TB_SETTLE_FAN - 1) / TB_SETTLE_FAN;
    nB = (nA + TB_SETTLE_FAN - 1) / TB_SETTLE_FAN;
    size_t o = base;
    V = o;    o = align_up(o + (size_t)nseg * n * sizeof(fp12));
    A = o;    o = align_up(o + (size_t)nseg * nA * sizeof(fp12));
    B = o;    o = align_up(o + (size_t)nseg * nB * sizeof(fp12));
    list = o; o = align_up(o + (size_t)n * 4);
    out = o;  o = align_up(o + n);
    total = o;
  }
};

// scratch of settling a failed grouped batch of n sets over m messages
// (tb_lib.hip settle_grouped; byte offsets into dev_ctx::sws).  Positions are
// the CSR's: position t is set grp_sets[t].  mlines: the m messages' line
// tables, not evaluated at a G1 point (68 x 288 B per message, structure of
// arrays with stride m); msg_of_pos: the message of each position (a word
// each).  The signature side is built chunk by chunk, `chunk` positions at a
// time: negr, the positions' -[r] g1; sigq / sskip, their signatures and skip
// flags in position order (the line kernel's Q and skip); slines, the chunk's
// signature line tables.  tail: settle_layout(n) placed after slines, its V
// indexed by position.
struct gsettle_layout {
  uint32_t n, m, chunk, n_chunks;
  size_t mlines, msg_of_pos, negr, sigq, sskip, slines, total;
  settle_layout tail;
  gsettle_layout(uint32_t n_, uint32_t m_, const plan_env& env = plan_env::get()) : n(n_), m(m_), tail(0) {
    chunk = std::max<uint32_t>(1u, std::min(n, env.gsettle_chunk));
    n_chunks = (n + chunk - 1) / chunk;
    size_t o = 0;
    mlines = o;     o = align_up(o + (size_t)m * LINE_BYTES_PER_PAIR);
    msg_of_pos = o; o = align_up(o + (size_t)n * 4);
    negr = o;       o = align_up(o + (size_t)chunk * sizeof(g1a));
    sigq = o;       o = align_up(o + (size_t)chunk * sizeof(g2a));
    sskip = o;      o = align_up(o + chunk);
    slines = o;     o = align_up(o + (size_t)chunk * LINE_BYTES_PER_PAIR);
    tail = settle_layout(n, o);
    total = tail.total;
  }
  // chunk k covers positions [lo(k), hi(k))
  uint32_t lo(uint32_t k) const { return k * chunk; }
  uint32_t hi(uint32_t k) const { return std::min<uint64_t>(n, (uint64_t)(k + 1) * chunk); }
};

}  // namespace plan
}  // namespace tb
