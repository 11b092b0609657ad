// gfx950 kernels for the BLS12-381 verification hot path: shared declarations.
//
// Randomized batch verification (BLS.batchVerify -> BlstBLS12381
// .prepareBatchVerify/completeBatchVerify, BLS.java:275-336,
// BlstBLS12381.java:112-189) is split into per-stage kernels, one thread per
// public key / signature set / pairing:
//
//   k_pk_decompress   48-B key -> affine G1 + validity (decode, !inf, in G1)
//   k_set_pk          per set: sum keys (any invalid -> set invalid), [r]apk -> affine P_i
//   k_set_hash        per set: H(m_i) = hash_to_G2 -> affine Q_i
//   k_sig_check       per set: decode sig, G2 check
//   signature side    small batches: pair (-[r_i] g1, sig_i) per set (k_set_pk);
//                     large batches: bucket sums by randomizer byte, one pair
//                     (-(d 2^(8w)) g1, B[w][d]) per bucket (k_msm_*, k_sigs.hip)
//   k_miller_wave     per pair, one 64-lane wave (small batches)
//   k_miller_lines_w2 / _quad / _duo + k_miller_acc*   larger batches: G2 line precompute, then the Fp12 accumulation
//   k_fp12_prod_wave  F = prod f_i  (chunked wave-parallel levels; the per-GPU partial, 576 B)
//   k_final_verify    final_exp(F) == 1 && no invalid set
//
// Every thread's work is independent; reductions are two-level (block tree
// in LDS, then one block over the block partials).
#pragma once
#include <cstdlib>
#include "tb_stages.h"
#include "tb_fp12_wave.h"
#include "tb_pkindex.h"  // pkx_cache, a parameter of the key index's kernels

using namespace tb;

#define TB_BLOCK 64
// Minimum waves per SIMD the heavy one-thread-per-item kernels are compiled
// for (__launch_bounds__ second argument): 1 lets a kernel use all 512
// registers per lane; 2 caps it at 256 (the compiler spills the rest) so two
// waves share each SIMD and hide each other's latency.  Build variants for
// A/B: tools/build_variant.py.
#ifndef TB_MIN_WAVES
#define TB_MIN_WAVES 1
#endif

// Latency-bound kernels (G2 sum, the single Miller loop, Fp12 products, the
// final exponentiation) run underneath throughput kernels that fill every
// SIMD; top wave priority lets their few waves win instruction arbitration.
__device__ TB_INLINE void tb_latency_prio() { __builtin_amdgcn_s_setprio(3); }

// [k]P for a 256-bit scalar (4 little-endian u64 words), MSB first
template <typename F>
__device__ TB_INLINE jac<F> jac_mul_u256(const jac<F>& P, const uint64_t* k) {
  jac<F> r = jac_inf<F>();
  for (int w = 3; w >= 0; --w) {
    uint64_t kw = k[w];
    TB_NOUNROLL for (int b = 63; b >= 0; --b) {
      r = jac_dbl_i(r);
      if ((kw >> b) & 1) r = jac_add_i(r, P);
    }
  }
  return r;
}

// Kernel declarations (definitions in the k_*.hip translation units), for the
// host code in tb_lib.hip.  Every defining file includes this header, so a
// definition whose parameters differ from its prototype does not compile.
extern "C" __global__ void k_pk_decompress(const uint8_t* __restrict__ pks, uint32_t K, g1a* __restrict__ pk_aff, uint8_t* __restrict__ pk_code);
extern "C" __global__ void k_set_pk(const uint32_t* __restrict__ pk_off, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code, const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad, const uint32_t* __restrict__ key_idx, uint32_t tab_n, uint32_t multi_wave, g1a* __restrict__ P2, const g1a* __restrict__ comb);
extern "C" __global__ void k_multi_list(const uint32_t* __restrict__ pk_off, uint32_t n, uint32_t* __restrict__ list, uint32_t* __restrict__ cnt);
extern "C" __global__ void k_set_pk_wave(const uint32_t* __restrict__ pk_off, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code, const uint64_t* __restrict__ rand, const uint32_t* __restrict__ list, const uint32_t* __restrict__ cnt, g1a* __restrict__ P, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad, const uint32_t* __restrict__ key_idx, uint32_t tab_n);
extern "C" __global__ void k_set_pk_agg_coop(const uint32_t* __restrict__ pk_off, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code, const uint64_t* __restrict__ rand, const uint32_t* __restrict__ list, const uint32_t* __restrict__ cnt, g1a* __restrict__ P, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad, const uint32_t* __restrict__ key_idx, uint32_t tab_n, g1a* __restrict__ P2, const g1a* __restrict__ comb, uint32_t unit_r);  // k_kcoop.hip
extern "C" __global__ void k_aggregate_pks(const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code, uint32_t K, uint8_t* __restrict__ out);
extern "C" __global__ void k_sk_to_pk(const uint64_t* __restrict__ sks, uint32_t n, uint8_t* __restrict__ out);
extern "C" __global__ void k_g1_comb_init(g1a* __restrict__ comb);
extern "C" __global__ void k_sig_check(const uint8_t* __restrict__ sigs, uint32_t n, g2a* __restrict__ sig_aff, uint8_t* __restrict__ sig_use, uint8_t* __restrict__ sig_code, uint32_t* __restrict__ n_bad, uint32_t skip_mode);
extern "C" __global__ void k_msm_bitsum_pairs(const g2j* __restrict__ bucket, const g1a* __restrict__ comb, g1a* __restrict__ P, g2a* __restrict__ Q, uint8_t* __restrict__ skip);
extern "C" __global__ void k_msm_hist(const uint64_t* __restrict__ rand, uint32_t n, uint32_t* __restrict__ cnt);
extern "C" __global__ void k_msm_scan(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off, uint32_t* __restrict__ cur);
extern "C" __global__ void k_msm_scatter(const uint64_t* __restrict__ rand, uint32_t n, uint32_t* __restrict__ cur, uint32_t* __restrict__ idx);
extern "C" __global__ void k_aggregate_sigs(const uint8_t* __restrict__ sigs, uint32_t K, uint8_t* __restrict__ out, int* __restrict__ status);
extern "C" __global__ void k_sig_validate(const uint8_t* __restrict__ sigs, uint32_t n, uint32_t* __restrict__ out);
extern "C" __global__ void k_set_hash(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, g2a* __restrict__ Q, uint8_t* __restrict__ skip);
// two-waves-per-SIMD twins of the large-batch per-set kernels (k_w2_*.hip) and
// the exact recomputation of the hash sets k_set_hash_w2 flags (k_hash.hip)
extern "C" __global__ void k_set_hash_w2(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, g2a* __restrict__ Q, uint8_t* __restrict__ skip, g2a* __restrict__ park);
extern "C" __global__ void k_set_hash_fix(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, g2a* __restrict__ Q, uint8_t* __restrict__ skip);
extern "C" __global__ void k_sig_check_w2(const uint8_t* __restrict__ sigs, uint32_t n, g2a* __restrict__ sig_aff, uint8_t* __restrict__ sig_use, uint8_t* __restrict__ sig_code, uint32_t* __restrict__ n_bad, uint32_t skip_mode);
extern "C" __global__ void k_set_pk_w2(const uint32_t* __restrict__ pk_off, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code, const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad, const uint32_t* __restrict__ key_idx, uint32_t tab_n, uint32_t multi_wave, g1a* __restrict__ P2, const g1a* __restrict__ comb);
extern "C" __global__ void k_aggregate_sigs_many(const uint8_t* __restrict__ sigs, const uint32_t* __restrict__ off, uint8_t* __restrict__ out, int* __restrict__ status);
extern "C" __global__ void k_verify_each(const g1a* __restrict__ P, const g2a* __restrict__ Q, const uint8_t* __restrict__ skip, const uint8_t* __restrict__ set_code, const g2a* __restrict__ sig_aff, const uint8_t* __restrict__ sig_use, const uint8_t* __restrict__ sig_code, uint32_t n, uint8_t* __restrict__ ok);
extern "C" __global__ void k_hash_to_g2(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, uint8_t* __restrict__ out);
extern "C" __global__ void k_sign(const uint64_t* __restrict__ sks, const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, uint8_t* __restrict__ out);
extern "C" __global__ void k_miller_acc1(const uint4* __restrict__ lines, const uint8_t* __restrict__ skip, const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, uint32_t n, fp12* __restrict__ f);
extern "C" __global__ void k_miller_acc2(const uint4* __restrict__ lines, const uint8_t* __restrict__ skip, const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, uint32_t n, fp12* __restrict__ f);
extern "C" __global__ void k_fp12_prod_wave_seg(const fp12* __restrict__ in, uint32_t n, uint32_t n_last, uint32_t nseg, uint32_t in_stride, uint32_t chunk, fp12* __restrict__ out, uint32_t out_stride);
extern "C" __global__ void k_fp12_seg_combine_coop(const fp12* __restrict__ vals, uint32_t nseg, uint32_t dpack, fp12* __restrict__ out);
#define TB_LINE_BYTES_PER_PAIR (68u * 288u)  // k_miller_lines output per pair
extern "C" __global__ void k_miller_wave(const g1a* __restrict__ P, const g2a* __restrict__ Q, const uint8_t* __restrict__ skip, const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, uint32_t n, fp12* __restrict__ f);
extern "C" __global__ void k_fp12_one(fp12* __restrict__ f);
extern "C" __global__ void k_fp12_prod_wave(const fp12* __restrict__ in, uint32_t n, uint32_t chunk, fp12* __restrict__ out);
extern "C" __global__ void k_final_verify_wave(const fp12* __restrict__ f, uint32_t g, const uint32_t* __restrict__ n_bad, int* __restrict__ result);
extern "C" __global__ void k_final_verify(const fp12* __restrict__ f, const uint32_t* __restrict__ n_bad, int* __restrict__ result);
#define TB_PARTIAL_BYTES 580u  // one device's partial record (= TBLS_PARTIAL_BYTES, include/tekubls.h)
extern "C" __global__ void k_final_verify_recs(const uint8_t* __restrict__ recs, uint32_t g, int* __restrict__ result);
// lane-cooperative forms (tb_cfe.h), 256 threads: the default final exponentiation
#define TB_CFE_THREADS 256
extern "C" __global__ void k_final_verify_recs_coop(const uint8_t* __restrict__ recs, uint32_t g, int* __restrict__ result);
extern "C" __global__ void k_final_verify_coop(const fp12* __restrict__ f, uint32_t g, const uint32_t* __restrict__ n_bad, int* __restrict__ result);
// TBLS_COOP=0 selects the one-wave final exponentiation too (A/B, fall-back)
inline bool tb_final_coop() {
  static const bool v = !(getenv("TBLS_COOP") && getenv("TBLS_COOP")[0] == '0');
  return v;
}
// the final verification of g partial records on stream s (*result in device memory)
inline void tb_launch_final_recs(const uint8_t* recs, uint32_t g, hipStream_t s, int* result) {
  if (tb_final_coop())
    hipLaunchKernelGGL(k_final_verify_recs_coop, dim3(1), dim3(TB_CFE_THREADS), 0, s, recs, g, result);
  else
    hipLaunchKernelGGL(k_final_verify_recs, dim3(1), dim3(64), 0, s, recs, g, result);
}
// resident committees (k_kcoop.hip): the bad-member mask, and [r] apk of sets given as participation bit rows
extern "C" __global__ void k_committee_mask(const uint32_t* __restrict__ members, uint32_t size, const uint8_t* __restrict__ tab_code, uint32_t tab_n, uint32_t* __restrict__ bad, uint32_t* __restrict__ valid);
extern "C" __global__ void k_set_pk_bits_coop(const uint32_t* __restrict__ rows, uint32_t stride_w, const uint32_t* __restrict__ members, uint32_t size, const uint32_t* __restrict__ bad, const g1a* __restrict__ csum, uint32_t sum_ok, const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, uint32_t tab_n, const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad, g1a* __restrict__ P2, const g1a* __restrict__ comb, uint32_t unit_r);
// grouped batches (k_kcoop.hip): the items of the groups (tb_plan.h group_walk), and the per-group sums of the sets' [r] apk
extern "C" __global__ void k_group_items(const uint32_t* __restrict__ grp_off, uint32_t m, uint32_t n, uint32_t walk, uint32_t* __restrict__ item_first);
extern "C" __global__ void k_group_pk_sum_coop(const g1a* __restrict__ pts, const uint8_t* __restrict__ code, uint32_t n, const uint32_t* __restrict__ grp_off, const uint32_t* __restrict__ grp_sets, const uint32_t* __restrict__ item_first, uint32_t m, uint32_t walk, uint32_t items_max, uint32_t pass, g1a* __restrict__ PG, uint8_t* __restrict__ pskip, g1a* __restrict__ part, uint8_t* __restrict__ part_skip);
// k_lines.hip: the segmented accumulator with f in LDS and two lines per
// product (tb_lines.h miller_accs_lds_body).  Measured at 131,072 sets
// (profiles/r05_bench_acc_lds_ab.json): Miller stage alone 13.3 -> 12.6 ms
// and scratch writes 3.3 -> 1.5 GB per launch.  Its grid is one round of
// workgroups at full LDS (4 x 36,864 B per CU), so a workgroup of the
// bucket-sum stream still resident on a CU pushes part of it into a second
// round: beside that stream the 131k step went 38.2 -> 43.9 ms.  So the
// bucket sums run on a high-priority stream (the signature stream, created
// at the hash stream's priority in tbls_init) and the accumulator waits for
// that stream: with both, the LDS kernel runs at every batch size -- 131k
// step 37.3 -> 36.1-36.6 ms (profiles/r05_bench_prio_join.json; the two
// were A/B switches in round 5, TBLS_SIG_PRIO / TBLS_ACC_JOIN).  Round 6
// removed the register-resident k_miller_accs and its TBLS_ACC_LDS switch.
extern "C" __global__ void k_miller_accs_lds(const uint4* __restrict__ lines, const uint8_t* __restrict__ skip, const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, uint32_t n, uint32_t per, uint32_t nseg, uint32_t g_pad, fp12* __restrict__ f_out, uint32_t seg_stride);
extern "C" __global__ void k_msm_bucket_tree(const g2a* __restrict__ sig_aff, const uint8_t* __restrict__ use, const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx, g2j* __restrict__ bucket);  // k_sigs.hip
// one workgroup per set (k_hwave.hip): the cofactor clearing lane-parallel, and the lane-cooperative form (256 threads)
extern "C" __global__ void k_set_hash_wave(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, g2a* __restrict__ Q, uint8_t* __restrict__ skip);
extern "C" __global__ void k_set_hash_coop(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, g2a* __restrict__ Q, uint8_t* __restrict__ skip, const uint64_t* __restrict__ rand);
// the small batches' key and signature stages, lane-cooperative (k_kcoop.hip)
extern "C" __global__ void k_keys_coop(const uint8_t* __restrict__ pks, const uint32_t* __restrict__ pk_off, const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, const uint32_t* __restrict__ key_idx, uint32_t tab_n, const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, g1a* __restrict__ P2, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad, const g1a* __restrict__ comb);
extern "C" __global__ void k_sig_check_coop(const uint8_t* __restrict__ sigs, uint32_t n, g2a* __restrict__ sig_aff, uint8_t* __restrict__ sig_use, uint8_t* __restrict__ sig_code, uint32_t* __restrict__ n_bad);
// the key table's index over its key bytes (k_pkindex.hip; workgroups of its TB_PKX_BLOCK threads)
extern "C" __global__ void k_pkx_build(const uint32_t* __restrict__ keys, uint32_t K, uint32_t* slots, uint32_t mask, uint64_t seed);
extern "C" __global__ void k_pk_lookup(const uint8_t* __restrict__ pks, uint32_t K, uint32_t align, const uint32_t* __restrict__ slots, uint32_t mask, uint64_t seed, const uint32_t* __restrict__ tab_keys, const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, pkx_cache cache, g1a* __restrict__ pk_aff, uint8_t* __restrict__ pk_code, uint32_t* __restrict__ miss, unsigned long long* __restrict__ stat);
extern "C" __global__ void k_pk_decompress_list(const uint8_t* __restrict__ pks, const uint32_t* __restrict__ list, g1a* __restrict__ pk_aff, uint8_t* __restrict__ pk_code, uint32_t* __restrict__ seen);
extern "C" __global__ void k_pk_learn(const uint8_t* __restrict__ pks, uint32_t align, const uint32_t* __restrict__ list, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code, pkx_cache cache);
// the per-key comb rows (tb_pkcomb.h): the lookup that also writes the keys' reference words, the learn kernel that
// also builds the learned rows' combs, the table's build (k_pkindex.hip; the builders run TB_PKCOMB_BLOCK threads), and
// k_set_pk_w2 reading the rows (k_w2_pk.hip)
#define TB_PKCOMB_BLOCK 64
extern "C" __global__ void k_pk_lookup_ref(const uint8_t* __restrict__ pks, uint32_t K, uint32_t align, const uint32_t* __restrict__ slots, uint32_t mask, uint64_t seed, const uint32_t* __restrict__ tab_keys, const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, pkx_cache cache, g1a* __restrict__ pk_aff, uint8_t* __restrict__ pk_code, uint32_t* __restrict__ miss, unsigned long long* __restrict__ stat, uint32_t* __restrict__ pk_ref, const uint8_t* __restrict__ cache_ready, uint32_t comb_cap, uint32_t tab_comb_on);
extern "C" __global__ void k_pk_learn_comb(const uint8_t* __restrict__ pks, uint32_t align, const uint32_t* __restrict__ list, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code, pkx_cache cache, g1a* __restrict__ cache_comb, uint8_t* __restrict__ cache_ready, uint32_t comb_cap, unsigned long long* __restrict__ comb_stat);
extern "C" __global__ void k_pk_comb_build(const g1a* __restrict__ tab_aff, const uint8_t* __restrict__ tab_code, uint32_t K, g1a* __restrict__ tab_comb, unsigned long long* __restrict__ comb_stat);
extern "C" __global__ void k_set_pk_comb_w2(const uint32_t* __restrict__ pk_off, const g1a* __restrict__ pk_aff, const uint8_t* __restrict__ pk_code, const uint64_t* __restrict__ rand, uint32_t n, g1a* __restrict__ P, uint8_t* __restrict__ set_code, uint32_t* __restrict__ n_bad, const uint32_t* __restrict__ key_idx, uint32_t tab_n, uint32_t multi_wave, g1a* __restrict__ P2, const g1a* __restrict__ comb, const uint32_t* __restrict__ pk_ref, const g1a* __restrict__ cache_comb, const g1a* __restrict__ tab_comb, unsigned long long* __restrict__ comb_stat);
extern "C" __global__ void k_pk_resolve(const uint8_t* __restrict__ pks, uint32_t n, uint32_t align, const uint32_t* __restrict__ slots, uint32_t mask, uint64_t seed, const uint32_t* __restrict__ tab_keys, uint32_t* __restrict__ idx_out);
// the hash-point memo (k_msgmemo.hip; workgroups of TB_MEMO_BLOCK threads, TB_MEMO_CHUNKS threads per point): the words of
// src and learn as tb_msgmemo.h spells them (pinned by static_assert in tb_lib.hip)
#define TB_MEMO_BLOCK 256u
#define TB_MEMO_CHUNKS 12u
#define TB_MEMO_SRC_ROW 0x80000000u
#define TB_MEMO_NONE 0xffffffffu
extern "C" __global__ void k_memo_fill(const uint32_t* __restrict__ src, const uint32_t* __restrict__ set_grp, uint32_t n_pairs, const g2a* __restrict__ Qh, const uint8_t* __restrict__ skiph, const g2a* __restrict__ rows, const uint8_t* __restrict__ row_skip, g2a* __restrict__ Q, uint8_t* __restrict__ skip);
extern "C" __global__ void k_memo_learn(const uint32_t* __restrict__ learn, uint32_t m_hash, const g2a* __restrict__ Qh, const uint8_t* __restrict__ skiph, g2a* __restrict__ rows, uint8_t* __restrict__ row_skip);
// settling a failed batch (k_pair.hip; tb_lib.hip settle_sets)
extern "C" __global__ void k_group_test_coop(const fp12* __restrict__ vals, uint32_t stride, uint32_t nseg, const uint32_t* __restrict__ list, uint8_t* __restrict__ out);
extern "C" __global__ void k_settle_mask(const uint8_t* __restrict__ set_code, uint32_t n, uint8_t* __restrict__ skip);
// settling a failed grouped batch (k_gsettle.hip; tb_lib.hip settle_grouped): the messages' unevaluated line tables, the
// signature pairs in CSR position order, and the accumulator over both (line 1 scaled by the set's [r] apk on load)
extern "C" __global__ void k_gsettle_msg_lines(const g2a* __restrict__ Q, const uint8_t* __restrict__ skip, uint32_t m, uint4* __restrict__ lines);
extern "C" __global__ void k_gsettle_prep(const uint32_t* __restrict__ grp_off, const uint32_t* __restrict__ grp_sets, uint32_t m, uint32_t n, uint32_t lo, uint32_t cn, const uint64_t* __restrict__ rand, const g1a* __restrict__ comb, const g2a* __restrict__ sig_aff, const uint8_t* __restrict__ sig_use, const uint8_t* __restrict__ set_code, const uint8_t* __restrict__ sig_code, const uint8_t* __restrict__ msg_skip, uint32_t* __restrict__ msg_of_pos, g1a* __restrict__ negr, g2a* __restrict__ sigq, uint8_t* __restrict__ sskip);
extern "C" __global__ void k_miller_accs_gsettle(const uint4* __restrict__ mlines, uint32_t m, const uint32_t* __restrict__ msg_of_pos, const uint32_t* __restrict__ grp_sets, const g1a* __restrict__ set_P, const uint8_t* __restrict__ set_code, const uint8_t* __restrict__ sig_code, const uint8_t* __restrict__ msg_skip, const uint4* __restrict__ slines, const uint8_t* __restrict__ sskip, uint32_t lo, uint32_t cn, uint32_t n, uint32_t nseg, uint32_t g_pad, fp12* __restrict__ V);
// lane-group cooperative mid-size kernels (k_hquad.hip): one DPP quad / one lane pair per set or pair; the one-lane line kernel at two waves per SIMD (k_w2_lines.hip)
extern "C" __global__ void k_set_hash_quad(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, g2a* __restrict__ Q, uint8_t* __restrict__ skip);
extern "C" __global__ void k_miller_lines_quad(const g1a* __restrict__ P, const g2a* __restrict__ Q, const uint8_t* __restrict__ skip, const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, uint32_t n, uint4* __restrict__ lines);
extern "C" __global__ void k_set_hash_duo(const uint8_t* __restrict__ msgs, const uint32_t* __restrict__ msg_off, const uint8_t* __restrict__ dst, uint32_t dlen, uint32_t n, g2a* __restrict__ Q, uint8_t* __restrict__ skip);
extern "C" __global__ void k_miller_lines_duo(const g1a* __restrict__ P, const g2a* __restrict__ Q, const uint8_t* __restrict__ skip, const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, uint32_t n, uint4* __restrict__ lines);
extern "C" __global__ void k_miller_lines_w2(const g1a* __restrict__ P, const g2a* __restrict__ Q, const uint8_t* __restrict__ skip, const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, uint32_t n, uint4* __restrict__ lines);
