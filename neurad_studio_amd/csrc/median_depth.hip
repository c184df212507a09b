// Median (quantile) depth of a ray: the midpoint of the first sample at which the accumulated weight reaches a threshold
// (DepthRenderer(method="median"), model_components/renderers.py:353-397; the contract is stated in include/neurad_hip.h
// at nrhip_median_depth).  The reference runs midpoints, cumsum, a constant tensor, searchsorted, clamp and gather: six
// launches and five passes over [R,S], and no packed form at all.  Here one 64-lane wavefront walks one ray front to back
// in chunks of 64 samples, as the compositing kernels do (composite.hip, packed_composite.h), and leaves it at the crossing:
//
//   carry    a float64 running sum; the chunk's prefix sums are a float64 wave scan (wave_scan.h), c = float32(carry + prefix)
//   crossing __ballot of !(c < q) over the live lanes, find-first-set: the first such sample.  The lane that owns it reads
//            its own starts / ends (the only read of those arrays) and writes the threshold's depth and index.
//   K        up to 8 thresholds ride on the same pass: a wave-uniform mask of the thresholds still open, the ray is left
//            when it is empty.  A threshold still open behind the last sample takes that sample (the reference's clamp).
//
// Dense and packed rays differ only in where a ray's samples lie.  No LDS, no atomics, nothing allocated; every output
// element has one writer, so the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "wave_scan.h"

namespace nrhip {
namespace {

constexpr int kWaves = 4;         // rays in flight per workgroup
constexpr int kMaxBlocks = 4096;  // grid cap: 16 384 waves, the rest of the rays grid-stride
constexpr int kMaxK = NRHIP_MEDIAN_MAX_THRESHOLDS;

struct Thresholds {  // kernel argument, by value
  float q[kMaxK];
  int k;
};

// PACKED: ray r owns the samples [seg[r], seg[r + 1]), clamped into [0, M]; dense: [r S, (r + 1) S) and M is not read.
template <bool PACKED>
__global__ __launch_bounds__(64 * kWaves) void median_depth_kernel(const float* __restrict__ w,
                                                                   const float* __restrict__ ts,
                                                                   const float* __restrict__ te,
                                                                   const int64_t* __restrict__ seg, int64_t R, int S,
                                                                   int64_t M, Thresholds th, float* __restrict__ od,
                                                                   int32_t* __restrict__ oi) {
  const int lane = threadIdx.x & 63;
  const int K = th.k;
  for (int64_t ray = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); ray < R; ray += (int64_t)gridDim.x * kWaves) {
    int64_t sb, se;
    if (PACKED) {
      sb = seg[ray], se = seg[ray + 1];
      sb = sb < 0 ? 0 : (sb > M ? M : sb);
      se = se < sb ? sb : (se > M ? M : se);
    } else {
      sb = ray * S, se = sb + S;
    }
    uint32_t open = (1u << K) - 1u;  // thresholds that have not crossed yet (the same in every lane)
    double carry = 0.0;
    for (int64_t i0 = sb; i0 < se && open; i0 += 64) {
      const int64_t i = i0 + lane;
      const bool live = i < se;
      const double incl = wscan::incl<wscan::Add>(live ? (double)w[i] : 0.0, lane);
      const float c = (float)(carry + incl);  // the ONE rounding to fp32 of the float64 prefix sum
      carry += wscan::last(incl);
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (!((open >> k) & 1u)) continue;
        const unsigned long long m = __ballot(live && !(c < th.q[k]));  // a NaN sum crosses where it stands
        if (!m) continue;
        open &= ~(1u << k);
        if (lane == __ffsll(m) - 1) {
          od[ray * K + k] = c != c ? c : (ts[i] + te[i]) * 0.5f;  // a NaN sum is kept, not turned into a depth
          if (oi) oi[ray * K + k] = (int32_t)(i - sb);
        }
      }
    }
    // never crossed: the last sample; a ray without samples (packed only): depth 0, index -1
    if (lane < K && ((open >> lane) & 1u)) {
      od[ray * K + lane] = se > sb ? (ts[se - 1] + te[se - 1]) * 0.5f : 0.f;
      if (oi) oi[ray * K + lane] = (int32_t)(se - sb) - 1;
    }
  }
}

int make_thresholds(const char* who, const float* thresholds, int32_t k, Thresholds& th) {
  NR_REQUIRE(k >= 1 && k <= kMaxK, NRHIP_ERR_INVALID_ARG, "%s: %d thresholds, not in [1,%d]", who, k, kMaxK);
  NR_REQUIRE(thresholds, NRHIP_ERR_INVALID_ARG, "%s: thresholds is NULL", who);
  th.k = k;
  for (int j = 0; j < kMaxK; ++j) {
    th.q[j] = j < k ? thresholds[j] : 0.f;
    NR_REQUIRE(std::isfinite(th.q[j]), NRHIP_ERR_INVALID_ARG, "%s: threshold %d is not finite", who, j);
  }
  return NRHIP_OK;
}

inline int blocks_for(int64_t r) {
  const int64_t b = (r + kWaves - 1) / kWaves;
  return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

}  // namespace
}  // namespace nrhip

using namespace nrhip;

extern "C" int nrhip_median_depth(const float* weights, const float* starts, const float* ends, int64_t r, int32_t s,
                                  const float* thresholds, int32_t k, float* out_depth, int32_t* out_index,
                                  void* stream) {
  NR_REQUIRE(r >= 0, NRHIP_ERR_INVALID_ARG, "median_depth: negative ray count");
  NR_REQUIRE(s >= 1, NRHIP_ERR_INVALID_ARG, "median_depth: %d samples per ray, needs at least one", s);
  Thresholds th;
  if (int rc = make_thresholds("median_depth", thresholds, k, th)) return rc;
  if (r == 0) return NRHIP_OK;
  NR_REQUIRE(weights && starts && ends && out_depth, NRHIP_ERR_INVALID_ARG, "median_depth: NULL pointer");
  median_depth_kernel<false><<<blocks_for(r), 64 * kWaves, 0, (hipStream_t)stream>>>(weights, starts, ends, nullptr, r, s,
                                                                                     r * s, th, out_depth, out_index);
  return check_launch("median_depth");
}

extern "C" int nrhip_median_depth_packed(const float* weights, const float* t_starts, const float* t_ends,
                                         const int64_t* segments, int64_t r, int64_t m, const float* thresholds,
                                         int32_t k, float* out_depth, int32_t* out_index, void* stream) {
  NR_REQUIRE(r >= 0 && m >= 0, NRHIP_ERR_INVALID_ARG, "median_depth_packed: negative ray or sample count");
  NR_REQUIRE(m < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "median_depth_packed: M >= 2^31");
  Thresholds th;
  if (int rc = make_thresholds("median_depth_packed", thresholds, k, th)) return rc;
  if (r == 0) return NRHIP_OK;
  NR_REQUIRE(segments && out_depth, NRHIP_ERR_INVALID_ARG, "median_depth_packed: segments or out_depth is NULL");
  NR_REQUIRE(m == 0 || (weights && t_starts && t_ends), NRHIP_ERR_INVALID_ARG,
             "median_depth_packed: NULL sample pointer with %lld samples", (long long)m);
  median_depth_kernel<true><<<blocks_for(r), 64 * kWaves, 0, (hipStream_t)stream>>>(weights, t_starts, t_ends, segments, r,
                                                                                    0, m, th, out_depth, out_index);
  return check_launch("median_depth_packed");
}
