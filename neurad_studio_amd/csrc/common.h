// Shared device/host helpers for libneurad_hip.so (gfx950 only).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/neurad_hip.h"

namespace nrhip {

void set_error(const char* fmt, ...);
int check_launch(const char* what);

// A/B switches of the library (NRHIP_* environment variables): read ONCE, when the library is loaded, into this struct --
// no getenv on any dispatch path.  A process that flips a switch afterwards (the parity tests, scripts/final_measure.sh's
// alternating runs) calls nrhip_tuning_reload().  Every switch selects between two implementations of the SAME result.
struct Tuning {
  int bin_round_log2;        // NRHIP_BIN_ROUND_LOG2 in 15..24: samples per round of the binned table gradient; default 23
  int bin_pairs;             // NRHIP_BIN_PAIRS: 1 "all", 0 "none", -1 unset (x-pair records at F = 1 only)
  bool bin_transpose;        // NRHIP_BIN_TRANSPOSE != "0": sample-index-major walk of coherent chunks (default on)
  bool bin_stats;            // NRHIP_BIN_STATS: print the record count of every round (synchronises; diagnostic)
  bool multi_bwd_runs;       // NRHIP_MULTI_BWD_RUNS != "0": run combining in the actor-grid gradient (default on)
  bool pair_bwd_runs;        // NRHIP_PAIR_BWD_RUNS != "0": run combining in the trajectory gradient (default on)
  bool mlp_generic;          // NRHIP_MLP_GENERIC: per-layer MLP kernels instead of the chained ones
  bool mlp_split_wgrad;      // NRHIP_MLP_SPLIT_WGRAD: weight gradients outside the chained backward
  bool mlp_split_bf16;       // NRHIP_MLP_SPLIT_BF16: 3-way bf16 split products in the composited render kernels
  int mlp_pairs;             // NRHIP_MLP_PAIRS: 1 / 0, -1 unset (fp16-pair products: the default of the composited kernels)
  bool mlp_pairs_train;      // NRHIP_MLP_PAIRS_TRAIN == "1": pair products in the per-sample (training forward) kernel too
  bool sampler_actor_inline; // NRHIP_SAMPLER_ACTOR_INLINE == "1": per-chunk in-box lookup in the fused sampler
  bool sdf_render_pair;      // NRHIP_SDF_RENDER_PAIR == "1": two rays per wave in sdf_render_fwd/bwd
};
const Tuning& tuning();

#define NR_REQUIRE(cond, code, ...)  \
  do {                               \
    if (!(cond)) {                   \
      ::nrhip::set_error(__VA_ARGS__); \
      return (code);                 \
    }                                \
  } while (0)

constexpr uint32_t kPrimeY = 2654435761u;  // encodings.py:419
constexpr uint32_t kPrimeZ = 805459861u;

// Device-side copy of nrhip_grid (kernel argument, by value).
struct GridDev {
  int L, F, log2T, dtype;
  float scal[NRHIP_MAX_LEVELS];
};

inline GridDev to_dev(const nrhip_grid& g) {
  GridDev d;
  d.L = g.num_levels;
  d.F = g.n_features;
  d.log2T = g.log2_table_size;
  d.dtype = g.param_dtype;
  for (int i = 0; i < NRHIP_MAX_LEVELS; ++i) d.scal[i] = i < g.num_levels ? g.scalings[i] : 0.f;
  return d;
}

int validate_grid(const nrhip_grid* g);

struct RaysDev {
  int64_t R;
  int S;
  int stride;  // row stride of starts/ends
  const float* o;
  const float* d;
  const float* area;
  const float* starts;
  const float* ends;
  const int32_t* order;  // optional processing order (permutation of the rays), honoured by the fused kernels
};
inline RaysDev to_dev(const nrhip_rays& r) {
  return RaysDev{r.n_rays, r.n_samples, r.sample_stride > 0 ? r.sample_stride : r.n_samples, r.origins, r.directions,
                 r.pixel_area, r.starts, r.ends, r.order};
}
int validate_rays(const nrhip_rays* r);

// nrhip_packed_rays on the device: the occupancy march's ragged segments.  Ray r owns the samples [segs[r], segs[r + 1]) of
// the [M]-shaped interval arrays and of every per-sample tensor; origins / directions / pixel area stay per RAY.  segs is
// NULL where the caller names a sample's ray another way (the table gradient's ray_of).
struct PackedRaysDev {
  int64_t R;
  int M;  // 1 <= M < 2^31: a batch without samples never reaches a kernel
  const float* o;
  const float* d;
  const float* area;
  const float* starts;
  const float* ends;
  const int64_t* segs;
};
inline PackedRaysDev to_dev(const nrhip_packed_rays& r) {
  return PackedRaysDev{r.n_rays, (int)r.n_samples, r.origins, r.directions, r.pixel_area, r.t_starts, r.t_ends, r.segments};
}
// The one check of the descriptor, for every entry point that takes one (`who` names it in the message): not NULL, counts
// not negative, M < 2^31, and -- unless the batch has no rays or no samples, when nothing is read -- no NULL array; the
// segments only where the entry point walks them.
int validate_packed_rays(const char* who, const nrhip_packed_rays* r, bool need_segments);
// A point set [n, stride >= 3 floats] (`who` names the entry point and the set): count not negative and < 2^31, stride >= 3,
// no NULL array unless the set is empty.
int validate_points(const char* who, const float* points, int32_t stride, int64_t n);

// Where a ray's samples lie, for kernels written once over both layouts: samples of the ray; row of a per-sample tensor
// that holds sample s of the ray; index of its interval in starts / ends.  Packed: the count is clamped into [0, M] and
// every index into [0, M), so segments that break their precondition still read inside the arrays.
__device__ __forceinline__ int ray_sample_count(const RaysDev& r, int64_t) { return r.S; }
__device__ __forceinline__ int64_t ray_sample_row(const RaysDev& r, int64_t ray, int s) { return ray * r.S + s; }
__device__ __forceinline__ int64_t ray_sample_interval(const RaysDev& r, int64_t ray, int s) { return ray * r.stride + s; }
__device__ __forceinline__ int ray_sample_count(const PackedRaysDev& r, int64_t ray) {
  const int64_t n = r.segs[ray + 1] - r.segs[ray];
  return (int)(n < (int64_t)r.M ? n : (int64_t)r.M);
}
__device__ __forceinline__ int64_t ray_sample_row(const PackedRaysDev& r, int64_t ray, int s) {
  const int64_t i = r.segs[ray] + s;
  return i < 0 ? 0 : (i < (int64_t)r.M ? i : (int64_t)r.M - 1);
}
__device__ __forceinline__ int64_t ray_sample_interval(const PackedRaysDev& r, int64_t ray, int s) {
  return ray_sample_row(r, ray, s);
}
// The other way round, for kernels with one thread per SAMPLE: the ray of the sample in row i of a per-sample tensor and
// the index of its interval.  Dense: the row is ray * S + s.  Packed: ray_of [M] (the march's ray_indices) names the ray
// and the row is the interval's own index; both are clamped into their arrays, segs is not read.
__device__ __forceinline__ int64_t ray_sample_ray_of_row(const RaysDev& r, const int64_t*, int64_t i) { return i / r.S; }
__device__ __forceinline__ int64_t ray_sample_interval_of_row(const RaysDev& r, int64_t ray, int64_t i) {
  return ray_sample_interval(r, ray, (int)(i - ray * r.S));
}
__device__ __forceinline__ int64_t ray_sample_ray_of_row(const PackedRaysDev& r, const int64_t* ray_of, int64_t i) {
  const int64_t ray = ray_of[i < 0 ? 0 : (i < (int64_t)r.M ? i : (int64_t)r.M - 1)];
  return ray < 0 ? 0 : (ray < r.R ? ray : r.R - 1);
}
__device__ __forceinline__ int64_t ray_sample_interval_of_row(const PackedRaysDev& r, int64_t, int64_t i) {
  return i < 0 ? 0 : (i < (int64_t)r.M ? i : (int64_t)r.M - 1);
}

// ---------------------------------------------------------------------------------------------
// Table element loads: F features of one entry, fp32 or fp16 storage, one vector load each.
// ---------------------------------------------------------------------------------------------
template <int F, bool HALF>
struct Entry;

template <int F>
struct Entry<F, false> {
  static __device__ __forceinline__ void load(const void* table, uint32_t row, float (&v)[F]) {
    // 32-bit byte offset from a wave-uniform base -> global_load with an SGPR base + one VGPR offset
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(table) + row * (uint32_t)(F * 4));
    if constexpr (F == 1) {
      v[0] = *p;
    } else if constexpr (F == 2) {
      float2 t = *reinterpret_cast<const float2*>(p);
      v[0] = t.x, v[1] = t.y;
    } else if constexpr (F == 4) {
      float4 t = *reinterpret_cast<const float4*>(p);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
      static_assert(F == 8, "F in {1,2,4,8}");
      float4 a = *reinterpret_cast<const float4*>(p);
      float4 b = *reinterpret_cast<const float4*>(p + 4);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    }
  }
};

template <int F>
struct Entry<F, true> {
  static __device__ __forceinline__ void load(const void* table, uint32_t row, float (&v)[F]) {
    const __half* p =
        reinterpret_cast<const __half*>(reinterpret_cast<const char*>(table) + row * (uint32_t)(F * 2));
    if constexpr (F == 1) {
      v[0] = __half2float(*p);
    } else if constexpr (F == 2) {
      float2 t = __half22float2(*reinterpret_cast<const __half2*>(p));
      v[0] = t.x, v[1] = t.y;
    } else if constexpr (F == 4) {
      uint2 raw = *reinterpret_cast<const uint2*>(p);
      float2 a = __half22float2(*reinterpret_cast<const __half2*>(&raw.x));
      float2 b = __half22float2(*reinterpret_cast<const __half2*>(&raw.y));
      v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else {
      static_assert(F == 8, "F in {1,2,4,8}");
      uint4 raw = *reinterpret_cast<const uint4*>(p);
      const __half2* h = reinterpret_cast<const __half2*>(&raw);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float2 t = __half22float2(h[i]);
        v[2 * i] = t.x, v[2 * i + 1] = t.y;
      }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// One hash-grid level: HashEncoding.pytorch_fwd for a single (point, level)
// (encodings.py:425-464).  x in [0,1]^3, `scale` = scalings[l], table_l = base row of the level.
// The lerp tree and corner pairing follow the reference exactly (f03/f12/f56/f47 -> f0312/f4756).
// ---------------------------------------------------------------------------------------------
struct Corners {
  uint32_t idx[8];  // reference corner order 0..7 (encodings.py:437-444), already masked (no level offset)
  float ox, oy, oz;
};

__device__ __forceinline__ Corners hash_corners(float x, float y, float z, float scale, uint32_t mask) {
  Corners c;
  // __fmul_rn / __fsub_rn: the product must be ROUNDED before floor/ceil and before the offset is taken,
  // exactly like torch's separate mul and sub.  Letting the compiler contract x*scale - floor(..) into an
  // fma changes the offset by up to half an ulp of sx (~5e-4 at scale 8192) -- measured 7e-5 rel-L2.
  const float sx = __fmul_rn(x, scale), sy = __fmul_rn(y, scale), sz = __fmul_rn(z, scale);
  const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
  const uint32_t ifx = (uint32_t)(int)fx, ify = (uint32_t)(int)fy, ifz = (uint32_t)(int)fz;
  const uint32_t icx = (uint32_t)(int)ceilf(sx), icy = (uint32_t)(int)ceilf(sy), icz = (uint32_t)(int)ceilf(sz);
  c.ox = __fsub_rn(sx, fx), c.oy = __fsub_rn(sy, fy), c.oz = __fsub_rn(sz, fz);
  // int32*int64 products in the reference never wrap in 64 bit; their low log2(T) bits equal the
  // uint32-wrapped products (T is a power of two), verified in tests against exact golden indices.
  const uint32_t hyc = icy * kPrimeY, hyf = ify * kPrimeY, hzc = icz * kPrimeZ, hzf = ifz * kPrimeZ;
  c.idx[0] = (icx ^ hyc ^ hzc) & mask;  // c c c
  c.idx[1] = (icx ^ hyf ^ hzc) & mask;  // c f c
  c.idx[2] = (ifx ^ hyf ^ hzc) & mask;  // f f c
  c.idx[3] = (ifx ^ hyc ^ hzc) & mask;  // f c c
  c.idx[4] = (icx ^ hyc ^ hzf) & mask;  // c c f
  c.idx[5] = (icx ^ hyf ^ hzf) & mask;  // c f f
  c.idx[6] = (ifx ^ hyf ^ hzf) & mask;  // f f f
  c.idx[7] = (ifx ^ hyc ^ hzf) & mask;  // f c f
  return c;
}

// trilinear blend of the 8 corner entries, reference order of operations (encodings.py:446-464)
template <int F>
__device__ __forceinline__ void lerp_corners(const Corners& c, const float (&f)[8][F], float (&out)[F]) {
  const float ox = c.ox, oy = c.oy, oz = c.oz;
  const float mx = 1.f - ox, my = 1.f - oy, mz = 1.f - oz;
#pragma unroll
  for (int i = 0; i < F; ++i) {
    // a*o + b*(1-o) as fma(a, o, b*(1-o)): 2 VALU ops per lerp; one rounding fewer than torch's mul,mul,add
    const float f03 = fmaf(f[0][i], ox, f[3][i] * mx);
    const float f12 = fmaf(f[1][i], ox, f[2][i] * mx);
    const float f56 = fmaf(f[5][i], ox, f[6][i] * mx);
    const float f47 = fmaf(f[4][i], ox, f[7][i] * mx);
    const float f0312 = fmaf(f03, oy, f12 * my);
    const float f4756 = fmaf(f47, oy, f56 * my);
    out[i] = fmaf(f0312, oz, f4756 * mz);
  }
}

// F = 1: the (floor x, ceil x) corners of one (y, z) differ only through ifx ^ icx -- the same value for all four such pairs
// of a sample.  When it is 0 or 1 (x integral, or floor(x) even: half of the samples) both entries lie in one aligned
// 2-entry pair and ONE 8-byte (fp16: 4-byte) load serves both; the other lanes fetch their ceil corners with a second,
// exec-masked load.  Same bytes, same results; the L1 sees 6 line accesses per (sample, level) on average instead of 8,
// and the level-partitioned F = 1 kernels (every access an L2 hit) run against exactly that rate.  row0 must be even.
template <bool HALF>
__device__ __forceinline__ void load_corners_f1(const void* table, uint32_t row0, const Corners& c, float (&f)[8][1]) {
  constexpr int kF[4] = {3, 2, 7, 6}, kC[4] = {0, 1, 4, 5};  // (f, c) corner of the pairs (y, z) = cc, fc, cf, ff
  if constexpr (!HALF) {
    // fp32 (round 4): ONE aligned 16-byte load per (y, z) where floor x ^ ceil x is 0, 1 or 3 -- three quarters of the
    // samples: both entries then lie in one aligned 4-entry block.  5 line accesses per (sample, level) instead of 6; the L1
    // charges per line, not per byte (scripts/probes/l1_coalesce_probe.hip).  row0 must be a multiple of 4.
    const bool same = ((c.idx[3] ^ c.idx[0]) >> 2) == 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t rf = row0 + c.idx[kF[p]], rc = row0 + c.idx[kC[p]];
      const float4 t = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(table) + (rf & ~3u) * 4u);
      const uint32_t a = rf & 3u, b = rc & 3u;
      f[kF[p]][0] = a == 0u ? t.x : (a == 1u ? t.y : (a == 2u ? t.z : t.w));
      f[kC[p]][0] = b == 0u ? t.x : (b == 1u ? t.y : (b == 2u ? t.z : t.w));  // meaningful where `same`
    }
    if (!same) {
#pragma unroll
      for (int p = 0; p < 4; ++p) Entry<1, false>::load(table, row0 + c.idx[kC[p]], f[kC[p]]);
    }
    return;
  }
  const bool same = ((c.idx[3] ^ c.idx[0]) >> 1) == 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t rf = row0 + c.idx[kF[p]], rc = row0 + c.idx[kC[p]];
    float lo, hi;
    if constexpr (HALF) {
      const float2 t = __half22float2(*reinterpret_cast<const __half2*>(reinterpret_cast<const char*>(table) + (rf & ~1u) * 2u));
      lo = t.x, hi = t.y;
    } else {
      const float2 t = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(table) + (rf & ~1u) * 4u);
      lo = t.x, hi = t.y;
    }
    f[kF[p]][0] = (rf & 1u) ? hi : lo;
    f[kC[p]][0] = (rc & 1u) ? hi : lo;  // meaningful where `same`
  }
  if (!same) {
#pragma unroll
    for (int p = 0; p < 4; ++p) Entry<1, HALF>::load(table, row0 + c.idx[kC[p]], f[kC[p]]);
  }
}

// PAIRED (F = 1 only): load_corners_f1.  For kernels whose threads do ONE level each (proposal_levels_lp: 286 -> 265 us on
// 2.1 M samples x 6 levels); where a thread walks all levels the exec-masked second load turns one memory round trip
// into one per level and loses (409 -> 492 us), so it is opt-in.
template <int F, bool HALF, bool PAIRED = false>
__device__ __forceinline__ void hash_level(const void* table, uint32_t level_row0, float x, float y, float z,
                                           float scale, uint32_t mask, float (&out)[F]) {
  const Corners c = hash_corners(x, y, z, scale, mask);
  float f[8][F];
  if constexpr (F == 1 && PAIRED) {
    load_corners_f1<HALF>(table, level_row0, c, f);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) Entry<F, HALF>::load(table, level_row0 + c.idx[k], f[k]);
  }
  lerp_corners<F>(c, f, out);
}

// Trilinear corner weights in the same corner order (for the scatter-add backward).
__device__ __forceinline__ void corner_weights(const Corners& c, float (&w)[8]) {
  const float ox = c.ox, oy = c.oy, oz = c.oz, mx = 1.f - ox, my = 1.f - oy, mz = 1.f - oz;
  w[0] = ox * oy * oz;
  w[1] = ox * my * oz;
  w[2] = mx * my * oz;
  w[3] = mx * oy * oz;
  w[4] = ox * oy * mz;
  w[5] = ox * my * mz;
  w[6] = mx * my * mz;
  w[7] = mx * oy * mz;
}

// ---------------------------------------------------------------------------------------------
// H2 + H3: sample -> gaussian (mean,std) -> contracted position in [0,1]^3 and contracted std
// (cameras/rays.py:109-124, M=1; spatial_distortions.py:103-113,126-141, order=inf)
// ---------------------------------------------------------------------------------------------
struct SamplePos {
  float x, y, z, std;
};

// x^(1/3) for x >= 0 via v_log_f32 / v_exp_f32 (~1e-6 relative).  Only the gaussian std (which feeds the smooth
// down-weighting 1/max(1, 2*s_l*std)) goes through it -- never a position -- so torch's pow(x, 1/3) need not be
// matched to the ulp; a full powf costs ~40 VALU instructions twice per sample.
__device__ __forceinline__ float fast_cbrt(float x) {
  return __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(x) * (1.0f / 3.0f));
}

// H2 alone: gaussian mean (world space) and std of a sample (cameras/rays.py:109-124, M=1)
__device__ __forceinline__ SamplePos sample_gaussian(float ox, float oy, float oz, float dx, float dy, float dz,
                                                     float area, float t0, float t1) {
#pragma clang fp contract(off)
  const float dist = (t1 - t0) / 2.f;
  const float t = t0 + 1.f * dist;
  SamplePos p;
  p.x = ox + dx * t, p.y = oy + dy * t, p.z = oz + dz * t;
  p.std = fast_cbrt((area * (t * t)) * dist);
  return p;
}

// H5: is the world-space point (x, y, z) strictly inside a box?  w: the box's 3x4 world->box matrix (a row of cand_w2b),
// b: its half sizes [3].  -> the box-frame position as well.  THE in-box test: find_hit (actors.hip) and the box-aware
// occupancy march (occgrid.hip) both call it on sample_gaussian's mean, so field and march agree on every sample.
__device__ __forceinline__ bool box_contains(const float* w, const float* b, float x, float y, float z, float& bx, float& by,
                                             float& bz) {
  bx = w[0] * x + w[1] * y + w[2] * z + w[3];
  by = w[4] * x + w[5] * y + w[6] * z + w[7];
  bz = w[8] * x + w[9] * y + w[10] * z + w[11];
  return fabsf(bx) < b[0] && fabsf(by) < b[1] && fabsf(bz) < b[2];
}

// H3 alone: ScaledSceneContraction(order=inf) of a gaussian -> [0,1]^3 (spatial_distortions.py:103-141)
__device__ __forceinline__ SamplePos contract_gaussian(float mx, float my, float mz, float std, float scale) {
#pragma clang fp contract(off)
  mx /= scale, my /= scale, mz /= scale, std /= scale;
  const float mag = fmaxf(fabsf(mx), fmaxf(fabsf(my), fabsf(mz)));
  if (!(mag < 1.f)) {
    const float cm = fmaxf(mag, 1.f);
    const float k = 2.f - (1.f / cm);
    mx = k * (mx / cm), my = k * (my / cm), mz = k * (mz / cm);
    const float sc = fast_cbrt(2.f * cm - 1.f) / cm;
    std = std * (sc * sc);
  }
  SamplePos p;
  p.x = (mx + 2.f) / 4.f, p.y = (my + 2.f) / 4.f, p.z = (mz + 2.f) / 4.f;
  p.std = std / 4.f;
  return p;
}

// Backward of the contraction's m' = k(mag) m past the scalar chain: gm <- k gm + d|m|_inf/dm g_mag.  torch's inf-norm
// backward splits g_mag evenly over the axes tied for the maximum, each with its sign (linalg_vector_norm_backward).
__device__ __forceinline__ void inf_norm_bwd(const float* m, const float* am, float mag, float k, float g_mag, float* gm) {
  const float share = g_mag / (float)((am[0] == mag) + (am[1] == mag) + (am[2] == mag));
#pragma unroll
  for (int c = 0; c < 3; ++c) gm[c] = gm[c] * k + (am[c] == mag ? (m[c] < 0.f ? -share : share) : 0.f);
}

// H2 then H3.  Position arithmetic mirrors torch op for op (separately rounded mul/add/div, no fma): one ulp of the
// contracted coordinate is 8192 * 6e-8 = 5e-4 of a cell at the finest level, so rounding-order matters.
__device__ __forceinline__ SamplePos sample_position(float ox, float oy, float oz, float dx, float dy, float dz,
                                                     float area, float t0, float t1, float scale) {
  const SamplePos g = sample_gaussian(ox, oy, oz, dx, dy, dz, area, t0, t1);
  return contract_gaussian(g.x, g.y, g.z, g.std, scale);
}

// H4: 1 / max(1, 2*scalings_l*std)   (neurad_encoding.py:302)
__device__ __forceinline__ float rescale_weight(float scale_l, float std) {
  return __builtin_amdgcn_rcpf(fmaxf(scale_l * 2.f * std, 1.f));  // v_rcp_f32 (1 ulp); weights are smooth in std
}

// S2 backward: d trunc_exp(x)/dx = exp(clamp(x, -15, 15)) (activations.py:37-41) with x = log(density) recovered from the
// saved forward output.  torch.clamp keeps a NaN where fminf / fmaxf return the other operand: a NaN density must poison
// the gradient here as it does there, not come back as e^-15.  Finite and infinite x take the clamp as before.
__device__ __forceinline__ float trunc_exp_bwd_factor(float density) {
  const float x = logf(density);
  return expf(x != x ? x : fminf(fmaxf(x, -15.f), 15.f));
}

// F3: 16 real SH components (utils/math.py:31-94) of a direction given as (dir+1)/2 -- the torch path
// evaluates the polynomials on that [0,1]-normalised vector directly (base_field.py:136-142).
__device__ __forceinline__ void sh4(float x, float y, float z, float (&c)[16]) {
  const float xx = x * x, yy = y * y, zz = z * z;
  c[0] = 0.28209479177387814f;
  c[1] = 0.4886025119029199f * y;
  c[2] = 0.4886025119029199f * z;
  c[3] = 0.4886025119029199f * x;
  c[4] = 1.0925484305920792f * x * y;
  c[5] = 1.0925484305920792f * y * z;
  c[6] = 0.9461746957575601f * zz - 0.31539156525251999f;
  c[7] = 1.0925484305920792f * x * z;
  c[8] = 0.5462742152960396f * (xx - yy);
  c[9] = 0.5900435899266435f * y * (3.f * xx - yy);
  c[10] = 2.890611442640554f * x * y * z;
  c[11] = 0.4570457994644658f * y * (5.f * zz - 1.f);
  c[12] = 0.3731763325901154f * z * (5.f * zz - 3.f);
  c[13] = 0.4570457994644658f * x * (5.f * zz - 1.f);
  c[14] = 1.445305721320277f * z * (xx - yy);
  c[15] = 0.5900435899266435f * x * (xx - 3.f * yy);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// DPP: v_mov_b32_dpp with control CTRL, all rows and banks, bound_ctrl = false: lanes without a source keep `old` -----
template <int CTRL>
__device__ __forceinline__ int dpp(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp(float old, float v) {
  return __builtin_bit_cast(float, dpp<CTRL>(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v)));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t old, uint32_t v) {
  return (uint32_t)dpp<CTRL>((int)old, (int)v);
}
template <int CTRL>
__device__ __forceinline__ double dpp(double old, double v) {
  const long long o = __builtin_bit_cast(long long, old), x = __builtin_bit_cast(long long, v);
  const uint32_t lo = (uint32_t)dpp<CTRL>((int)(uint32_t)o, (int)(uint32_t)x);
  const uint32_t hi = (uint32_t)dpp<CTRL>((int)(uint32_t)(o >> 32), (int)(uint32_t)(x >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int CTRL>
__device__ __forceinline__ long long dpp(long long old, long long v) {  // (the integer sums of pose_opt.hip)
  return __builtin_bit_cast(long long, dpp<CTRL>(__builtin_bit_cast(double, old), __builtin_bit_cast(double, v)));
}
// Rows of 16 lanes.  row_shr:n = 0x110+n: lane i reads lane i-n of its row; row_shl:n = 0x100+n: lane i reads lane i+n.
// Lanes whose source is outside the row get `fill`.
template <int N, class T>
__device__ __forceinline__ T dpp_row_shr(T v, T fill) {
  return dpp<0x110 + N>(fill, v);
}
template <int N, class T>
__device__ __forceinline__ T dpp_row_shl(T v, T fill) {
  return dpp<0x100 + N>(fill, v);
}

// Run combining before atomics: equal keys in adjacent lanes form a run, `run` numbers the runs of the wave (the count
// of run heads up to and including the lane).  Segmented suffix sum of v[0..N) onto each run's head lane, inside the
// 16-lane rows.  A macro, not a function template: the function form changes the code of the kernels around it (more
// VGPRs and instructions in the binned emit kernels).  v, N and run are pasted as they are: pass a plain array variable,
// a constant and a plain uint32_t variable, no expressions.  (NR_SEG_STEP_ is the macro's own helper and has to stay
// defined for it.)
#define NR_SEG_STEP_(v, N, run, OFF)                                       \
  {                                                                        \
    const bool same = dpp_row_shl<OFF>(run, 0xffffffffu) == run;           \
    _Pragma("unroll") for (int j = 0; j < N; ++j) {                        \
      const float t = dpp_row_shl<OFF>(v[j], 0.f);                         \
      if (same) v[j] += t;                                                 \
    }                                                                      \
  }
#define NR_SUM_RUNS_ONTO_HEADS(v, N, run) \
  NR_SEG_STEP_(v, N, run, 1) NR_SEG_STEP_(v, N, run, 2) NR_SEG_STEP_(v, N, run, 4) NR_SEG_STEP_(v, N, run, 8)

// Orders one wave's LDS traffic (the one-wave-per-ray kernels exchange through LDS without a workgroup barrier).
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Host-side dispatch on features-per-level: fn(std::integral_constant<int, F>) -- the argument converts to a constant
// expression, so `kernel<F>` works inside a generic lambda.  f must be validated (validate_grid): anything but 1, 2, 4
// goes to 8.  The second form also carries a flag (fp16 storage, x-pair records) as std::bool_constant.
template <class Fn>
inline void dispatch_f(int f, Fn&& fn) {
  switch (f) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    default: fn(std::integral_constant<int, 8>{}); break;
  }
}
template <class Fn>
inline void dispatch_f(int f, bool flag, Fn&& fn) {
  dispatch_f(f, [&](auto F) {
    if (flag) fn(F, std::true_type{});
    else fn(F, std::false_type{});
  });
}

inline int grid_for(int64_t threads, int block) { return (int)((threads + block - 1) / block); }

// --------------------------------------------------------------------------------------------
// fp32 MFMA building block shared by the fused render kernel and the chained MLP kernels.
using f32x4 = __attribute__((ext_vector_type(4))) float;

// One MFMA layer on a 16-sample tile, weights as the A operand read from LDS in fragment order
// [mb][s4][lane][s3] (one conflict-free ds_read_b128 per 4 k-steps), samples as the B operand in registers:
// acc[mb] += Σ_s A[mb][s] * B[s],  NS k-steps, NBLK output blocks, all statically unrolled.
template <int NBLK, int NS>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ wf, int lane, const float (&b)[NS],
                                           f32x4 (&acc)[NBLK]) {
#pragma unroll
  for (int s4 = 0; s4 < NS / 4; ++s4) {
    f32x4 a[NBLK];
#pragma unroll
    for (int mb = 0; mb < NBLK; ++mb)
      a[mb] = *reinterpret_cast<const f32x4*>(wf + ((mb * (NS / 4) + s4) * 64 + lane) * 4);
#pragma unroll
    for (int s3 = 0; s3 < 4; ++s3)
#pragma unroll
      for (int mb = 0; mb < NBLK; ++mb)
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mb][s3], b[4 * s4 + s3], acc[mb], 0, 0, 0);
  }
}

}  // namespace nrhip
