// Packed (ragged) compositing for the occupancy-marched samples of occgrid.hip: nerfacc's packed render_weight_from_alpha /
// render_weight_from_density / accumulate_along_rays and their fusion, forward and backward.
// `seg` is int64 [R+1]: ray r owns the packed samples [seg[r], seg[r+1]).  Owner-computes: one wavefront walks one ray in
// chunks of 64 samples with a carried prefix (the structure of the dense kernels of composite.hip, same arithmetic), rays
// are handed out grid-stride over a capped grid.  No atomics (bitwise reproducible), no LDS, nothing allocated.
//
// Channel rows [M,C]: when C is a multiple of 4 (and the rows are 16-byte aligned) LP lanes share a sample and each owns K
// float4 of its row, LP * K == C / 4 -- C = 32: 8 lanes x 1, C = 48: 4 lanes x 3 -- so every load / store of a wave is a
// run of full 16-byte pieces.  Any other C takes the generic path (a lane per sample, a loop over the channels).
#pragma once
#include "common.h"
#include "wave_scan.h"

namespace nrhip {
namespace packed {

constexpr int kWaves = 4;        // rays in flight per workgroup
constexpr int kMaxBlocks = 4096;  // grid cap: 16 384 waves, the rest of the rays grid-stride
constexpr int kMaxK = 3;         // float4 per lane and sample on the vector path

enum Mode { kAlpha = 0, kDensity = 1, kWeights = 2 };  // what `x` holds: alphas, sigmas, or the weights themselves

struct Plan {
  int lp, k;  // k == 0: generic path (lp = 1)
};

// host: lanes per sample / float4 per lane for C channels; generic when C is no multiple of 4 or a row pointer is unaligned
inline Plan plan_for(int c, const void* p0, const void* p1, const void* p2) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2);
  if ((c & 3) != 0 || (bits & 15) != 0) return {1, 0};
  const int nv = c >> 2;
  int lp = nv & -nv;
  if (lp > 8) lp = 8;
  const int k = nv / lp;
  if (k > kMaxK) return {1, 0};
  return {lp, k};
}

inline int blocks_for(int64_t r) {
  const int64_t b = (r + kWaves - 1) / kWaves;
  return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

// total over each aligned group of lp in {1,2,4,8} lanes, in every lane of the group (DPP quad_perm / row_half_mirror)
__device__ __forceinline__ float group_sum(float q, int lp) {
  if (lp >= 2) q += dpp<0xB1>(0.f, q);  // quad_perm [1,0,3,2]
  if (lp >= 4) q += dpp<0x4E>(0.f, q);  // quad_perm [2,3,0,1]
  if (lp >= 8) q += dpp<0x141>(0.f, q);  // row_half_mirror: the other quad of the 8 (quads are uniform by now)
  return q;
}

// total over the lanes of the wave with the same lane % lp, lp in {1,2,4,8}: row rotations inside the 16-lane rows, then the
// four rows
__device__ __forceinline__ float class_sum(float v, int lp) {
  if (lp <= 1) v += dpp<0x121>(0.f, v);  // row_ror:1
  if (lp <= 2) v += dpp<0x122>(0.f, v);  // row_ror:2
  if (lp <= 4) v += dpp<0x124>(0.f, v);  // row_ror:4
  v += dpp<0x128>(0.f, v);               // row_ror:8
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// Forward of every packed op.  ts / te: interval ends [M] (kDensity: needed; otherwise only for the depth).  x [M]: alphas,
// sigmas or weights.  feat [M,C], read iff `of` is given (an empty batch has no feat to point at, its rows of `of` are still
// zeroed).  Outputs, each may be NULL: of [R,C] = sum w f, od [R] = sum w (ts + te) / 2, oa [R] = sum w, and per sample ow
// (weights), ot (transmittance), oal (alphas).  A ray with an empty segment gets zeros.
template <int MODE>
__global__ __launch_bounds__(64 * kWaves) void fwd_kernel(const float* __restrict__ ts, const float* __restrict__ te,
                                                          const float* __restrict__ x, const float* __restrict__ feat,
                                                          const int64_t* __restrict__ seg, int64_t R, int C, int LP, int K,
                                                          float* __restrict__ of, float* __restrict__ od,
                                                          float* __restrict__ oa, float* __restrict__ ow,
                                                          float* __restrict__ ot, float* __restrict__ oal) {
  const int lane = threadIdx.x & 63;
  const int sub = lane & (LP - 1), sl = lane / LP, spw = 64 / LP;
  for (int64_t ray = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); ray < R; ray += (int64_t)gridDim.x * kWaves) {
    const int64_t sb = seg[ray], se = seg[ray + 1];
    float carry = (MODE == kAlpha) ? 1.f : 0.f;
    float acc = 0.f, dep = 0.f;
    float4 fa[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) fa[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i0 = sb; i0 < se; i0 += 64) {
      const int64_t i = i0 + lane;
      const bool live = i < se;
      float w;
      if (MODE == kWeights) {
        w = live ? x[i] : 0.f;
      } else {
        float alpha, step, T;  // step = (1 - alpha) [kAlpha] or sigma * delta [kDensity]
        if (MODE == kAlpha) {
          alpha = live ? x[i] : 0.f;
          step = 1.f - alpha;
          const float incl = wscan::incl<wscan::Mul>(step, lane);
          T = carry * wscan::shift_up1(incl, 1.f, lane);
          carry *= wscan::last(incl);
        } else {
          step = live ? x[i] * (te[i] - ts[i]) : 0.f;
          alpha = 1.f - expf(-step);
          const float incl = wscan::incl<wscan::Add>(step, lane);
          T = expf(-(carry + wscan::shift_up1(incl, 0.f, lane)));
          carry += wscan::last(incl);
        }
        w = live ? alpha * T : 0.f;
        if (live) {
          if (ow) ow[i] = w;
          if (ot) ot[i] = T;
          if (oal) oal[i] = alpha;
        }
      }
      acc += w;
      if (od && live) dep += w * ((ts[i] + te[i]) / 2.f);
      if (of) {
        const int cnt = (int)(se - i0 < 64 ? se - i0 : 64);
        if (K > 0) {
          for (int j0 = 0; j0 < cnt; j0 += spw) {
            const int j = j0 + sl;
            const float wj = __shfl(w, j, 64);
            if (j < cnt) {
              const float4* fp = reinterpret_cast<const float4*>(feat + (i0 + j) * C) + sub;
#pragma unroll
              for (int k = 0; k < kMaxK; ++k)
                if (k < K) {
                  const float4 f4 = fp[k * LP];
                  fa[k].x = fmaf(wj, f4.x, fa[k].x);
                  fa[k].y = fmaf(wj, f4.y, fa[k].y);
                  fa[k].z = fmaf(wj, f4.z, fa[k].z);
                  fa[k].w = fmaf(wj, f4.w, fa[k].w);
                }
            }
          }
        } else {
          // generic C: one wave reduction per channel and chunk, the row's running sum lives in `of` (owner-only, in order)
          for (int ch = 0; ch < C; ++ch) {
            const float p = wscan::reduce<wscan::Add>(live ? w * feat[i * C + ch] : 0.f);
            if (lane == 0) of[ray * C + ch] = (i0 == sb ? 0.f : of[ray * C + ch]) + p;
          }
        }
      }
    }
    if (of) {
      if (K > 0) {
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
          if (k < K) {
            float4 v = fa[k];
            v.x = class_sum(v.x, LP), v.y = class_sum(v.y, LP), v.z = class_sum(v.z, LP), v.w = class_sum(v.w, LP);
            if (lane < LP) reinterpret_cast<float4*>(of + ray * C)[sub + k * LP] = v;
          }
      } else if (sb >= se) {
        for (int ch = lane; ch < C; ch += 64) of[ray * C + ch] = 0.f;
      }
    }
    if (oa) {
      acc = wscan::reduce<wscan::Add>(acc);
      if (lane == 0) oa[ray] = acc;
    }
    if (od) {
      dep = wscan::reduce<wscan::Add>(dep);
      if (lane == 0) od[ray] = dep;
    }
  }
}

// Backward of every packed op.  Upstream: gF [R,C] (with feat), gD [R], gA [R] per ray, gW [M] on the weights and gT [M] on
// the transmittance (kAlpha) per sample; each may be NULL.  The gradient that reaches the weight of sample i is
//   G_i = gW_i + gA + gD mid_i + sum_c gF_c f_ic
// kWeights: gx = G.  kAlpha / kDensity: the dense weights_bwd_kernel's formulas on G (composite.hip), the transmittance
// recomputed per chunk from the forward's own carries, the sums over k > i as a suffix scan over the chunks last-to-first.
// gf [M,C] = w_i gF_c.  gx / gf may be NULL.
template <int MODE>
__global__ __launch_bounds__(64 * kWaves) void bwd_kernel(const float* __restrict__ ts, const float* __restrict__ te,
                                                          const float* __restrict__ x, const float* __restrict__ feat,
                                                          const int64_t* __restrict__ seg, const float* __restrict__ gF,
                                                          const float* __restrict__ gD, const float* __restrict__ gA,
                                                          const float* __restrict__ gW, const float* __restrict__ gT,
                                                          int64_t R, int C, int LP, int K, float* __restrict__ gx,
                                                          float* __restrict__ gf) {
  const int lane = threadIdx.x & 63;
  const int sub = lane & (LP - 1), sl = lane / LP, spw = 64 / LP;
  for (int64_t ray = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); ray < R; ray += (int64_t)gridDim.x * kWaves) {
    const int64_t sb = seg[ray], se = seg[ray + 1];
    if (sb >= se) continue;
    const int64_t n = se - sb;
    const int64_t nchunk = (n + 63) / 64;
    const float gd = gD ? gD[ray] : 0.f, ga = gA ? gA[ray] : 0.f;
    float4 g4[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      g4[k] = (feat && k < K) ? reinterpret_cast<const float4*>(gF + ray * C)[sub + k * LP] : make_float4(0.f, 0.f, 0.f, 0.f);

    // G of the chunk at i0 (cnt live samples), lane = sample; with `write`, the chunk's rows of gf from the weights w
    auto upstream = [&](int64_t i0, int cnt, float w, bool write) -> float {
      const int64_t i = i0 + lane;
      const bool live = lane < cnt;
      float G = ga;
      if (gW && live) G += gW[i];
      if (gD && live) G += gd * ((ts[i] + te[i]) / 2.f);
      if (feat) {
        float qs = 0.f;
        if (K > 0) {
          for (int j0 = 0; j0 < cnt; j0 += spw) {
            const int j = j0 + sl;
            const float wj = __shfl(w, j, 64);
            float q = 0.f;
            if (j < cnt) {
              const float4* fp = reinterpret_cast<const float4*>(feat + (i0 + j) * C) + sub;
              float4* gp = reinterpret_cast<float4*>(gf + (i0 + j) * C) + sub;
#pragma unroll
              for (int k = 0; k < kMaxK; ++k)
                if (k < K) {
                  const float4 f4 = fp[k * LP];
                  q = fmaf(g4[k].x, f4.x, q);
                  q = fmaf(g4[k].y, f4.y, q);
                  q = fmaf(g4[k].z, f4.z, q);
                  q = fmaf(g4[k].w, f4.w, q);
                  if (write && gf) gp[k * LP] = make_float4(wj * g4[k].x, wj * g4[k].y, wj * g4[k].z, wj * g4[k].w);
                }
            }
            q = group_sum(q, LP);
            const float t = __shfl(q, (lane & (spw - 1)) * LP, 64);  // sample j0 + s sits in the lanes [s LP, (s+1) LP)
            if ((lane & ~(spw - 1)) == j0) qs = t;
          }
        } else if (live) {
          for (int ch = 0; ch < C; ++ch) {
            const float g = gF[ray * C + ch];
            qs = fmaf(g, feat[i * C + ch], qs);
            if (write && gf) gf[i * C + ch] = w * g;
          }
        }
        G += qs;
      }
      return live ? G : 0.f;
    };

    if (MODE == kWeights) {
      for (int64_t i0 = sb; i0 < se; i0 += 64) {
        const int64_t i = i0 + lane;
        const int cnt = (int)(se - i0 < 64 ? se - i0 : 64);
        const float w = i < se ? x[i] : 0.f;
        const float G = upstream(i0, cnt, w, true);
        if (gx && i < se) gx[i] = G;
      }
      continue;
    }

    // the forward's carry into every chunk, lane c keeps chunk c's (chunks past 63 restart from chunk 63's); kAlpha: the
    // ray's first exact zero factor z (1 - alpha_z == 0), see below
    float saved = (MODE == kAlpha) ? 1.f : 0.f;
    int64_t z = n;
    {
      float carry = saved;
      for (int64_t ch = 0; ch < nchunk; ++ch) {
        if (lane == ch) saved = carry;
        const int64_t i = sb + ch * 64 + lane;
        const bool live = i < se;
        if (MODE == kAlpha) {
          const float step = live ? 1.f - x[i] : 1.f;
          const unsigned long long m = __ballot(live && step == 0.f);
          if (z == n && m) z = ch * 64 + __ffsll(m) - 1;
          carry *= wscan::last(wscan::incl<wscan::Mul>(step, lane));
        } else {
          const float step = live ? x[i] * (te[i] - ts[i]) : 0.f;
          carry += wscan::last(wscan::incl<wscan::Add>(step, lane));
        }
      }
    }
    // kAlpha, alpha_z == 1 exactly: every T_k behind z is 0, so the division of the suffix sum by 1 - alpha_z cannot recover
    //   -T_z sum_{k>z} (G_k alpha_k + gT_k) prod_{z<j<k} (1 - alpha_j)
    // that torch's cumprod backward keeps (composite.hip: weights_bwd_kernel); it comes from a product scan restarted at z
    float zsum = 0.f;
    if (MODE == kAlpha && z + 1 < n) {
      float pc = 1.f;
      for (int64_t ch = (z + 1) / 64; ch < nchunk; ++ch) {
        const int64_t s = ch * 64 + lane, i = sb + s;
        const bool in = s > z && s < n;
        const int cnt = (int)(n - ch * 64 < 64 ? n - ch * 64 : 64);
        const float alpha = in ? x[i] : 0.f;
        const float incl = wscan::incl<wscan::Mul>(1.f - alpha, lane);
        const float P = pc * wscan::shift_up1(incl, 1.f, lane);
        pc *= wscan::last(incl);
        const float G = upstream(sb + ch * 64, cnt, 0.f, false);
        const float Gk = in ? G * alpha + (gT ? gT[i] : 0.f) : 0.f;
        zsum += wscan::reduce<wscan::Add>(Gk * P);
      }
    }
    float suffix = 0.f;  // sum over the samples of later chunks
    for (int64_t ch = nchunk - 1; ch >= 0; --ch) {
      float carry = __shfl(saved, (int)(ch < 63 ? ch : 63), 64);
      for (int64_t p = 63; p < ch; ++p) {  // rays longer than 4096 samples: walk on from chunk 63
        const int64_t i = sb + p * 64 + lane;
        if (MODE == kAlpha) carry *= wscan::last(wscan::incl<wscan::Mul>(1.f - x[i], lane));
        else carry += wscan::last(wscan::incl<wscan::Add>(x[i] * (te[i] - ts[i]), lane));
      }
      const int64_t s = ch * 64 + lane, i = sb + s;
      const bool live = s < n;
      const int cnt = (int)(n - ch * 64 < 64 ? n - ch * 64 : 64);
      float alpha, step, delta = 1.f, T;
      if (MODE == kAlpha) {
        alpha = live ? x[i] : 0.f;
        step = 1.f - alpha;
        const float incl = wscan::incl<wscan::Mul>(step, lane);
        T = carry * wscan::shift_up1(incl, 1.f, lane);
      } else {
        delta = live ? te[i] - ts[i] : 0.f;
        step = live ? x[i] * delta : 0.f;
        alpha = 1.f - expf(-step);
        const float incl = wscan::incl<wscan::Add>(step, lane);
        T = expf(-(carry + wscan::shift_up1(incl, 0.f, lane)));
      }
      const float G = upstream(sb + ch * 64, cnt, live ? alpha * T : 0.f, true);
      const float gti = (MODE == kAlpha && gT && live) ? gT[i] : 0.f;
      const float term = live ? (G * alpha + gti) * T : 0.f;  // G_k w_k + gT_k T_k
      const float incl_r = wscan::rincl<wscan::Add>(term, lane);
      const float after = wscan::shift_down1(incl_r, 0.f, lane) + suffix;  // sum_{k>i}
      if (live && gx) {
        float g;
        if (MODE == kAlpha) {
          g = G * T - after / fmaxf(1.f - alpha, 1e-10f);
          if (s == z) g -= T * zsum;
        } else {
          g = (G * T * expf(-step) - after) * delta;
        }
        gx[i] = g;
      }
      suffix += wscan::first(incl_r);
    }
  }
}

// lower bound of every ray id in the sorted ray_indices: seg[r] = #{i : ray_indices[i] < r}, r in [0, R]
__global__ __launch_bounds__(256) void segments_kernel(const int64_t* __restrict__ ri, int64_t M, int64_t R,
                                                       int64_t* __restrict__ seg) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r <= R; r += (int64_t)gridDim.x * 256) {
    int64_t lo = 0, hi = M;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (ri[mid] < r) lo = mid + 1;
      else hi = mid;
    }
    seg[r] = lo;
  }
}

}  // namespace packed
}  // namespace nrhip
