// Packed (ragged) compositing for the occupancy-marched samples of occgrid.hip: nerfacc's packed render_weight_from_alpha /
// render_weight_from_density / accumulate_along_rays and their fusion, forward and backward.
// `seg` is int64 [R+1]: ray r owns the packed samples [seg[r], seg[r+1]).  Owner-computes: one wavefront walks one ray in
// chunks of 64 samples with a carried prefix (the structure of the dense kernels of composite.hip, same arithmetic), rays
// are handed out grid-stride over a capped grid.  No atomics (bitwise reproducible), no LDS, nothing allocated.  The same
// structure carries the training node's head + compositing (head_fwd_kernel / head_bwd_kernel at the end of the file).
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

// sum_j w_j f_j over one chunk of a ray (cnt live samples from i0, lane = sample, w = its weight; 0 on a dead lane).  Vector
// path: into the running float4 rows `fa`; generic C: one wave reduction per channel, the row's running sum lives in `of`
// (owner-only, in order; the ray's first chunk, i0 == sb, starts it)
__device__ __forceinline__ void accumulate_rows(const float* __restrict__ feat, float* __restrict__ of, int64_t ray,
                                                int64_t sb, int64_t i0, int cnt, float w, int C, int LP, int K, int lane,
                                                float4 (&fa)[kMaxK]) {
  const int sub = lane & (LP - 1), sl = lane / LP, spw = 64 / LP;
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
    const bool live = lane < cnt;
    for (int ch = 0; ch < C; ++ch) {
      const float p = wscan::reduce<wscan::Add>(live ? w * feat[(i0 + lane) * C + ch] : 0.f);
      if (lane == 0) of[ray * C + ch] = (i0 == sb ? 0.f : of[ray * C + ch]) + p;
    }
  }
}

// the ray's row of `of` once its chunks are through: the class sums of `fa` (vector path), zeros for an empty segment
// (generic C: a ray with samples has its row in place already)
__device__ __forceinline__ void store_rows(float* __restrict__ of, int64_t ray, bool empty, int C, int LP, int K, int lane,
                                           const float4 (&fa)[kMaxK]) {
  if (K > 0) {
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) {
        float4 v = fa[k];
        v.x = class_sum(v.x, LP), v.y = class_sum(v.y, LP), v.z = class_sum(v.z, LP), v.w = class_sum(v.w, LP);
        if (lane < LP) reinterpret_cast<float4*>(of + ray * C)[(lane & (LP - 1)) + k * LP] = v;
      }
  } else if (empty) {
    for (int ch = lane; ch < C; ch += 64) of[ray * C + ch] = 0.f;
  }
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
      if (of) accumulate_rows(feat, of, ray, sb, i0, (int)(se - i0 < 64 ? se - i0 : 64), w, C, LP, K, lane, fa);
    }
    if (of) store_rows(of, ray, sb >= se, C, LP, K, lane, fa);
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

// What reaches the weights of one chunk of `ray` from the per-ray and per-sample cotangents (bwd_kernel: G), lane = sample:
// the chunk starts at i0 with cnt live samples, g4 = the ray's row of gF (vector path), ga / gd its gA / gD.  With `write`,
// the chunk's rows of gf = w gF.  feat == NULL: no feature term (and gF, gf are not touched).
__device__ __forceinline__ float upstream_of_chunk(const float* __restrict__ ts, const float* __restrict__ te,
                                                   const float* __restrict__ feat, const float* __restrict__ gF,
                                                   const float* __restrict__ gW, float* __restrict__ gf, int64_t ray,
                                                   int C, int LP, int K, const float4 (&g4)[kMaxK], float ga, float gd,
                                                   bool has_gd, int64_t i0, int cnt, float w, bool write, int lane) {
  const int sub = lane & (LP - 1), sl = lane / LP, spw = 64 / LP;
  const int64_t i = i0 + lane;
  const bool live = lane < cnt;
  float G = ga;
  if (gW && live) G += gW[i];
  if (has_gd && live) G += gd * ((ts[i] + te[i]) / 2.f);
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
  const int sub = lane & (LP - 1);
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

    auto upstream = [&](int64_t i0, int cnt, float w, bool write) -> float {
      return upstream_of_chunk(ts, te, feat, gF, gW, gf, ray, C, LP, K, g4, ga, gd, gD != nullptr, i0, cnt, w, write, lane);
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

// ---- head + packed compositing (training: nrhip_sdf_render_packed_fwd / _bwd), the packed sibling of train_fused.hip's
// sdf_render kernels.  x [M] is the geometry MLP's first output; beta_ptr points at the RAW parameter on the device (no host
// read), NULL selects the density head:
//   SDF head      alpha = sigmoid(-x (|beta| + beta_min))
//   density head  alpha = 1 - exp(-trunc_exp(x) (te - ts))          (d trunc_exp = exp(clamp(x, -15, 15)))
// and the compositing is fwd_kernel<kAlpha>'s on those alphas -- no sky residual, depth over all samples, zeros for a ray
// without samples.  The alphas are an output: the backward starts from them.
__device__ __forceinline__ float head_alpha(float x, float delta, bool dens, float beta) {
  return dens ? -expm1f(-expf(x) * delta) : sigmoidf_(-x * beta);
}

__global__ __launch_bounds__(64 * kWaves) void head_fwd_kernel(const float* __restrict__ ts, const float* __restrict__ te,
                                                               const float* __restrict__ x,
                                                               const float* __restrict__ beta_ptr, float beta_min,
                                                               const float* __restrict__ feat,
                                                               const int64_t* __restrict__ seg, int64_t R, int C, int LP,
                                                               int K, float* __restrict__ oal, float* __restrict__ ow,
                                                               float* __restrict__ of, float* __restrict__ od,
                                                               float* __restrict__ oa) {
  const int lane = threadIdx.x & 63;
  const bool dens = beta_ptr == nullptr;
  const float beta = dens ? 0.f : fabsf(*beta_ptr) + beta_min;
  for (int64_t ray = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); ray < R; ray += (int64_t)gridDim.x * kWaves) {
    const int64_t sb = seg[ray], se = seg[ray + 1];
    float carry = 1.f, acc = 0.f, dep = 0.f;
    float4 fa[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) fa[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i0 = sb; i0 < se; i0 += 64) {
      const int64_t i = i0 + lane;
      const bool live = i < se;
      const float t0 = live ? ts[i] : 0.f, t1 = live ? te[i] : 0.f;
      const float alpha = live ? head_alpha(x[i], t1 - t0, dens, beta) : 0.f;
      const float incl = wscan::incl<wscan::Mul>(1.f - alpha, lane);
      const float w = alpha * (carry * wscan::shift_up1(incl, 1.f, lane));
      carry *= wscan::last(incl);
      if (live) {
        if (oal) oal[i] = alpha;
        if (ow) ow[i] = w;
      }
      acc += w;
      dep += w * ((t0 + t1) / 2.f);
      accumulate_rows(feat, of, ray, sb, i0, (int)(se - i0 < 64 ? se - i0 : 64), w, C, LP, K, lane, fa);
    }
    store_rows(of, ray, sb >= se, C, LP, K, lane, fa);
    acc = wscan::reduce<wscan::Add>(acc);
    dep = wscan::reduce<wscan::Add>(dep);
    if (lane == 0) {
      oa[ray] = acc;
      od[ray] = dep;
    }
  }
}

// Backward: bwd_kernel<kAlpha>'s suffix scan over the saved alphas, chained into the head.  (An alpha of exactly 1 needs
// no restarted product scan here: both heads multiply d alpha by 1 - alpha.)  gx [M] = d x, gf [M,C] = w gF, and d beta
// leaves as one partial per WAVE in gb_part [gridDim.x * kWaves] (its rays in grid-stride order: a function of R alone),
// summed in a fixed order by beta_reduce_kernel -- no atomics, bitwise reproducible.  feat == NULL: no gF upstream.
__global__ __launch_bounds__(64 * kWaves) void head_bwd_kernel(
    const float* __restrict__ ts, const float* __restrict__ te, const float* __restrict__ x,
    const float* __restrict__ beta_ptr, float beta_min, const float* __restrict__ al, const float* __restrict__ feat,
    const int64_t* __restrict__ seg, const float* __restrict__ gF, const float* __restrict__ gD,
    const float* __restrict__ gA, const float* __restrict__ gW, int64_t R, int C, int LP, int K, float* __restrict__ gx,
    float* __restrict__ gf, float* __restrict__ gb_part) {
  const int lane = threadIdx.x & 63;
  const int sub = lane & (LP - 1);
  const bool dens = beta_ptr == nullptr;
  const float beta = dens ? 0.f : fabsf(*beta_ptr) + beta_min;
  float gb = 0.f;
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
    // the forward's carry into every chunk, lane c keeps chunk c's (chunks past 63 restart from chunk 63's)
    float saved = 1.f;
    {
      float carry = 1.f;
      for (int64_t ch = 0; ch < nchunk; ++ch) {
        if (lane == ch) saved = carry;
        const int64_t i = sb + ch * 64 + lane;
        carry *= wscan::last(wscan::incl<wscan::Mul>(i < se ? 1.f - al[i] : 1.f, lane));
      }
    }
    float suffix = 0.f;  // sum over the samples of later chunks
    for (int64_t ch = nchunk - 1; ch >= 0; --ch) {
      float carry = __shfl(saved, (int)(ch < 63 ? ch : 63), 64);
      for (int64_t p = 63; p < ch; ++p)  // rays longer than 4096 samples: walk on from chunk 63 (full chunks)
        carry *= wscan::last(wscan::incl<wscan::Mul>(1.f - al[sb + p * 64 + lane], lane));
      const int64_t s = ch * 64 + lane, i = sb + s;
      const bool live = s < n;
      const int cnt = (int)(n - ch * 64 < 64 ? n - ch * 64 : 64);
      const float alpha = live ? al[i] : 0.f;
      const float incl = wscan::incl<wscan::Mul>(1.f - alpha, lane);
      const float T = carry * wscan::shift_up1(incl, 1.f, lane);
      const float G = upstream_of_chunk(ts, te, feat, gF, gW, gf, ray, C, LP, K, g4, ga, gd, gD != nullptr, sb + ch * 64, cnt,
                                        live ? alpha * T : 0.f, true, lane);
      const float term = live ? G * alpha * T : 0.f;
      const float incl_r = wscan::rincl<wscan::Add>(term, lane);
      const float after = wscan::shift_down1(incl_r, 0.f, lane) + suffix;  // sum_{k>i} G_k w_k
      if (live) {
        const float xi = x[i];
        if (dens) {
          // d sigma = delta (G T (1 - alpha) - after), then trunc_exp's backward
          const float gsig = (G * T * (1.f - alpha) - after) * (te[i] - ts[i]);
          gx[i] = gsig * expf(fminf(fmaxf(xi, -15.f), 15.f));
        } else {
          const float gal = G * T - after / fmaxf(1.f - alpha, 1e-10f);
          const float ds = gal * alpha * (1.f - alpha);  // sigmoid'(u), u = -x beta
          gx[i] = -ds * beta;
          gb -= ds * xi;
        }
      }
      suffix += wscan::first(incl_r);
    }
  }
  gb = wscan::reduce<wscan::Add>(gb);
  if (lane == 0) gb_part[blockIdx.x * kWaves + (threadIdx.x >> 6)] = gb;
}

// d beta = sign(beta) sum(partials): one wavefront, fixed summation order
__global__ __launch_bounds__(64) void beta_reduce_kernel(const float* __restrict__ part, int n,
                                                         const float* __restrict__ beta_ptr, float* __restrict__ out) {
  float t = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) t += part[i];
  t = wscan::reduce<wscan::Add>(t);
  if (threadIdx.x == 0) {
    const float b = *beta_ptr;
    out[0] = b > 0.f ? t : (b < 0.f ? -t : 0.f);  // d|b|/db = sign(b), 0 at 0 like torch
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
