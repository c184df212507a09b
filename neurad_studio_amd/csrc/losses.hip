// SURVEY §8(f) row 2 -- the losses that consume the sampler outputs every training step:
//   zipnerf_interlevel_loss (model_components/losses.py:645-705) and distortion_loss (losses.py:137-156).
// The reference evaluates each with ~40 small torch kernels per proposal level (sort, two cumsums, searchsorted,
// five take_along_dims ...) on [R, 68] / [R, 129] tensors.  Here one wavefront owns one ray: the 2(Sf+1) blurred
// step-function knots never leave LDS, the "sort" is a merge of two already sorted sequences (c - r and c + r),
// the three prefix sums are wave scans, and the gradient w.r.t. the proposal weights (the only input that carries
// one: the fine histogram is detached, losses.py:678-679) is produced in the same pass.
// The prefix sums accumulate in fp64 and round every prefix to fp32, exactly what torch's CPU cumsum does for fp32
// (at::acc_type<float> = double); a plain fp32 scan lands 1e-4 away after the division by (w_p + 1e-5).
#include "common.h"
#include "wave_scan.h"

namespace nrhip {
namespace {

constexpr int kMaxFine = 128;                   // fine (field) samples per ray
constexpr int kMaxProp = 512;                   // proposal samples per ray
constexpr int kKnots = 2 * (kMaxFine + 1) + 2;  // blurred knots incl. the 0 / 1 padding
constexpr int kRaysPerBlock = 4;

// One ray's scratch, carved out of dynamic LDS for the launch's actual sample counts: sized for the maxima (6.2 KB per ray)
// the four rays of a workgroup held the CU at 6 workgroups = 24 of its 32 waves; NeuRAD's 32 fine / 128 proposal samples
// need 1.6 KB.
struct RayLds {
  float* c;    // [sf + 1]
  float* wn;   // [sf + 1]      w / (c[i+1] - c[i]), then y1
  float* x;    // [2 sf + 4]    c_  (padded knots)
  float* y;    // [2 sf + 4]    w_  (padded blurred pdf)
  float* cdf;  // [2 sf + 4]    padded cdf
  float* v;    // [sp + 1]      cdf interpolated at the proposal edges
};
__host__ __device__ constexpr int ray_lds_floats(int sf, int sp) { return 2 * (sf + 1) + 3 * (2 * sf + 4) + (sp + 1); }

// wave-wide sums / scans on DPP row shifts + readlane (wave_scan.h): the fp64 scans below were six dependent pairs of
// ds_bpermute each as shuffles, three times per ray and chunk
__device__ __forceinline__ double wave_sum_d(double v) { return wscan::reduce<wscan::Add>(v); }
__device__ __forceinline__ float wave_sum_f(float v) { return wscan::reduce<wscan::Add>(v); }
// torch's clamp_min(0): a NaN stays a NaN (fmaxf would return the 0 and hide an inf - inf of a fine bin without width)
__device__ __forceinline__ float clamp_min0(float v) { return v < 0.f ? 0.f : v; }
// inclusive prefix sum of arr[0..n) in place: fp64 accumulation, every prefix rounded to fp32 (see header)
__device__ __forceinline__ void scan_inplace(float* arr, int n, int lane) {
  double carry = 0.0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    double v = wscan::incl<wscan::Add>(i < n ? (double)arr[i] : 0.0, lane);
    v += carry;
    if (i < n) arr[i] = (float)v;
    carry = wscan::last(v);
  }
}

__global__ __launch_bounds__(64 * kRaysPerBlock) void interlevel_loss_kernel(
    const float* __restrict__ c_all, const float* __restrict__ w_all, int sf, const float* __restrict__ cp_all,
    const float* __restrict__ wp_all, int sp, float r, int64_t R, float* __restrict__ loss, float* __restrict__ gwp) {
  extern __shared__ float lds_dyn[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * kRaysPerBlock + wid;
  if (ray >= R) return;
  RayLds L;
  L.c = lds_dyn + wid * ray_lds_floats(sf, sp);
  L.wn = L.c + (sf + 1);
  L.x = L.wn + (sf + 1);
  L.y = L.x + (2 * sf + 4);
  L.cdf = L.y + (2 * sf + 4);
  L.v = L.cdf + (2 * sf + 4);
  const float* c = c_all + ray * (sf + 1);
  const float* w = w_all + ray * sf;
  // ---- fine histogram: last weight absorbs the missing mass, heights = weight / width (losses.py:680-683) ------
  float acc = 0.f;
  for (int i = lane; i < sf; i += 64) acc += w[i];
  acc = wave_sum_f(acc);
  for (int i = lane; i <= sf; i += 64) L.c[i] = c[i];
  wave_fence();
  for (int i = lane; i < sf; i += 64) {
    const float wi = w[i] + (i == sf - 1 ? 1.f - acc : 0.f);
    L.wn[i] = wi / (L.c[i + 1] - L.c[i]);
  }
  if (lane == 0) L.wn[sf] = 0.f;
  wave_fence();
  // ---- _blur_stepfun (losses.py:645-653): knots = merge of (c - r) and (c + r); y2 = +-y1 in knot order ---------
  const int n1 = sf + 1, M = 2 * n1;
  float* xr = L.x + 1;   // knot m of the merge at xr[m]; x[0] / x[M+1] are the 0 / 1 padding
  float* y2 = L.y + 1;   // y2[m], later yr[m] shifted by one
  for (int k = lane; k < n1; k += 64) {
    const float y1 = (L.wn[k] - (k > 0 ? L.wn[k - 1] : 0.f)) / (2.f * r);
    const float a = L.c[k] - r, b = L.c[k] + r;
    int pa = k, pb = k;  // stable merge: ties keep the (c - r) element first
    for (int q = 0; q < n1; ++q) {
      pa += (L.c[q] + r < a) ? 1 : 0;
      pb += (L.c[q] - r <= b) ? 1 : 0;
    }
    xr[pa] = a, xr[pb] = b;
    L.cdf[pa] = y1, L.cdf[pb] = -y1;  // cdf[] is free until the third scan: y2 in knot order
  }
  wave_fence();
  // inner cumsum over y2[0..M-2]
  scan_inplace(L.cdf, M - 1, lane);
  wave_fence();
  // yr_inc[m] = cumsum((xr[m+1] - xr[m]) * inner[m]), clamp_min(0); yr = [0, yr_inc]
  for (int m = lane; m < M - 1; m += 64) y2[m + 1] = (xr[m + 1] - xr[m]) * L.cdf[m];
  wave_fence();
  scan_inplace(y2 + 1, M - 1, lane);
  wave_fence();
  for (int m = lane; m < M - 1; m += 64) y2[m + 1] = clamp_min0(y2[m + 1]);
  if (lane == 0) y2[0] = 0.f;  // yr[0]
  wave_fence();
  // ---- piecewise-linear pdf -> piecewise-quadratic cdf (losses.py:691-693), then the 0 / 1 padding (695-698) -----
  float* cdf = L.cdf + 1;
  for (int m = lane; m < M - 1; m += 64) cdf[m + 1] = 0.5f * (y2[m + 1] + y2[m]) * (xr[m + 1] - xr[m]);
  wave_fence();
  scan_inplace(cdf + 1, M - 1, lane);
  if (lane == 0) {
    cdf[0] = 0.f;
    L.x[0] = 0.f, L.y[0] = 0.f, L.cdf[0] = 0.f;
    L.x[M + 1] = 1.f, L.y[M + 1] = 0.f, L.cdf[M + 1] = 1.f;
  }
  wave_fence();
  // ---- _sorted_interp_quad at the proposal edges (losses.py:656-669) ------------------------------------------
  const int K = M + 2;
  const float* cp = cp_all + ray * (sp + 1);
  for (int k = lane; k <= sp; k += 64) {
    const float x = cp[k];
    int lo = 0, hi = K;  // first index with c_[idx] >= x  (torch.searchsorted, right=False)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (L.x[mid] < x) lo = mid + 1; else hi = mid;
    }
    const int left = lo > 0 ? lo - 1 : 0, right = lo < K - 1 ? lo : K - 1;
    const float xp0 = L.x[left], xp1 = L.x[right], f0 = L.y[left], f1 = L.y[right], c0 = L.cdf[left];
    float off = (x - xp0) / (xp1 - xp0);
    off = (off != off) ? 0.f : fminf(fmaxf(off, 0.f), 1.f);  // nan_to_num(nan -> 0), clip to [0, 1] (inf -> 1)
    L.v[k] = c0 + (x - xp0) * (f0 + f1 * off + f0 * (1.f - off)) * 0.5f;
  }
  wave_fence();
  // ---- loss and its gradient w.r.t. the proposal weights (losses.py:703-704) -----------------------------------
  const float* wp = wp_all + ray * sp;
  float part = 0.f;
  for (int k = lane; k < sp; k += 64) {
    const float ws = L.v[k + 1] - L.v[k];
    const float p = wp[k], den = p + 1e-5f;
    const float d = clamp_min0(ws - p);
    part += d * d / den;
    if (gwp) gwp[ray * sp + k] = -(2.f * d / den + d * d / (den * den));
  }
  part = wave_sum_f(part);
  if (lane == 0) loss[ray] = part;
}

// lossfun_distortion (losses.py:137-148): loss = sum_i w_i sum_j w_j |u_i - u_j| + sum_i w_i^2 delta_i / 3
__global__ __launch_bounds__(64 * kRaysPerBlock) void distortion_loss_kernel(const float* __restrict__ c_all,
                                                                             const float* __restrict__ w_all, int s,
                                                                             int64_t R, float* __restrict__ loss,
                                                                             float* __restrict__ gw) {
  __shared__ float u_all[kRaysPerBlock][kMaxProp], w_lds[kRaysPerBlock][kMaxProp];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * kRaysPerBlock + wid;
  if (ray >= R) return;
  const float* c = c_all + ray * (s + 1);
  const float* w = w_all + ray * s;
  float* u = u_all[wid];
  float* wl = w_lds[wid];
  for (int i = lane; i < s; i += 64) u[i] = (c[i + 1] + c[i]) / 2.f, wl[i] = w[i];
  wave_fence();
  float part = 0.f;
  for (int i = lane; i < s; i += 64) {
    float inner = 0.f;
    for (int j = 0; j < s; ++j) inner += wl[j] * fabsf(u[i] - u[j]);
    const float wi = wl[i], delta = c[i + 1] - c[i];
    part += wi * inner + wi * wi * delta / 3.f;
    if (gw) gw[ray * s + i] = 2.f * inner + (2.f / 3.f) * wi * delta;
  }
  part = wave_sum_f(part);
  if (lane == 0) loss[ray] = part;
}

}  // namespace

// ---- carving: NeuRADModel._compute_is_close_to_lidar (models/neurad.py:677-700) and the proposal
// carving term sum((w * (is_lidar & ~close))^2) (models/neurad.py:399-408) ------------------------------------------------
// The reference spends ~7 elementwise ops per sample level on the mask and ~6 more (with autograd) on each loss term; here
// one pass per level writes the mask and, when weights are given, the per-ray loss and its gradient 2 w far.
__global__ __launch_bounds__(256) void lidar_carving_kernel(const float* __restrict__ starts,
                                                            const float* __restrict__ ends, int stride,
                                                            const float* __restrict__ weights,
                                                            const uint8_t* __restrict__ is_lidar,
                                                            const uint8_t* __restrict__ did_return,
                                                            const float* __restrict__ dist, float eps, float non_return,
                                                            int64_t R, int S, uint8_t* __restrict__ is_close,
                                                            float* __restrict__ loss_ray, float* __restrict__ grad_w) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= R) return;
  const bool lidar = is_lidar[ray] != 0;
  const bool returned = did_return ? did_return[ray] != 0 : true;
  const float dr = dist[ray];
  float acc = 0.f;
  for (int s = lane; s < S; s += 64) {
    const float mid = (starts[ray * stride + s] + ends[ray * stride + s]) * 0.5f;
    const bool close = lidar && (returned ? fabsf(dr - mid) < eps : mid < non_return);
    if (is_close) is_close[ray * S + s] = close ? 1 : 0;
    if (weights) {
      const float wf = (lidar && !close) ? weights[ray * S + s] : 0.f;
      acc += wf * wf;
      if (grad_w) grad_w[ray * S + s] = 2.f * wf;
    }
  }
  if (loss_ray) {
    acc = wave_sum_f(acc);
    if (lane == 0) loss_ray[ray] = acc;
  }
}

// ---- the same two per-sample terms on PACKED (occupancy-marched) samples: ray r owns the samples [seg[r], seg[r+1]) of
// the [M]-shaped arrays, one wavefront walks one ray in chunks of 64 with a carried prefix, rays are handed out grid-stride
// over a capped grid (the contract of packed_composite.h: no atomics, no LDS, nothing allocated, one writer per element, an
// empty segment writes 0 to its ray's row).  The contracts and their error bounds: include/neurad_hip.h.
namespace {

constexpr int kPackedMaxBlocks = 4096;  // grid cap: 16 384 waves, the rest of the rays grid-stride
inline int packed_blocks_for(int64_t r) {
  const int64_t b = (r + kRaysPerBlock - 1) / kRaysPerBlock;
  return (int)(b < kPackedMaxBlocks ? b : kPackedMaxBlocks);
}
// a ray's segment, clamped into [0, M]: broken segments read inside the arrays
__device__ __forceinline__ void packed_segment(const int64_t* __restrict__ seg, int64_t ray, int64_t M, int64_t& sb,
                                               int64_t& se) {
  sb = seg[ray], se = seg[ray + 1];
  sb = sb < 0 ? 0 : (sb > M ? M : sb);
  se = se < sb ? sb : (se > M ? M : se);
}

// One chunk of a ray for the distortion loss, lane = sample, everything in float64 from the fp32 inputs: the sample's
// weight, midpoint and width, and the sums over the EARLIER samples of the ray A = sum w_j, B = sum w_j m_j (the chunk's
// exclusive prefix on top of the carry, taken by a shift of the inclusive scan: no own term is subtracted back out).
struct DistChunk {
  double w, m, d, A, B;
};
__device__ __forceinline__ DistChunk dist_chunk(const float* __restrict__ s, const float* __restrict__ e,
                                                const float* __restrict__ w, int64_t i, bool live, int lane, double& cA,
                                                double& cB) {
  DistChunk c;
  c.w = live ? (double)w[i] : 0.0;
  const double si = live ? (double)s[i] : 0.0, ei = live ? (double)e[i] : 0.0;
  c.m = (si + ei) * 0.5, c.d = ei - si;  // both exact: fp32 inputs
  const double inA = wscan::incl<wscan::Add>(c.w, lane), inB = wscan::incl<wscan::Add>(c.w * c.m, lane);
  c.A = cA + wscan::shift_up1(inA, 0.0, lane), c.B = cB + wscan::shift_up1(inB, 0.0, lane);
  cA += wscan::last(inA), cB += wscan::last(inB);
  return c;
}
// d loss / d w_k: the samples before k weigh m_k - m_j, those behind it m_j - m_k, with W / Bt the ray's totals of A / B
__device__ __forceinline__ float dist_grad(const DistChunk& c, double W, double Bt) {
  return (float)(2.0 * (c.m * (c.A - (W - c.A - c.w)) - (c.B - (Bt - c.B - c.w * c.m))) + (2.0 / 3.0) * c.w * c.d);
}

// Distortion loss of packed samples in its O(n) form (sorted midpoints: |m_i - m_j| = m_i - m_j for j < i):
//   loss = 2 sum_i w_i (m_i A_i - B_i) + sum_i w_i^2 delta_i / 3
// The gradient needs the ray's totals before any sample's value, so it takes TWO WALKS of the segment: the first gives the
// loss and the totals, the second (the same scans on the same data, so the same prefixes bit for bit; its reads hit the
// cache lines the first walk brought in) writes the gradient.  A ray of at most 64 samples has its totals after its only
// chunk and writes the gradient in the first walk.  Without grad_w there is one walk.
__global__ __launch_bounds__(64 * kRaysPerBlock) void packed_distortion_loss_kernel(
    const float* __restrict__ s, const float* __restrict__ e, const float* __restrict__ w, const int64_t* __restrict__ seg,
    int64_t R, int64_t M, float* __restrict__ loss, float* __restrict__ gw) {
  const int lane = threadIdx.x & 63;
  for (int64_t ray = (int64_t)blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6); ray < R;
       ray += (int64_t)gridDim.x * kRaysPerBlock) {
    int64_t sb, se;
    packed_segment(seg, ray, M, sb, se);
    const bool single = se - sb <= 64;
    double cA = 0.0, cB = 0.0, inter = 0.0, intra = 0.0;
    for (int64_t i0 = sb; i0 < se; i0 += 64) {
      const int64_t i = i0 + lane;
      const bool live = i < se;
      const DistChunk c = dist_chunk(s, e, w, i, live, lane, cA, cB);
      inter += c.w * (c.m * c.A - c.B);  // a dead lane: w = 0
      intra += c.w * c.w * c.d;
      if (gw && single && live) gw[i] = dist_grad(c, cA, cB);
    }
    const double total = 2.0 * wscan::reduce<wscan::Add>(inter) + wscan::reduce<wscan::Add>(intra) / 3.0;
    if (lane == 0) loss[ray] = (float)total;
    if (gw && !single) {
      const double W = cA, Bt = cB;
      cA = 0.0, cB = 0.0;
      for (int64_t i0 = sb; i0 < se; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool live = i < se;
        const DistChunk c = dist_chunk(s, e, w, i, live, lane, cA, cB);
        if (live) gw[i] = dist_grad(c, W, Bt);
      }
    }
  }
}

// lidar_carving_kernel on packed samples: the same mask, bit for bit; the squares are summed in float64.  A camera ray
// reads no sample: its mask and gradient are zeros whatever the samples hold.
__global__ __launch_bounds__(64 * kRaysPerBlock) void packed_lidar_carving_kernel(
    const float* __restrict__ ts, const float* __restrict__ te, const float* __restrict__ weights,
    const int64_t* __restrict__ seg, const uint8_t* __restrict__ is_lidar, const uint8_t* __restrict__ did_return,
    const float* __restrict__ dist, float eps, float non_return, int64_t R, int64_t M, uint8_t* __restrict__ is_close,
    float* __restrict__ loss_ray, float* __restrict__ grad_w) {
  const int lane = threadIdx.x & 63;
  for (int64_t ray = (int64_t)blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6); ray < R;
       ray += (int64_t)gridDim.x * kRaysPerBlock) {
    int64_t sb, se;
    packed_segment(seg, ray, M, sb, se);
    const bool lidar = is_lidar[ray] != 0;
    const bool returned = did_return ? did_return[ray] != 0 : true;
    const float dr = dist[ray];
    double acc = 0.0;
    for (int64_t i = sb + lane; i < se; i += 64) {
      bool close = false;
      float wf = 0.f;
      if (lidar) {
        const float mid = (ts[i] + te[i]) * 0.5f;
        close = returned ? fabsf(dr - mid) < eps : mid < non_return;
        if (weights && !close) wf = weights[i];
      }
      if (is_close) is_close[i] = close ? 1 : 0;
      acc += (double)wf * (double)wf;  // exact: 48 bits
      if (grad_w) grad_w[i] = 2.f * wf;
    }
    if (loss_ray) {
      acc = wave_sum_d(acc);
      if (lane == 0) loss_ray[ray] = (float)acc;
    }
  }
}

// the argument checks the two packed entry points share; *launch: there are rays to run
int packed_loss_args(const char* who, int64_t r, int64_t m, const void* segments, bool* launch) {
  *launch = false;
  NR_REQUIRE(r >= 0 && m >= 0, NRHIP_ERR_INVALID_ARG, "%s: negative ray or sample count", who);
  NR_REQUIRE(m < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "%s: M >= 2^31", who);
  if (r == 0) return NRHIP_OK;  // no rays: empty tensors have no address
  NR_REQUIRE(segments, NRHIP_ERR_INVALID_ARG, "%s: segments is NULL", who);
  *launch = true;
  return NRHIP_OK;
}

}  // namespace
}  // namespace nrhip

using namespace nrhip;

extern "C" int nrhip_interlevel_loss(const float* c, const float* w, int32_t n_fine, const float* cp, const float* wp,
                                     int32_t n_prop, float pulse_width, int64_t r, float* loss_per_ray, float* grad_wp,
                                     void* stream) {
  NR_REQUIRE(r >= 0 && n_fine >= 1 && n_prop >= 1 && pulse_width > 0.f, NRHIP_ERR_INVALID_ARG,
             "interlevel_loss: bad argument");
  NR_REQUIRE(n_fine <= kMaxFine && n_prop <= kMaxProp, NRHIP_ERR_UNSUPPORTED,
             "interlevel_loss: %d fine / %d proposal samples per ray exceed %d / %d", n_fine, n_prop, kMaxFine, kMaxProp);
  if (r == 0) return NRHIP_OK;
  NR_REQUIRE(c && w && cp && wp && loss_per_ray, NRHIP_ERR_INVALID_ARG, "interlevel_loss: null pointer");
  interlevel_loss_kernel<<<(unsigned)((r + kRaysPerBlock - 1) / kRaysPerBlock), 64 * kRaysPerBlock,
                           (size_t)kRaysPerBlock * ray_lds_floats(n_fine, n_prop) * sizeof(float), (hipStream_t)stream>>>(c, w, n_fine, cp, wp, n_prop, pulse_width, r, loss_per_ray, grad_wp);
  return check_launch("interlevel_loss");
}

extern "C" int nrhip_distortion_loss(const float* c, const float* w, int32_t n_samples, int64_t r, float* loss_per_ray,
                                     float* grad_w, void* stream) {
  NR_REQUIRE(r >= 0 && n_samples >= 1, NRHIP_ERR_INVALID_ARG, "distortion_loss: bad argument");
  NR_REQUIRE(n_samples <= kMaxProp, NRHIP_ERR_UNSUPPORTED, "distortion_loss: %d samples per ray exceed %d", n_samples,
             kMaxProp);
  if (r == 0) return NRHIP_OK;
  NR_REQUIRE(c && w && loss_per_ray, NRHIP_ERR_INVALID_ARG, "distortion_loss: null pointer");
  distortion_loss_kernel<<<(unsigned)((r + kRaysPerBlock - 1) / kRaysPerBlock), 64 * kRaysPerBlock, 0,
                           (hipStream_t)stream>>>(c, w, n_samples, r, loss_per_ray, grad_w);
  return check_launch("distortion_loss");
}

extern "C" int nrhip_lidar_carving(const float* starts, const float* ends, int32_t sample_stride, const float* weights,
                                   const uint8_t* is_lidar, const uint8_t* did_return, const float* distance,
                                   float carving_epsilon, float non_return_lidar_distance, int64_t r, int32_t s,
                                   uint8_t* is_close, float* loss_per_ray, float* grad_weights, void* stream) {
  NR_REQUIRE(r >= 0 && s >= 0, NRHIP_ERR_INVALID_ARG, "lidar_carving: bad argument");
  if (r == 0) return NRHIP_OK;  // no rays: empty tensors have no address
  NR_REQUIRE(starts && ends && is_lidar && distance && (is_close || loss_per_ray || grad_weights), NRHIP_ERR_INVALID_ARG,
             "lidar_carving: bad argument");
  NR_REQUIRE(weights || (!loss_per_ray && !grad_weights), NRHIP_ERR_INVALID_ARG, "lidar_carving: the loss needs the weights");
  nrhip::lidar_carving_kernel<<<(int)((r + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      starts, ends, sample_stride > 0 ? sample_stride : s, weights, is_lidar, did_return, distance, carving_epsilon,
      non_return_lidar_distance, r, s, is_close, loss_per_ray, grad_weights);
  return nrhip::check_launch("lidar_carving");
}

extern "C" int nrhip_packed_distortion_loss(const float* s_starts, const float* s_ends, const float* weights,
                                            const int64_t* segments, int64_t r, int64_t m, float* loss_per_ray,
                                            float* grad_w, void* stream) {
  bool launch;
  if (int rc = packed_loss_args("packed_distortion_loss", r, m, segments, &launch)) return rc;
  if (!launch) return NRHIP_OK;
  NR_REQUIRE(loss_per_ray, NRHIP_ERR_INVALID_ARG, "packed_distortion_loss: loss_per_ray is NULL");
  NR_REQUIRE(m == 0 || (s_starts && s_ends && weights), NRHIP_ERR_INVALID_ARG,
             "packed_distortion_loss: NULL sample pointer with %lld samples", (long long)m);
  packed_distortion_loss_kernel<<<packed_blocks_for(r), 64 * kRaysPerBlock, 0, (hipStream_t)stream>>>(
      s_starts, s_ends, weights, segments, r, m, loss_per_ray, grad_w);
  return check_launch("packed_distortion_loss");
}

extern "C" int nrhip_packed_lidar_carving(const float* t_starts, const float* t_ends, const float* weights,
                                          const int64_t* segments, const uint8_t* is_lidar, const uint8_t* did_return,
                                          const float* distance, float carving_epsilon, float non_return_lidar_distance,
                                          int64_t r, int64_t m, uint8_t* is_close, float* loss_per_ray,
                                          float* grad_weights, void* stream) {
  bool launch;
  if (int rc = packed_loss_args("packed_lidar_carving", r, m, segments, &launch)) return rc;
  if (!launch) return NRHIP_OK;
  NR_REQUIRE(is_lidar && distance, NRHIP_ERR_INVALID_ARG, "packed_lidar_carving: is_lidar or distance is NULL");
  NR_REQUIRE(is_close || loss_per_ray || grad_weights, NRHIP_ERR_INVALID_ARG, "packed_lidar_carving: no output (NULL)");
  NR_REQUIRE(m == 0 || (t_starts && t_ends), NRHIP_ERR_INVALID_ARG,
             "packed_lidar_carving: NULL sample pointer with %lld samples", (long long)m);
  NR_REQUIRE(m == 0 || weights || (!loss_per_ray && !grad_weights), NRHIP_ERR_INVALID_ARG,
             "packed_lidar_carving: the loss needs the weights (NULL)");
  packed_lidar_carving_kernel<<<packed_blocks_for(r), 64 * kRaysPerBlock, 0, (hipStream_t)stream>>>(
      t_starts, t_ends, weights, segments, is_lidar, did_return, distance, carving_epsilon, non_return_lidar_distance, r, m,
      is_close, loss_per_ray, grad_weights);
  return check_launch("packed_lidar_carving");
}
