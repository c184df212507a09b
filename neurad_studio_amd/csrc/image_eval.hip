// Camera image evaluation: PSNR and SSIM of two fp32 channel-last images [H, W, C], the camera half of
// NeuRADModel.get_image_metrics_and_images (models/neurad.py:568-587; there torchmetrics' PeakSignalNoiseRatio(data_range=1)
// and structural_similarity_index_measure with its defaults: reflect pad, a 15-channel grouped conv2d over five product
// images, two min/max reductions, a dozen elementwise passes, E[x^2] - mu^2 on values near 1).  Here:
//
//   stats_kernel      pass 1: both images once, kStatItems elements per workgroup.  The fp32 difference, squared and summed in
//                     float64 (per-workgroup partial in a slab), and min / max of each image (per-workgroup partials; fminf /
//                     fmaxf drop a NaN, the NaN itself travels in the squared error: NaN - x is NaN).
//   stats_final       one workgroup: the partials in a fixed order; psnr = 10 log10(D^2 n / sum) in float64, rounded once
//                     (+inf for identical images); R = max(max a - min a, max b - min b), c1 = (0.01 R)^2, c2 = (0.03 R)^2 in
//                     float64, rounded once each, left on the device for pass 2.
//   ssim_kernel       pass 2: a workgroup owns kT x kT windows of ONE channel (blockIdx.z).  It stages the (kT + 10)^2 halo
//                     of both images in LDS as SHIFTED values a - p, b - q (p, q: the halo's centre pixel, clamped into the
//                     image), runs the horizontal 11-tap pass over the five moments (a', b', a'^2, b'^2, a'b') into LDS and
//                     the vertical pass out of it, four vertically adjacent windows per lane from one sliding column.  The
//                     variances and the covariance do not depend on the shift, the means get it back: the cancellation of
//                     sum g x^2 - mu^2 is bounded by the local contrast, not by the pixel value.  Every tap sum is one fmaf
//                     chain in tap order 0..10 (tests/image_eval_refs.py emulates it and bounds it).  s goes to ssim_map
//                     where the caller gave one, and into a float64 per-workgroup partial.
//   ssim_final        one workgroup: the partials in a fixed order, divided by the window count, rounded once; NaN where
//                     pass 1 saw one (a NaN pixel also reaches every window over it by arithmetic).
//
// LDS: halo rows of kHalo = 42 floats, moment rows of kT = 32 floats.  In both passes a lane's index runs along x first, so the
// 32 lanes of a ds_read_b32 group read 32 consecutive dwords of one row -- every bank once, whatever the pitch; the
// vertical pass walks DOWN a column per lane, and the lanes of a group sit side by side in the row.  2 x 42^2 + 5 x 42 x 32
// floats = 40.1 KB: three workgroups per CU.
// No atomics, no host read, no allocation: graph-capturable on one stream, and the same inputs give the same bits.
// Both images constant (R = 0): c1 = c2 = 0 and every window is 0 / 0: ssim is NaN (the reference's 0 / 0 as well).
#include <cmath>

#include "common.h"

namespace nrhip {
namespace {

constexpr int kBlock = 256;
constexpr int kStatItems = NRHIP_IMAGE_STAT_ITEMS;  // elements per workgroup of pass 1: 16 rounds of 256 threads
constexpr int kT = NRHIP_SSIM_TILE;                 // windows per tile edge
constexpr int kTaps = 11;
constexpr int kHalo = kT + kTaps - 1;
constexpr int kRowsPerLane = 4;                     // vertically adjacent windows of one lane
static_assert(kT == 32 && kBlock == kT * (kT / kRowsPerLane), "one lane per column of four windows");

struct Taps {
  float g[kTaps];
};

// the 11-tap Gaussian, sigma 1.5, normalised in float64, each tap rounded to fp32 once
Taps gaussian_taps() {
  double e[kTaps], sum = 0.0;
  for (int i = 0; i < kTaps; ++i) {
    const double d = (double)(i - kTaps / 2) / 1.5;
    e[i] = std::exp(-d * d / 2.0), sum += e[i];
  }
  Taps t;
  for (int i = 0; i < kTaps; ++i) t.g[i] = (float)(e[i] / sum);
  return t;
}

// lanes by a fixed shuffle tree, then the four waves as ((w0 + w1) + w2) + w3: one order, every run
__device__ __forceinline__ double block_sum_fixed(double s, double* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = s;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
// (lo, hi) of the workgroup: minimum of lo, maximum of hi; fminf / fmaxf: a NaN is dropped
__device__ __forceinline__ void block_min_max(float& lo, float& hi, float* sh_lo, float* sh_hi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = fminf(lo, __shfl_down(lo, off, 64));
    hi = fmaxf(hi, __shfl_down(hi, off, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh_lo[wave] = lo, sh_hi[wave] = hi;
  __syncthreads();
  lo = fminf(fminf(sh_lo[0], sh_lo[1]), fminf(sh_lo[2], sh_lo[3]));
  hi = fmaxf(fmaxf(sh_hi[0], sh_hi[1]), fmaxf(sh_hi[2], sh_hi[3]));
}

// pass 1.  psum [nb] float64; RANGE: pmm [nb, 4] = min a, max a, min b, max b
template <bool RANGE>
__global__ __launch_bounds__(kBlock) void stats_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                       double* __restrict__ psum, float* __restrict__ pmm) {
  __shared__ double sh[4];
  __shared__ float sh_lo[4], sh_hi[4];
  const float inf = __uint_as_float(0x7f800000u);
  const int64_t base = (int64_t)blockIdx.x * kStatItems;
  double s = 0.0;
  float lo_a = inf, hi_a = -inf, lo_b = inf, hi_b = -inf;
#pragma unroll 4
  for (int k = 0; k < kStatItems / kBlock; ++k) {
    const int64_t i = base + k * kBlock + threadIdx.x;
    if (i < n) {
      const float x = a[i], y = b[i];
      const double d = (double)__fsub_rn(x, y);
      s += d * d;
      if (RANGE) lo_a = fminf(lo_a, x), hi_a = fmaxf(hi_a, x), lo_b = fminf(lo_b, y), hi_b = fmaxf(hi_b, y);
    }
  }
  const double bs = block_sum_fixed(s, sh);
  if (threadIdx.x == 0) psum[blockIdx.x] = bs;
  if (RANGE) {
    block_min_max(lo_a, hi_a, sh_lo, sh_hi);
    __syncthreads();
    block_min_max(lo_b, hi_b, sh_lo, sh_hi);
    if (threadIdx.x == 0) {
      float* o = pmm + (int64_t)blockIdx.x * 4;
      o[0] = lo_a, o[1] = hi_a, o[2] = lo_b, o[3] = hi_b;
    }
  }
}

// consts [4] (RANGE only): c1, c2, the squared-error sum as fp32 (NaN where an input was), unused
template <bool RANGE>
__global__ __launch_bounds__(kBlock) void stats_final_kernel(const double* __restrict__ psum, const float* __restrict__ pmm,
                                                             int nb, int64_t n, float psnr_range, float* __restrict__ psnr,
                                                             float* __restrict__ consts) {
  __shared__ double sh[4];
  __shared__ float sh_lo[4], sh_hi[4];
  const float inf = __uint_as_float(0x7f800000u);
  double s = 0.0;
  float lo_a = inf, hi_a = -inf, lo_b = inf, hi_b = -inf;
  for (int i = threadIdx.x; i < nb; i += kBlock) {
    s += psum[i];
    if (RANGE) {
      const float* m = pmm + (int64_t)i * 4;
      lo_a = fminf(lo_a, m[0]), hi_a = fmaxf(hi_a, m[1]), lo_b = fminf(lo_b, m[2]), hi_b = fmaxf(hi_b, m[3]);
    }
  }
  const double sse = block_sum_fixed(s, sh);
  if (RANGE) {
    block_min_max(lo_a, hi_a, sh_lo, sh_hi);
    __syncthreads();
    block_min_max(lo_b, hi_b, sh_lo, sh_hi);
  }
  if (threadIdx.x != 0) return;
  const double d = (double)psnr_range;
  *psnr = (float)(10.0 * log10(d * d * (double)n / sse));  // IEEE: x / 0 = +inf -> +inf; NaN stays NaN
  if (RANGE) {
    const double r = fmax((double)hi_a - (double)lo_a, (double)hi_b - (double)lo_b);
    consts[0] = (float)((0.01 * r) * (0.01 * r));
    consts[1] = (float)((0.03 * r) * (0.03 * r));
    consts[2] = (float)sse;
    consts[3] = 0.f;
  }
}

// pass 2.  grid (ceil((W - 10) / kT), ceil((H - 10) / kT), C); ppart [gridDim.z, gridDim.y, gridDim.x] float64
__global__ __launch_bounds__(kBlock) void ssim_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                      int C, Taps taps, const float* __restrict__ consts,
                                                      float* __restrict__ map, double* __restrict__ ppart) {
  __shared__ float sa[kHalo * kHalo], sb[kHalo * kHalo];
  __shared__ float hm[5][kHalo * kT];
  __shared__ double sh[4];
  const int c = blockIdx.z, x0 = blockIdx.x * kT, y0 = blockIdx.y * kT, tid = threadIdx.x;
  const int py = min(y0 + kHalo / 2, H - 1), px = min(x0 + kHalo / 2, W - 1);
  const int64_t pi = ((int64_t)py * W + px) * C + c;
  const float p = a[pi], q = b[pi];

  // the halo, shifted; outside the image: 0 (those taps reach only windows that are not written)
  for (int i = tid; i < kHalo * kHalo; i += kBlock) {
    const int r = i / kHalo, col = i - r * kHalo, y = y0 + r, x = x0 + col;
    float va = 0.f, vb = 0.f;
    if (y < H && x < W) {
      const int64_t idx = ((int64_t)y * W + x) * C + c;
      va = __fsub_rn(a[idx], p), vb = __fsub_rn(b[idx], q);
    }
    sa[i] = va, sb[i] = vb;
  }
  __syncthreads();

  // horizontal pass: row r, window column x <- taps x .. x + 10
  for (int i = tid; i < kHalo * kT; i += kBlock) {
    const int r = i / kT, x = i - r * kT;
    const float* ra = sa + r * kHalo + x;
    const float* rb = sb + r * kHalo + x;
    float va = ra[0], vb = rb[0];
    float ma = __fmul_rn(taps.g[0], va), mb = __fmul_rn(taps.g[0], vb);
    float maa = __fmul_rn(taps.g[0], __fmul_rn(va, va)), mbb = __fmul_rn(taps.g[0], __fmul_rn(vb, vb));
    float mab = __fmul_rn(taps.g[0], __fmul_rn(va, vb));
#pragma unroll
    for (int k = 1; k < kTaps; ++k) {
      va = ra[k], vb = rb[k];
      const float g = taps.g[k];
      ma = fmaf(g, va, ma), mb = fmaf(g, vb, mb);
      maa = fmaf(g, __fmul_rn(va, va), maa), mbb = fmaf(g, __fmul_rn(vb, vb), mbb), mab = fmaf(g, __fmul_rn(va, vb), mab);
    }
    hm[0][i] = ma, hm[1][i] = mb, hm[2][i] = maa, hm[3][i] = mbb, hm[4][i] = mab;
  }
  __syncthreads();

  // vertical pass: column x, windows yl .. yl + 3 from the rows yl .. yl + 13, each window its taps in the order 0 .. 10
  const int x = tid & (kT - 1), yl = (tid / kT) * kRowsPerLane;
  float m[5][kRowsPerLane];
#pragma unroll
  for (int f = 0; f < 5; ++f) {
#pragma unroll
    for (int rr = 0; rr < kRowsPerLane + kTaps - 1; ++rr) {
      const float v = hm[f][(yl + rr) * kT + x];
#pragma unroll
      for (int j = 0; j < kRowsPerLane; ++j) {
        const int k = rr - j;
        if (k == 0) m[f][j] = __fmul_rn(taps.g[0], v);
        else if (k > 0 && k < kTaps) m[f][j] = fmaf(taps.g[k], v, m[f][j]);
      }
    }
  }

  const float c1 = consts[0], c2 = consts[1];
  double part = 0.0;
#pragma unroll
  for (int j = 0; j < kRowsPerLane; ++j) {
    const float ma = m[0][j], mb = m[1][j];
    const float mua = __fadd_rn(p, ma), mub = __fadd_rn(q, mb);
    const float var_a = __fsub_rn(m[2][j], __fmul_rn(ma, ma)), var_b = __fsub_rn(m[3][j], __fmul_rn(mb, mb));
    const float cov = __fsub_rn(m[4][j], __fmul_rn(ma, mb));
    const float n1 = __fadd_rn(__fmul_rn(2.f, __fmul_rn(mua, mub)), c1), n2 = __fadd_rn(__fmul_rn(2.f, cov), c2);
    const float d1 = __fadd_rn(__fadd_rn(__fmul_rn(mua, mua), __fmul_rn(mub, mub)), c1);
    const float d2 = __fadd_rn(__fadd_rn(var_a, var_b), c2);
    const float s = __fdiv_rn(__fmul_rn(n1, n2), __fmul_rn(d1, d2));
    const int y = y0 + yl + j, xx = x0 + x;
    if (y < H - (kTaps - 1) && xx < W - (kTaps - 1)) {
      if (map) map[((int64_t)y * (W - (kTaps - 1)) + xx) * C + c] = s;
      part += (double)s;
    }
  }
  const double bs = block_sum_fixed(part, sh);
  if (tid == 0) ppart[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = bs;
}

__global__ __launch_bounds__(kBlock) void ssim_final_kernel(const double* __restrict__ ppart, int64_t np, int64_t count,
                                                            const float* __restrict__ consts, float* __restrict__ ssim) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < np; i += kBlock) s += ppart[i];
  const double total = block_sum_fixed(s, sh);
  if (threadIdx.x == 0) {
    const float sse = consts[2];
    *ssim = sse != sse ? sse : (float)(total / (double)count);
  }
}

struct Scratch {
  int64_t nb, tiles_x, tiles_y, np, off_psum, off_pmm, off_consts, off_ppart, bytes;
};
Scratch layout(int64_t h, int64_t w, int64_t c) {
  Scratch s;
  s.nb = (h * w * c + kStatItems - 1) / kStatItems;
  s.tiles_x = (w - (kTaps - 1) + kT - 1) / kT, s.tiles_y = (h - (kTaps - 1) + kT - 1) / kT;
  s.np = s.tiles_x * s.tiles_y * c;
  int64_t o = 0;
  s.off_psum = o, o += s.nb * 8;    // double [nb]
  s.off_ppart = o, o += s.np * 8;   // double [c, tiles_y, tiles_x]
  s.off_pmm = o, o += s.nb * 16;    // float  [nb, 4]
  s.off_consts = o, o += 16;        // float  [4]
  s.bytes = o;
  return s;
}

int validate_shape(const char* who, int32_t h, int32_t w, int32_t c) {
  NR_REQUIRE(h >= kTaps && w >= kTaps, NRHIP_ERR_INVALID_ARG, "%s: image %d x %d is smaller than the %d x %d window", who, h, w,
             kTaps, kTaps);
  NR_REQUIRE(c == 1 || c == 3, NRHIP_ERR_UNSUPPORTED, "%s: %d channels, not 1 or 3", who, c);
  NR_REQUIRE((int64_t)h * w * c < (INT64_C(1) << 31) && (h + kT - 1) / kT <= 65535, NRHIP_ERR_UNSUPPORTED,
             "%s: image %d x %d x %d has >= 2^31 elements or more than 65535 rows of tiles", who, h, w, c);
  return NRHIP_OK;
}

}  // namespace
}  // namespace nrhip

using namespace nrhip;

extern "C" int nrhip_image_metrics_workspace(int32_t h, int32_t w, int32_t c, int64_t* bytes) {
  NR_REQUIRE(bytes, NRHIP_ERR_INVALID_ARG, "image_metrics_workspace: bytes is NULL");
  if (int rc = validate_shape("image_metrics_workspace", h, w, c)) return rc;
  *bytes = layout(h, w, c).bytes;
  return NRHIP_OK;
}

extern "C" int nrhip_image_metrics(const float* a, const float* b, int32_t h, int32_t w, int32_t c, float psnr_range,
                                   float* ssim_map, void* workspace, int64_t workspace_bytes, float* out, void* stream) {
  if (int rc = validate_shape("image_metrics", h, w, c)) return rc;
  NR_REQUIRE(a && b, NRHIP_ERR_INVALID_ARG, "image_metrics: an image is NULL");
  NR_REQUIRE(out, NRHIP_ERR_INVALID_ARG, "image_metrics: out is NULL");
  NR_REQUIRE(psnr_range > 0.f, NRHIP_ERR_INVALID_ARG, "image_metrics: psnr_range %g is not positive", (double)psnr_range);
  const Scratch s = layout(h, w, c);
  NR_REQUIRE(workspace && workspace_bytes >= s.bytes, NRHIP_ERR_INVALID_ARG,
             "image_metrics: workspace is NULL or smaller than nrhip_image_metrics_workspace asks for (%lld < %lld)",
             (long long)workspace_bytes, (long long)s.bytes);
  NR_REQUIRE(((uintptr_t)workspace & 15) == 0, NRHIP_ERR_INVALID_ARG, "image_metrics: workspace is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* psum = (double*)(ws + s.off_psum);
  double* ppart = (double*)(ws + s.off_ppart);
  float* pmm = (float*)(ws + s.off_pmm);
  float* consts = (float*)(ws + s.off_consts);
  const int64_t n = (int64_t)h * w * c;
  stats_kernel<true><<<(unsigned)s.nb, kBlock, 0, st>>>(a, b, n, psum, pmm);
  stats_final_kernel<true><<<1, kBlock, 0, st>>>(psum, pmm, (int)s.nb, n, psnr_range, out, consts);
  const dim3 grid((unsigned)s.tiles_x, (unsigned)s.tiles_y, (unsigned)c);
  ssim_kernel<<<grid, kBlock, 0, st>>>(a, b, h, w, c, gaussian_taps(), consts, ssim_map, ppart);
  ssim_final_kernel<<<1, kBlock, 0, st>>>(ppart, s.np, (int64_t)(h - (kTaps - 1)) * (w - (kTaps - 1)) * c, consts, out + 1);
  return check_launch("image_metrics");
}

extern "C" int nrhip_image_psnr(const float* a, const float* b, int64_t n, float psnr_range, void* workspace, float* out,
                                void* stream) {
  NR_REQUIRE(n >= 1, NRHIP_ERR_INVALID_ARG, "image_psnr: n = %lld, not >= 1", (long long)n);
  NR_REQUIRE(n < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "image_psnr: n >= 2^31");
  NR_REQUIRE(a && b, NRHIP_ERR_INVALID_ARG, "image_psnr: an image is NULL");
  NR_REQUIRE(out, NRHIP_ERR_INVALID_ARG, "image_psnr: out is NULL");
  NR_REQUIRE(psnr_range > 0.f, NRHIP_ERR_INVALID_ARG, "image_psnr: psnr_range %g is not positive", (double)psnr_range);
  NR_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, NRHIP_ERR_INVALID_ARG,
             "image_psnr: workspace is NULL or not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = (n + kStatItems - 1) / kStatItems;
  stats_kernel<false><<<(unsigned)nb, kBlock, 0, st>>>(a, b, n, (double*)workspace, nullptr);
  stats_final_kernel<false><<<1, kBlock, 0, st>>>((const double*)workspace, nullptr, (int)nb, n, psnr_range, out, nullptr);
  return check_launch("image_psnr");
}
