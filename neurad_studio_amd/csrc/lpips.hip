// LPIPS (torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True), the third number of the
// reference's get_image_metrics_and_images, models/neurad.py:267,587): AlexNet features of cat([a, b]) tapped after each
// ReLU, unit-normalised per pixel, a weighted squared difference per tap, the pixel mean.  Forward only.
// fp16 operands with fp32 accumulation on every layer: the CPU emulation of exactly that (tests/lpips_refs.py,
// DESIGN.md §8) stays below 1e-4 absolute of float64 on every end-to-end case, against a budget of 5e-4.
//
//   stage_kernel        two fp32 [n, 3] images -> fp16 [2 n, 4]: (2 v - 1 - shift) / scale in float64, rounded to fp32 and
//                       then to fp16 (the path of torch's double -> half), channel 3 zero.  The same pass raises a device
//                       flag when a value is outside [0, 1] or not finite (torchmetrics' _valid_img); nobody reads it here.
//   conv_kernel<KS, S, P, MT, NT>   implicit GEMM on v_mfma_f32_32x32x16_f16 for input channel counts that are multiples of
//                       16: M = OUTPUT pixels of the whole batch (m = (b Ho + oy) Wo + ox: tiles cross rows and images,
//                       the border test is per pixel and per tap), N = output channels, K = KS KS Cin walked tap by tap.
//                       A fragments are 16-byte loads straight from the NHWC activation, B fragments 16-byte loads of the
//                       packed weights, as in vgg_loss.hip's conv3_kernel.  A tap outside the image contributes zeros that
//                       were never loaded from there: the lane reads pixel 0 of the tensor and drops it.
//   conv1_kernel<MT>    the 3 -> 64, 11 x 11, stride 4, pad 2 layer on the 4-channel staged image.  K is laid out as
//                       [ky < 11][kx < 12][c < 4] = 528 = 33 k-steps of 16: one k-step is four neighbouring taps of a row,
//                       a lane's 8 operands are TWO neighbouring pixels (two 8-byte loads; the row start is only 8-byte
//                       aligned when W is odd).  Real products are 363 of the 528; kx = 11 and c = 3 are padding, zero in
//                       the packed weights AND in the fragment (the lane never loads them), so no garbage meets a zero.
//   pool3s2_kernel      max_pool2d(3, 2), floor mode, no padding: every window lies inside the image.
//   head kernels        8 lanes per pixel pair, fp32: both squared norms, then sum_c lin_c (fa_c / na - fb_c / nb)^2, the
//                       lanes' sums joined by a fixed butterfly; float64 partial per workgroup (32 pixels), added in a fixed
//                       order by one workgroup per image pair, divided by the pixel count, one rounding to fp32.  No
//                       atomics: the same bits every run.
#include <cmath>

#include "common.h"

namespace nrhip {
namespace {

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using half4 = __attribute__((ext_vector_type(4))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

union Frag {
  uint4 u;
  uint2 d[2];
  half8 h;
};

constexpr int kBlock = 256;
constexpr int kImgC = NRHIP_LPIPS_IMAGE_CHANNELS;
constexpr int kKU = 2;       // k-steps requested before their MFMAs (vgg_loss.hip's measurement); 64, 192, 384, 256 are
                             // all multiples of 16 * kKU
constexpr int kRowSteps = 3; // conv1: k-steps per kernel row (12 taps x 4 channels / 16)
constexpr int kHeadLanes = 8;                      // head: lanes per pixel
constexpr int kHeadPixels = NRHIP_LPIPS_HEAD_PIXELS;  // head: pixels per workgroup
static_assert(kHeadPixels * kHeadLanes == kBlock, "head tiling");

struct Layer {
  int cin, cout, ks, stride, pad;
};
constexpr Layer kLayers[5] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};

inline int find_layer(int cin, int cout, int ks, int stride, int pad) {
  for (int l = 0; l < 5; ++l)
    if (kLayers[l].cin == cin && kLayers[l].cout == cout && kLayers[l].ks == ks && kLayers[l].stride == stride &&
        kLayers[l].pad == pad)
      return l;
  return -1;
}
inline int find_weight(int cin, int cout, int ks) {
  for (int l = 0; l < 5; ++l)
    if (kLayers[l].cin == cin && kLayers[l].cout == cout && kLayers[l].ks == ks) return l;
  return -1;
}
// k-steps of one layer's reduction: conv1 walks 11 rows of 3, the others KS KS taps of Cin / 16
inline int k_steps(const Layer& l) { return l.cin == 3 ? l.ks * kRowSteps : l.ks * l.ks * (l.cin / 16); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- weights -> fragment order ------------------------------------------------------------------------------------------
// wfrag[step][nb < cout / 32][lane] = 8 halves B[k = 16 step' + 8 (lane >> 5) + e][j = 32 nb + (lane & 31)], zero where k is
// padding.  General layers: step = tap * (cin / 16) + kc, the 8 halves are channels 16 kc + 8 (lane >> 5) + e of tap (ky, kx).
// conv1: step = ky * 3 + q, the 8 halves are (kx = 4 q + 2 (lane >> 5) + (e >> 2), c = e & 3).
__global__ void conv_pack_kernel(const float* __restrict__ w, int cout, int cin, int ks, int steps, int nb_n,
                                 uint4* __restrict__ wfrag) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)steps * nb_n * 64) return;
  const int lane = (int)(t & 63);
  const int64_t q = t >> 6;
  const int nb = (int)(q % nb_n), step = (int)(q / nb_n);
  const int j = nb * 32 + (lane & 31), kb = lane >> 5;
  Frag f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int c, ky, kx;
    if (cin == 3) {
      ky = step / kRowSteps;
      kx = 4 * (step - ky * kRowSteps) + 2 * kb + (e >> 2);
      c = e & 3;
    } else {
      const int kc_n = cin / 16, tap = step / kc_n;
      ky = tap / ks, kx = tap - ky * ks;
      c = (step - tap * kc_n) * 16 + 8 * kb + e;
    }
    float v = 0.f;
    if (c < cin && kx < ks && j < cout) v = w[(((int64_t)j * cin + c) * ks + ky) * ks + kx];
    f.h[e] = (_Float16)v;
  }
  wfrag[t] = f.u;
}

// ---- convolution: shared pieces ---------------------------------------------------------------------------------------------
template <int MT>
struct Pixels {
  int oy[MT], ox[MT];
  int64_t img[MT];  // first input pixel of the output pixel's own image
  bool valid[MT];
};

template <int MT>
__device__ __forceinline__ void locate(int64_t m0, int i, int64_t M, int H, int W, int Ho, int Wo, Pixels<MT>& p) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int64_t m = m0 + mt * 32 + i;
    p.valid[mt] = m < M;
    const int64_t mm = p.valid[mt] ? m : 0;
    const int64_t b = mm / ((int64_t)Ho * Wo);
    const int rem = (int)(mm - b * Ho * Wo);
    p.oy[mt] = rem / Wo;
    p.ox[mt] = rem - p.oy[mt] * Wo;
    p.img[mt] = b * H * W;
  }
}

template <int MT, int NT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[MT][NT]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
}

// v = acc + bias, ReLU, one rounding to fp16
template <int MT, int NT>
__device__ __forceinline__ void epilogue(const f32x16 (&acc)[MT][NT], const float* __restrict__ bias, _Float16* __restrict__ out,
                                         int64_t m0, int64_t M, int tn, int lane, int cout, int relu) {
  const int i = lane & 31, kb = lane >> 5;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int c = (tn * NT + nt) * 32 + i;
    if (c >= cout) continue;
    const float bj = bias ? bias[c] : 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = m0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kb;
        if (m >= M) continue;
        float v = acc[mt][nt][r] + bj;
        if (relu) v = v < 0.f ? 0.f : v;  // (a NaN stays a NaN)
        out[m * cout + c] = (_Float16)v;
      }
  }
}

// ---- convolution, Cin a multiple of 16 ----------------------------------------------------------------------------------------
template <int KS, int STRIDE, int PAD, int MT, int NT>
__global__ __launch_bounds__(kBlock) void conv_kernel(const _Float16* __restrict__ in, const uint4* __restrict__ wfrag,
                                                      const float* __restrict__ bias, _Float16* __restrict__ out, int H, int W,
                                                      int Ho, int Wo, int cin, int cout, int nb_n, int relu, int64_t M) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_n = nb_n / NT;
  const int64_t t = (int64_t)blockIdx.x * 4 + wave;
  const int tn = (int)(t % tiles_n);
  const int64_t m0 = (t / tiles_n) * (32 * MT);
  if (m0 >= M) return;  // (whole waves; the kernel has no barrier)
  const int i = lane & 31, kb = lane >> 5;
  const int kc_n = cin >> 4;
  Pixels<MT> p;
  locate<MT>(m0, i, M, H, W, Ho, Wo, p);
  f32x16 acc[MT][NT];
  zero_acc<MT, NT>(acc);

  for (int tap = 0; tap < KS * KS; ++tap) {
    const int ky = tap / KS, kx = tap - KS * ky;
    bool ok[MT];
    const _Float16* ap[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int yy = p.oy[mt] * STRIDE - PAD + ky, xx = p.ox[mt] * STRIDE - PAD + kx;
      ok[mt] = p.valid[mt] && yy >= 0 && yy < H && xx >= 0 && xx < W;  // inside the pixel's OWN image
      const int64_t src = ok[mt] ? p.img[mt] + (int64_t)yy * W + xx : 0;
      ap[mt] = in + src * cin + kb * 8;
    }
    const uint4* wp = wfrag + ((int64_t)tap * kc_n * nb_n + tn * NT) * 64 + lane;
    for (int kc0 = 0; kc0 < kc_n; kc0 += kKU) {  // kc_n is a multiple of kKU (checked on the host)
      Frag a[kKU][MT], bf[kKU][NT];
#pragma unroll
      for (int u = 0; u < kKU; ++u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {  // (a border lane reads pixel 0 and drops it: no branch)
          const uint4 v = *(const uint4*)(ap[mt] + (kc0 + u) * 16);
          a[u][mt].u = ok[mt] ? v : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bf[u][nt].u = wp[((int64_t)(kc0 + u) * nb_n + nt) * 64];
      }
#pragma unroll
      for (int u = 0; u < kKU; ++u)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[u][mt].h, bf[u][nt].h, acc[mt][nt], 0, 0, 0);
    }
  }
  epilogue<MT, NT>(acc, bias, out, m0, M, tn, lane, cout, relu);
}

// ---- convolution of the staged image: 3 (stored 4) -> 64, 11 x 11, stride 4, pad 2 ----------------------------------------------
template <int MT>
__global__ __launch_bounds__(kBlock) void conv1_kernel(const _Float16* __restrict__ in, const uint4* __restrict__ wfrag,
                                                       const float* __restrict__ bias, _Float16* __restrict__ out, int H, int W,
                                                       int Ho, int Wo, int relu, int64_t M) {
  constexpr int KS = 11, STRIDE = 4, PAD = 2, NT = 2, NB = 2, COUT = 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * 4 + wave;
  const int64_t m0 = t * (32 * MT);
  if (m0 >= M) return;
  const int i = lane & 31, kb = lane >> 5;
  Pixels<MT> p;
  locate<MT>(m0, i, M, H, W, Ho, Wo, p);
  f32x16 acc[MT][NT];
  zero_acc<MT, NT>(acc);

  for (int ky = 0; ky < KS; ++ky) {
    Frag a[kRowSteps][MT], bf[kRowSteps][NT];
#pragma unroll
    for (int q = 0; q < kRowSteps; ++q) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int yy = p.oy[mt] * STRIDE - PAD + ky;
        const bool row_ok = p.valid[mt] && yy >= 0 && yy < H;
#pragma unroll
        for (int s = 0; s < 2; ++s) {  // the lane's two taps of this k-step
          const int kx = 4 * q + 2 * kb + s;
          const int xx = p.ox[mt] * STRIDE - PAD + kx;
          const bool ok = row_ok && kx < KS && xx >= 0 && xx < W;
          const int64_t src = ok ? p.img[mt] + (int64_t)yy * W + xx : 0;
          const uint2 v = *(const uint2*)(in + src * kImgC);
          a[q][mt].d[s] = ok ? v : uint2{0u, 0u};
        }
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bf[q][nt].u = wfrag[((int64_t)(ky * kRowSteps + q) * NB + nt) * 64 + lane];
    }
#pragma unroll
    for (int q = 0; q < kRowSteps; ++q)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[q][mt].h, bf[q][nt].h, acc[mt][nt], 0, 0, 0);
  }
  epilogue<MT, NT>(acc, bias, out, m0, M, 0, lane, COUT, relu);
}

struct Plan {
  int mt, nt, nb_n;
  int64_t waves;
};

// nt: two 32-channel blocks per wave (64, 192, 384 and 256 are all multiples of 64); mt: 64 pixels per wave once that still
// leaves 2048 waves (two per SIMD of 256 CUs), else 32 -- vgg_loss.hip's rule.
int resolve_plan(const char* who, int64_t m, int layer, int plan, Plan& p) {
  NR_REQUIRE(m >= 0 && m < (INT64_C(1) << 31), m < 0 ? NRHIP_ERR_INVALID_ARG : NRHIP_ERR_UNSUPPORTED,
             "%s: %lld output pixels outside [0, 2^31)", who, (long long)m);
  NR_REQUIRE(plan >= 0 && plan <= 2, NRHIP_ERR_INVALID_ARG, "%s: plan %d not in {0: auto, 1, 2: 32-pixel blocks per wave}", who,
             plan);
  p.nb_n = kLayers[layer].cout / 32;
  p.nt = 2;
  p.mt = plan ? plan : (((m + 63) / 64) * (p.nb_n / p.nt) >= 2048 ? 2 : 1);
  p.waves = ((m + 32 * p.mt - 1) / (32 * p.mt)) * (p.nb_n / p.nt);
  return NRHIP_OK;
}

int require_layer(const char* who, int cin, int cout, int ks, int stride, int pad, int& layer) {
  layer = find_layer(cin, cout, ks, stride, pad);
  NR_REQUIRE(layer >= 0, NRHIP_ERR_UNSUPPORTED,
             "%s: convolution %d -> %d, kernel %d, stride %d, pad %d unsupported (AlexNet's five: 3->64 k11 s4 p2, 64->192 k5 s1 "
             "p2, 192->384 / 384->256 / 256->256 k3 s1 p1)",
             who, cin, cout, ks, stride, pad);
  return NRHIP_OK;
}

// ---- maxpool 3 x 3, stride 2 ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pool3s2_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out, int64_t B,
                                                         int H, int W, int C) {
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1, G = C >> 3;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= B * Ho * Wo * G) return;
  const int cg = (int)(t % G);
  const int64_t pix = t / G;
  const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho);
  const int64_t b = pix / ((int64_t)Wo * Ho);
  Frag o;
#pragma unroll
  for (int k = 0; k < 9; ++k) {  // rows 2 yo .. 2 yo + 2 <= H - 1, columns alike: inside the image
    Frag v;
    v.u = *(const uint4*)(in + ((b * H + 2 * yo + k / 3) * W + 2 * xo + k % 3) * C + cg * 8);
    if (k == 0) {
      o.u = v.u;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = (float)v.h[e], best = (float)o.h[e];
        if (x > best || x != x) o.h[e] = v.h[e];  // NaN taken like torch
      }
    }
  }
  *(uint4*)(out + pix * C + cg * 8) = o.u;
}

// ---- staging ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void stage_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n_pixels,
                                                       const float* __restrict__ shift, const float* __restrict__ scale,
                                                       _Float16* __restrict__ out, int32_t* __restrict__ flag) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= 2 * n_pixels) return;
  const float* src = t < n_pixels ? a + 3 * t : b + 3 * (t - n_pixels);
  half4 h;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = src[c];
    bad = bad || !(v >= 0.f && v <= 1.f);  // (a NaN fails both comparisons)
    const double x = ((2.0 * (double)v - 1.0) - (double)shift[c]) / (double)scale[c];
    h[c] = (_Float16)(float)x;
  }
  h[3] = (_Float16)0.f;
  *(half4*)(out + t * kImgC) = h;
  if (bad) atomicOr(flag, 1);
}

// ---- head -------------------------------------------------------------------------------------------------------------------------
// (a, b, c, d) over the four waves as ((a + b) + c) + d, lanes by a fixed shuffle tree: one order, every run
__device__ __forceinline__ double block_sum_fixed(double s, double* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = s;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// feat [2 B][P][C] fp16; block (x, y) takes pixels [32 x, 32 x + 32) of pair y, 8 neighbouring lanes per pixel: lane j of a
// pixel takes the 8-channel groups j, j + 8, ... so the 8 lanes read 128 consecutive bytes; their sums meet in an xor
// butterfly (commutative at every level: all 8 lanes hold the same bits).  partial[y * gridDim.x + x]
template <class T>
__device__ __forceinline__ T sum8(T v) {
#pragma unroll
  for (int off = 1; off < kHeadLanes; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kBlock) void head_partial_kernel(const _Float16* __restrict__ feat, const float* __restrict__ lin,
                                                              int64_t B, int64_t P, int C, float eps, int eps_mode,
                                                              double* __restrict__ partial) {
  __shared__ double sh[4];
  const int sub = threadIdx.x & (kHeadLanes - 1);
  const int64_t pix = (int64_t)blockIdx.x * kHeadPixels + (threadIdx.x >> 3);
  const int64_t pc = pix < P ? pix : P - 1;  // (a lane past the end works on the last pixel and drops it: no divergent shuffle)
  const int64_t pair = blockIdx.y;
  const _Float16* fa = feat + (pair * P + pc) * C;
  const _Float16* fb = feat + ((pair + B) * P + pc) * C;
  float sa = 0.f, sb = 0.f;
  for (int c0 = sub * 8; c0 < C; c0 += 8 * kHeadLanes) {
    Frag x, y;
    x.u = *(const uint4*)(fa + c0), y.u = *(const uint4*)(fb + c0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float u = (float)x.h[e], v = (float)y.h[e];
      sa += u * u, sb += v * v;
    }
  }
  sa = sum8(sa), sb = sum8(sb);
  // division, not a multiplication by the reciprocal: n(f)_c = f_c / norm is what the formula states (one rounding)
  const float na = eps_mode == NRHIP_LPIPS_EPS_INSIDE ? sqrtf(eps + sa) : sqrtf(sa) + eps;
  const float nb = eps_mode == NRHIP_LPIPS_EPS_INSIDE ? sqrtf(eps + sb) : sqrtf(sb) + eps;
  float acc = 0.f;
  for (int c0 = sub * 8; c0 < C; c0 += 8 * kHeadLanes) {  // (the second read of the pixel's 2 C halves comes from the L1 / L2)
    Frag x, y;
    x.u = *(const uint4*)(fa + c0), y.u = *(const uint4*)(fb + c0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float delta = (float)x.h[e] / na - (float)y.h[e] / nb;
      acc += lin[c0 + e] * (delta * delta);
    }
  }
  acc = sum8(acc);
  const double bs = block_sum_fixed(sub == 0 && pix < P ? (double)acc : 0.0, sh);
  if (threadIdx.x == 0) partial[pair * gridDim.x + blockIdx.x] = bs;
}

__global__ __launch_bounds__(kBlock) void head_final_kernel(const double* __restrict__ partial, int64_t nparts, int64_t P,
                                                            int accumulate, float* __restrict__ out) {
  __shared__ double sh[4];
  const int64_t pair = blockIdx.x;
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < nparts; k += kBlock) s += partial[pair * nparts + k];
  const double total = block_sum_fixed(s, sh);
  if (threadIdx.x == 0) out[pair] = (float)((accumulate ? (double)out[pair] : 0.0) + total / (double)P);
}

}  // namespace
}  // namespace nrhip

using namespace nrhip;

extern "C" int nrhip_lpips_stage_images(const float* a, const float* b, int64_t n_pixels, const float* shift, const float* scale,
                                        void* out, int32_t* flag, void* stream) {
  NR_REQUIRE(n_pixels >= 0 && n_pixels < (INT64_C(1) << 30), NRHIP_ERR_INVALID_ARG, "lpips_stage_images: bad pixel count");
  if (n_pixels == 0) return NRHIP_OK;
  NR_REQUIRE(a && b && shift && scale && out && flag, NRHIP_ERR_INVALID_ARG, "lpips_stage_images: NULL pointer");
  NR_REQUIRE(((uintptr_t)out & 7) == 0, NRHIP_ERR_INVALID_ARG, "lpips_stage_images: out is not 8-byte aligned");
  stage_kernel<<<grid_for(2 * n_pixels, kBlock), kBlock, 0, (hipStream_t)stream>>>(a, b, n_pixels, shift, scale, (_Float16*)out,
                                                                                   flag);
  return check_launch("lpips_stage_images");
}

extern "C" int nrhip_conv2d_plan(int64_t n_pixels, int32_t cin, int32_t cout, int32_t ksize, int32_t stride, int32_t pad,
                                 int32_t plan, int32_t* pixel_blocks, int32_t* channel_blocks, int64_t* waves) {
  NR_REQUIRE(pixel_blocks && channel_blocks && waves, NRHIP_ERR_INVALID_ARG, "conv2d_plan: NULL out-pointer");
  int layer;
  if (int rc = require_layer("conv2d_plan", cin, cout, ksize, stride, pad, layer)) return rc;
  Plan p;
  if (int rc = resolve_plan("conv2d_plan", n_pixels, layer, plan, p)) return rc;
  *pixel_blocks = p.mt, *channel_blocks = p.nt, *waves = p.waves;
  return NRHIP_OK;
}

extern "C" int nrhip_conv2d_pack_bytes(int32_t cout, int32_t cin, int32_t ksize, int64_t* bytes) {
  NR_REQUIRE(bytes, NRHIP_ERR_INVALID_ARG, "conv2d_pack_bytes: bytes is NULL");
  const int layer = find_weight(cin, cout, ksize);
  NR_REQUIRE(layer >= 0, NRHIP_ERR_UNSUPPORTED,
             "conv2d_pack_bytes: weight [%d, %d, %d, %d] unsupported (AlexNet's five: [64,3,11,11], [192,64,5,5], [384,192,3,3], "
             "[256,384,3,3], [256,256,3,3])",
             cout, cin, ksize, ksize);
  *bytes = (int64_t)k_steps(kLayers[layer]) * (cout / 32) * 64 * 16;
  return NRHIP_OK;
}

extern "C" int nrhip_conv2d_pack(const float* weight, int32_t cout, int32_t cin, int32_t ksize, void* wfrag, void* stream) {
  int64_t bytes = 0;
  if (int rc = nrhip_conv2d_pack_bytes(cout, cin, ksize, &bytes)) return rc;
  NR_REQUIRE(weight && wfrag, NRHIP_ERR_INVALID_ARG, "conv2d_pack: NULL pointer");
  NR_REQUIRE(aligned16(wfrag), NRHIP_ERR_INVALID_ARG, "conv2d_pack: wfrag is not 16-byte aligned");
  const Layer& l = kLayers[find_weight(cin, cout, ksize)];
  conv_pack_kernel<<<grid_for(bytes / 16, kBlock), kBlock, 0, (hipStream_t)stream>>>(weight, cout, cin, ksize, k_steps(l),
                                                                                      cout / 32, (uint4*)wfrag);
  return check_launch("conv2d_pack");
}

extern "C" int nrhip_conv2d(const void* in, const void* wfrag, const float* bias, void* out, int32_t b, int32_t h, int32_t w,
                            int32_t cin, int32_t cout, int32_t ksize, int32_t stride, int32_t pad, int32_t relu, int32_t plan,
                            void* stream) {
  int layer;
  if (int rc = require_layer("conv2d", cin, cout, ksize, stride, pad, layer)) return rc;
  NR_REQUIRE(b >= 0 && h >= 1 && w >= 1, NRHIP_ERR_INVALID_ARG, "conv2d: bad shape %d x %d x %d", b, h, w);
  NR_REQUIRE(h + 2 * pad >= ksize && w + 2 * pad >= ksize, NRHIP_ERR_INVALID_ARG,
             "conv2d: a %d x %d input has no %d x %d window at pad %d", h, w, ksize, ksize, pad);
  NR_REQUIRE(layer != 0 || (h >= NRHIP_LPIPS_MIN_SIZE && w >= NRHIP_LPIPS_MIN_SIZE), NRHIP_ERR_INVALID_ARG,
             "conv2d: a %d x %d image is smaller than %d x %d (AlexNet's second pool would be empty)", h, w, NRHIP_LPIPS_MIN_SIZE,
             NRHIP_LPIPS_MIN_SIZE);
  NR_REQUIRE((int64_t)b * h * w < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "conv2d: >= 2^31 input pixels");
  const int ho = (h + 2 * pad - ksize) / stride + 1, wo = (w + 2 * pad - ksize) / stride + 1;
  const int64_t m = (int64_t)b * ho * wo;
  Plan p;
  if (int rc = resolve_plan("conv2d", m, layer, plan, p)) return rc;
  if (m == 0) return NRHIP_OK;
  NR_REQUIRE(in && wfrag && out, NRHIP_ERR_INVALID_ARG, "conv2d: NULL pointer");
  NR_REQUIRE(aligned16(wfrag) && (cin == 3 ? ((uintptr_t)in & 7) == 0 : aligned16(in)), NRHIP_ERR_INVALID_ARG,
             "conv2d: in / wfrag misaligned");
  const unsigned blocks = (unsigned)((p.waves + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  const _Float16* x = (const _Float16*)in;
  const uint4* wf = (const uint4*)wfrag;
  _Float16* y = (_Float16*)out;
  const int r = relu ? 1 : 0;
  static_assert((64 / 16) % kKU == 0 && (192 / 16) % kKU == 0 && (384 / 16) % kKU == 0 && (256 / 16) % kKU == 0, "kKU");
#define NR_CONV(KS, S, P, MT) conv_kernel<KS, S, P, MT, 2><<<blocks, kBlock, 0, st>>>(x, wf, bias, y, h, w, ho, wo, cin, cout, p.nb_n, r, m)
  if (layer == 0) {
    if (p.mt == 2) conv1_kernel<2><<<blocks, kBlock, 0, st>>>(x, wf, bias, y, h, w, ho, wo, r, m);
    else conv1_kernel<1><<<blocks, kBlock, 0, st>>>(x, wf, bias, y, h, w, ho, wo, r, m);
  } else if (layer == 1) {
    if (p.mt == 2) NR_CONV(5, 1, 2, 2);
    else NR_CONV(5, 1, 2, 1);
  } else {
    if (p.mt == 2) NR_CONV(3, 1, 1, 2);
    else NR_CONV(3, 1, 1, 1);
  }
#undef NR_CONV
  return check_launch("conv2d");
}

extern "C" int nrhip_maxpool3s2_fwd(const void* in, void* out, int64_t b, int32_t h, int32_t w, int32_t c, void* stream) {
  NR_REQUIRE(b >= 0 && h >= 3 && w >= 3 && c >= 8 && c % 8 == 0, NRHIP_ERR_INVALID_ARG,
             "maxpool3s2_fwd: bad shape %lld x %d x %d x %d (at least 3 x 3, channels a multiple of 8)", (long long)b, h, w, c);
  NR_REQUIRE(b * h * w < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "maxpool3s2_fwd: >= 2^31 pixels");
  if (b == 0) return NRHIP_OK;
  NR_REQUIRE(in && out, NRHIP_ERR_INVALID_ARG, "maxpool3s2_fwd: NULL pointer");
  NR_REQUIRE(aligned16(in) && aligned16(out), NRHIP_ERR_INVALID_ARG, "maxpool3s2_fwd: tensor not 16-byte aligned");
  const int64_t threads = b * ((h - 3) / 2 + 1) * ((w - 3) / 2 + 1) * (c / 8);
  pool3s2_kernel<<<grid_for(threads, kBlock), kBlock, 0, (hipStream_t)stream>>>((const _Float16*)in, (_Float16*)out, b, h, w, c);
  return check_launch("maxpool3s2_fwd");
}

extern "C" int nrhip_lpips_head_workspace(int64_t b, int64_t n_pixels, int64_t* bytes) {
  NR_REQUIRE(bytes, NRHIP_ERR_INVALID_ARG, "lpips_head_workspace: bytes is NULL");
  NR_REQUIRE(b >= 0 && n_pixels >= 0, NRHIP_ERR_INVALID_ARG, "lpips_head_workspace: negative count");
  *bytes = b * ((n_pixels + kHeadPixels - 1) / kHeadPixels) * 8;
  return NRHIP_OK;
}

extern "C" int nrhip_lpips_head(const void* feat, const float* lin, int64_t b, int64_t n_pixels, int32_t c, float eps,
                                int32_t eps_mode, int32_t accumulate, void* workspace, int64_t workspace_bytes, float* out,
                                void* stream) {
  NR_REQUIRE(b >= 1 && b < 65536 && n_pixels >= 1 && n_pixels < (INT64_C(1) << 31), NRHIP_ERR_INVALID_ARG,
             "lpips_head: %lld pairs of %lld pixels outside [1, 65536) x [1, 2^31)", (long long)b, (long long)n_pixels);
  NR_REQUIRE(c >= 8 && c % 8 == 0, NRHIP_ERR_INVALID_ARG, "lpips_head: %d channels (a multiple of 8)", c);
  NR_REQUIRE(eps_mode == NRHIP_LPIPS_EPS_INSIDE || eps_mode == NRHIP_LPIPS_EPS_OUTSIDE, NRHIP_ERR_INVALID_ARG,
             "lpips_head: eps_mode %d not in {0: inside the root, 1: added to the root}", eps_mode);
  NR_REQUIRE(eps >= 0.f, NRHIP_ERR_INVALID_ARG, "lpips_head: eps is negative or NaN");
  NR_REQUIRE(feat && lin && out, NRHIP_ERR_INVALID_ARG, "lpips_head: NULL pointer");
  NR_REQUIRE(aligned16(feat), NRHIP_ERR_INVALID_ARG, "lpips_head: feat is not 16-byte aligned");
  const int64_t nparts = (n_pixels + kHeadPixels - 1) / kHeadPixels;
  NR_REQUIRE(workspace && workspace_bytes >= b * nparts * 8 && ((uintptr_t)workspace & 7) == 0, NRHIP_ERR_INVALID_ARG,
             "lpips_head: workspace is NULL, misaligned or smaller than nrhip_lpips_head_workspace asks for");
  hipStream_t st = (hipStream_t)stream;
  head_partial_kernel<<<dim3((unsigned)nparts, (unsigned)b), kBlock, 0, st>>>((const _Float16*)feat, lin, b, n_pixels, c, eps,
                                                                               eps_mode, (double*)workspace);
  head_final_kernel<<<(unsigned)b, kBlock, 0, st>>>((const double*)workspace, nparts, n_pixels, accumulate ? 1 : 0, out);
  return check_launch("lpips_head");
}
