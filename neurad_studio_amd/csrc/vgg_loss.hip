// VGG-19 perceptual loss (model_components/losses.py:582-625, switched on by LossSettings.vgg_mult, models/neurad.py:69):
// the network up to relu5_1 on cat([rgb, image]), five L1 terms on the relu{1..5}_1 features, a gradient into the rendered
// half only.  fp16 operands with fp32 accumulation, the arithmetic of the reference's mixed-precision trainer.
//
//   conv3_kernel<MT, NT>  3x3 convolution (stride 1, pad 1) as an implicit GEMM on v_mfma_f32_32x32x16_f16: M = pixels of the
//                         WHOLE batch (m = (b H + y) W + x, so the 6 x 6 images of conv5_1 still fill 32-row tiles; the halo
//                         test is per pixel and never crosses into a neighbouring image), N = output channels, K = 9 Cin.
//                         A wave owns 32 MT pixels x 32 NT channels.  A fragments are 16-byte loads straight from the NHWC
//                         activation (lane = pixel, 8 consecutive channels), B fragments 16-byte loads of the pre-packed
//                         weights (fragment order, L2 resident); the four waves of a workgroup take neighbouring N tiles of
//                         the same pixels, so their A loads meet in the L1.  No LDS staging yet: the kernel is bound by the
//                         vector L1 and its latency, not by the matrix cores (DESIGN.md §8 has the measurement).
//                         Epilogue: v = acc * p (+ bias) (ReLU) (* [mask > 0]), one rounding to fp16.
//   pack                  mode 0: B[k][j] = w[j][k][ky][kx]; mode 1 (input gradient): B[k][j] = w[k][j][2 - ky][2 - kx].
//                         The 3-channel side is stored as NRHIP_VGG_IMAGE_CHANNELS = 16 channels, zero-padded.
//   working scale         every fp16 gradient tensor has a device state {amax, S}: stored = S * true, S a power of two, amax
//                         the largest stored magnitude (unsigned atomic max on the float's bits: non-negative floats order
//                         as their bits do, and a NaN sorts above +inf, so a non-finite value poisons the state).  A consumer
//                         multiplies by p = the power of two that brings amax into [0.5, 1) in its own epilogue (exact) and
//                         writes S_out = S_in * p.  No host read anywhere.
//   maxpool 2x2           floor mode; the backward recomputes the first maximum in row-major order (torch's choice) from the
//                         saved input; a dropped odd row / column gets exactly zero.
//   L1                    forward: float64 per-workgroup partials, added in a fixed order by one workgroup, one rounding to
//                         fp32.  Backward: c = w g / numel in float64, normalised to [0.5, 1) and rounded once to fp16;
//                         optionally added to the gradient that arrives from the layer above, both at a common power of two.
#include <cmath>

#include "common.h"

namespace nrhip {
namespace {

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

union Frag {
  uint4 u;
  half8 h;
};

constexpr int kKU = 2;  // k-steps (16 channels each) whose loads a wave requests before their MFMAs; every channel count but the
                        // image's 16 is a multiple of 16 * kKU.  Measured at the flagship batch, whole call: 1: 4.01 ms, 2: 3.68 ms,
                        // 4: 3.82 ms, 8: 3.77 ms
constexpr int kBlock = 256;
constexpr int kImgC = NRHIP_VGG_IMAGE_CHANNELS;
constexpr int kL1Items = NRHIP_L1_ITEMS;  // elements per workgroup of the L1 kernels: 8 per thread

inline bool vgg_channels(int c) { return c == 3 || c == 64 || c == 128 || c == 256 || c == 512; }
inline int stored_channels(int c) { return c == 3 ? kImgC : c; }

// the power of two p with amax * p in [0.5, 1); 1 for amax == 0; NaN for a non-finite amax (poison)
__device__ __forceinline__ float pow2_norm(float amax) {
  if (!(amax < __uint_as_float(0x7f800000u))) return __uint_as_float(0x7fc00000u);
  if (amax == 0.f) return 1.f;
  int e;
  (void)frexpf(amax, &e);
  return ldexpf(1.f, -e);
}

__device__ __forceinline__ uint32_t abs_bits(_Float16 h) { return __float_as_uint((float)h) & 0x7fffffffu; }

__device__ __forceinline__ uint32_t wave_max_bits(uint32_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// ---- weights -> fragment order ------------------------------------------------------------------------------------------
// wfrag[tap = ky * 3 + kx][kc < K / 16][nb < NP / 32][lane] = 8 halves B[k = 16 kc + 8 (lane >> 5) + e][j = 32 nb + (lane & 31)];
// K = stored channels of the GEMM's input side, NP = the output side rounded up to 32; zero outside the real channels.
__global__ void conv3_pack_kernel(const float* __restrict__ w, int co, int ci, int mode, int kc_n, int nb_n,
                                  uint4* __restrict__ wfrag) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)9 * kc_n * nb_n * 64) return;
  const int lane = (int)(t & 63);
  const int64_t q = t >> 6;
  const int nb = (int)(q % nb_n), kc = (int)((q / nb_n) % kc_n), tap = (int)(q / ((int64_t)nb_n * kc_n));
  const int ky = tap / 3, kx = tap - 3 * ky;
  const int kreal = mode == 0 ? ci : co, nreal = mode == 0 ? co : ci;
  const int j = nb * 32 + (lane & 31), k0 = kc * 16 + 8 * (lane >> 5);
  Frag f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    float v = 0.f;
    if (k < kreal && j < nreal)
      v = mode == 0 ? w[(((int64_t)j * ci + k) * 3 + ky) * 3 + kx] : w[(((int64_t)k * ci + j) * 3 + (2 - ky)) * 3 + (2 - kx)];
    f.h[e] = (_Float16)v;
  }
  wfrag[t] = f.u;
}

// ---- convolution --------------------------------------------------------------------------------------------------------
template <int MT, int NT, int KU>
__global__ __launch_bounds__(kBlock) void conv3_kernel(const _Float16* __restrict__ in, const uint4* __restrict__ wfrag,
                                                       const float* __restrict__ bias, const _Float16* __restrict__ mask,
                                                       const float* __restrict__ in_state, float* __restrict__ out_state,
                                                       _Float16* __restrict__ out, int H, int W, int cin_s, int cout_s,
                                                       int nb_n, int relu, int64_t M) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_n = nb_n / NT;
  const int64_t t = (int64_t)blockIdx.x * 4 + wave;
  const int tn = (int)(t % tiles_n);
  const int64_t m0 = (t / tiles_n) * (32 * MT);
  if (m0 >= M) return;  // (whole waves; the kernel has no barrier)
  const int i = lane & 31, kb = lane >> 5;
  const int kc_n = cin_s >> 4;
  int py[MT], px[MT];
  int64_t pm[MT];
  bool pv[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int64_t m = m0 + mt * 32 + i;
    pv[mt] = m < M;
    pm[mt] = pv[mt] ? m : 0;
    const int rem = (int)(pm[mt] % ((int64_t)H * W));
    py[mt] = rem / W;
    px[mt] = rem - py[mt] * W;
  }
  f32x16 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
    bool ok[MT];
    const _Float16* ap[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int yy = py[mt] + dy, xx = px[mt] + dx;
      ok[mt] = pv[mt] && yy >= 0 && yy < H && xx >= 0 && xx < W;  // inside the pixel's OWN image
      const int64_t src = ok[mt] ? pm[mt] + (int64_t)dy * W + dx : 0;
      ap[mt] = in + src * cin_s + kb * 8;
    }
    const uint4* wp = wfrag + ((int64_t)tap * kc_n * nb_n + tn * NT) * 64 + lane;
    // KU k-steps per trip, all of their loads requested before the first MFMA (a loop with a run-time trip count around an
    // MFMA is never unrolled by the compiler: the trip count is made a multiple of KU on the host instead)
    for (int kc0 = 0; kc0 < kc_n; kc0 += KU) {
      Frag a[KU][MT], bf[KU][NT];
#pragma unroll
      for (int u = 0; u < KU; ++u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {  // (a halo lane reads pixel 0 and drops it: no branch)
          const uint4 v = *(const uint4*)(ap[mt] + (kc0 + u) * 16);
          a[u][mt].u = ok[mt] ? v : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bf[u][nt].u = wp[((int64_t)(kc0 + u) * nb_n + nt) * 64];
      }
#pragma unroll
      for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[u][mt].h, bf[u][nt].h, acc[mt][nt], 0, 0, 0);
    }
  }

  float p = 1.f, s_in = 1.f;
  if (in_state) {
    p = pow2_norm(in_state[0]);
    s_in = in_state[1];
  }
  uint32_t lmax = 0u;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int c = (tn * NT + nt) * 32 + i;
    if (c >= cout_s) continue;
    const float bj = bias ? bias[c] : 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = m0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kb;
        if (m >= M) continue;
        float v = acc[mt][nt][r] * p + bj;
        if (relu) v = v < 0.f ? 0.f : v;  // (a NaN stays a NaN)
        const int64_t o = m * cout_s + c;
        if (mask && !((float)mask[o] > 0.f)) v = 0.f;
        const _Float16 h = (_Float16)v;
        out[o] = h;
        const uint32_t b = abs_bits(h);
        lmax = b > lmax ? b : lmax;
      }
  }
  if (out_state) {
    lmax = wave_max_bits(lmax);
    if (lane == 0 && lmax) atomicMax(reinterpret_cast<uint32_t*>(out_state), lmax);
    if (t == 0 && lane == 0) out_state[1] = s_in * p;
  }
}

struct Plan {
  int mt, nt, nb_n;
  int64_t waves;
};

// nt: two 32-channel blocks per wave wherever there are two (everything but the gradient that reaches the image);
// mt: 64 pixels per wave once that still leaves 2048 waves (two per SIMD of 256 CUs), else 32 -- the deep layers are small.
Plan auto_plan(int64_t m, int cout) {
  Plan p;
  p.nb_n = (stored_channels(cout) + 31) / 32;
  p.nt = p.nb_n >= 2 ? 2 : 1;
  p.mt = ((m + 63) / 64) * (p.nb_n / p.nt) >= 2048 ? 2 : 1;
  return p;
}

int resolve_plan(const char* who, int64_t m, int cin, int cout, int plan, Plan& p) {
  NR_REQUIRE(m >= 0 && m < (INT64_C(1) << 31), m < 0 ? NRHIP_ERR_INVALID_ARG : NRHIP_ERR_UNSUPPORTED,
             "%s: %lld pixels outside [0, 2^31)", who, (long long)m);
  NR_REQUIRE(vgg_channels(cin) && vgg_channels(cout) && !(cin == 3 && cout == 3), NRHIP_ERR_UNSUPPORTED,
             "%s: channels %d -> %d unsupported (each of 3, 64, 128, 256, 512; not 3 -> 3)", who, cin, cout);
  NR_REQUIRE(plan >= 0 && plan <= 2, NRHIP_ERR_INVALID_ARG, "%s: plan %d not in {0: auto, 1, 2: 32-pixel blocks per wave}", who,
             plan);
  p = auto_plan(m, cout);
  if (plan) p.mt = plan;
  p.waves = ((m + 32 * p.mt - 1) / (32 * p.mt)) * (p.nb_n / p.nt);
  return NRHIP_OK;
}

// ---- maxpool ------------------------------------------------------------------------------------------------------------
// the first maximum of the window in row-major order, NaN taken like torch: (v > best || isnan(v))
__device__ __forceinline__ void window_argmax(const Frag (&v)[4], int e, float& best, int& arg) {
  best = (float)v[0].h[e];
  arg = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const float x = (float)v[k].h[e];
    if (x > best || x != x) best = x, arg = k;
  }
}

__device__ __forceinline__ void window_load(const _Float16* __restrict__ in, int64_t b, int yo, int xo, int H, int W, int C,
                                            int cg, Frag (&v)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    v[k].u = *(const uint4*)(in + ((b * H + 2 * yo + (k >> 1)) * W + 2 * xo + (k & 1)) * C + cg * 8);
}

__global__ __launch_bounds__(kBlock) void maxpool_fwd_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out,
                                                             int64_t B, int H, int W, int C) {
  const int Ho = H >> 1, Wo = W >> 1, G = C >> 3;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= B * Ho * Wo * G) return;
  const int cg = (int)(t % G);
  const int64_t pix = t / G;
  const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho);
  const int64_t b = pix / ((int64_t)Wo * Ho);
  Frag v[4], o;
  window_load(in, b, yo, xo, H, W, C, cg, v);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float best;
    int arg;
    window_argmax(v, e, best, arg);
    o.h[e] = v[arg].h[e];
  }
  *(uint4*)(out + pix * C + cg * 8) = o.u;
}

// one thread per (window of the ceil grid, 8 channels): it writes the up to four input positions it covers, so the dropped
// odd row / column is written (zero) too
__global__ __launch_bounds__(kBlock) void maxpool_bwd_kernel(const _Float16* __restrict__ in, const _Float16* __restrict__ gout,
                                                             const float* __restrict__ in_state, float* __restrict__ out_state,
                                                             _Float16* __restrict__ gin, int64_t B, int H, int W, int C) {
  const int Ho = H >> 1, Wo = W >> 1, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1, G = C >> 3;
  float p = 1.f, s_in = 1.f, amax = 0.f;
  if (in_state) {
    amax = in_state[0];
    p = pow2_norm(amax);
    s_in = in_state[1];
  }
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t == 0 && out_state) out_state[0] = amax * p, out_state[1] = s_in * p;  // a routing: the maximum moves with it
  if (t >= B * Hc * Wc * G) return;
  const int cg = (int)(t % G);
  const int64_t pix = t / G;
  const int xo = (int)(pix % Wc), yo = (int)((pix / Wc) % Hc);
  const int64_t b = pix / ((int64_t)Wc * Hc);
  Frag o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k].u = uint4{0u, 0u, 0u, 0u};
  if (yo < Ho && xo < Wo) {
    Frag v[4], g;
    window_load(in, b, yo, xo, H, W, C, cg, v);
    g.u = *(const uint4*)(gout + ((b * Ho + yo) * Wo + xo) * C + cg * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float best;
      int arg;
      window_argmax(v, e, best, arg);
      const _Float16 ge = (_Float16)((float)g.h[e] * p);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k == arg) o[k].h[e] = ge;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = 2 * yo + (k >> 1), x = 2 * xo + (k & 1);
    if (y < H && x < W) *(uint4*)(gin + ((b * H + y) * W + x) * C + cg * 8) = o[k].u;
  }
}

// ---- L1 feature loss ----------------------------------------------------------------------------------------------------
// (a, b, c, d) over the four waves as ((a + b) + c) + d, lanes by a fixed shuffle tree: one order, every run
__device__ __forceinline__ double block_sum_fixed(double s, double* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = s;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// a thread's 8 consecutive elements: one 16-byte load where the tensors allow it, element by element otherwise
__device__ __forceinline__ int load8(const _Float16* __restrict__ p, int64_t i, int64_t n, bool vec, Frag& f) {
  f.u = uint4{0u, 0u, 0u, 0u};
  if (i >= n) return 0;
  const int cnt = (int)(n - i < 8 ? n - i : 8);
  if (vec && cnt == 8) {
    f.u = *(const uint4*)(p + i);
  } else {
    for (int e = 0; e < cnt; ++e) f.h[e] = p[i + e];
  }
  return cnt;
}
__device__ __forceinline__ void store8(_Float16* __restrict__ p, int64_t i, int cnt, bool vec, const Frag& f) {
  if (vec && cnt == 8) {
    *(uint4*)(p + i) = f.u;
  } else {
    for (int e = 0; e < cnt; ++e) p[i + e] = f.h[e];
  }
}

__global__ __launch_bounds__(kBlock) void l1_partial_kernel(const _Float16* __restrict__ fx, const _Float16* __restrict__ fy,
                                                            int64_t n, int vec, double* __restrict__ partial) {
  __shared__ double sh[4];
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 8;
  Frag a, b;
  const int cnt = load8(fx, i, n, vec, a);
  load8(fy, i, n, vec, b);
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e < cnt) s += fabs((double)a.h[e] - (double)b.h[e]);  // exact difference, float64 sum
  const double bs = block_sum_fixed(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = bs;
}

__global__ __launch_bounds__(kBlock) void l1_final_kernel(const double* __restrict__ partial, int64_t nparts, int64_t n,
                                                          float weight, const float* __restrict__ accum,
                                                          float* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < nparts; k += kBlock) s += partial[k];
  const double total = block_sum_fixed(s, sh);
  if (threadIdx.x == 0) *out = (float)((accum ? (double)*accum : 0.0) + (double)weight * (total / (double)n));
}

// out = S_out * (c * sign(fx - fy) [fx > 0] + above / S_above), c = weight * g / n.  Without `above`: S_out brings |c| into
// [0.5, 1) and the one rounding to fp16 is done by hand from float64.  With it: S_out brings |c| + amax_above / S_above into
// [0.5, 1), both terms are brought to S_out (powers of two: exact) and added in fp32.
__global__ __launch_bounds__(kBlock) void l1_bwd_kernel(const _Float16* __restrict__ fx, const _Float16* __restrict__ fy,
                                                        int64_t n, float weight, const float* __restrict__ g, int mask_fx,
                                                        const _Float16* __restrict__ above, const float* __restrict__ above_state,
                                                        int vec, float* __restrict__ out_state, _Float16* __restrict__ out) {
  __shared__ uint32_t shmax[4];
  const double c = (double)weight * (double)g[0] / (double)n;
  const float cabs = (float)fabs(c);
  float s_out, r_above = 0.f;
  if (above) {
    const float s_a = above_state[1];
    s_out = pow2_norm(cabs + above_state[0] / s_a);
    r_above = s_out / s_a;
  } else {
    s_out = pow2_norm(cabs);
  }
  // c * S_out in [0.5, 1): fp16 has 11 significant bits there, so its nearest-even neighbour is rint(v * 2^11) / 2^11
  const double cs = c * (double)s_out;
  const float cf = above ? (float)cs : (float)(rint(cs * 2048.0) / 2048.0);
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 8;
  Frag a, b, u, o;
  const int cnt = load8(fx, i, n, vec, a);
  load8(fy, i, n, vec, b);
  if (above) load8(above, i, n, vec, u);
  uint32_t lmax = 0u;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = (float)a.h[e], y = (float)b.h[e];
    float v = x > y ? cf : (x < y ? -cf : (x == y ? 0.f : cf * (x - y)));  // (NaN features poison)
    if (mask_fx && !(x > 0.f)) v = 0.f;
    if (above) v += (float)u.h[e] * r_above;
    o.h[e] = (_Float16)v;
    if (e < cnt) {
      const uint32_t bts = abs_bits(o.h[e]);
      lmax = bts > lmax ? bts : lmax;
    }
  }
  store8(out, i, cnt, vec, o);
  if (out_state) {
    lmax = wave_max_bits(lmax);
    if ((threadIdx.x & 63) == 0) shmax[threadIdx.x >> 6] = lmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t m = shmax[0];
      for (int k = 1; k < 4; ++k) m = shmax[k] > m ? shmax[k] : m;
      if (m) atomicMax(reinterpret_cast<uint32_t*>(out_state), m);
      if (blockIdx.x == 0) out_state[1] = s_out;
    }
  }
}

// ---- the image side -----------------------------------------------------------------------------------------------------
// cat([x, y]) of two fp32 NHWC [n_pixels, 3] images -> fp16 [2 n_pixels, 16], channels 3..15 zero
__global__ __launch_bounds__(kBlock) void stage_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t n_pixels,
                                                       _Float16* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= 2 * n_pixels) return;
  const float* src = t < n_pixels ? x + 3 * t : y + 3 * (t - n_pixels);
  Frag f;
  f.u = uint4{0u, 0u, 0u, 0u};
  f.h[0] = (_Float16)src[0], f.h[1] = (_Float16)src[1], f.h[2] = (_Float16)src[2];
  uint4* dst = (uint4*)(out + t * kImgC);
  dst[0] = f.u;
  dst[1] = uint4{0u, 0u, 0u, 0u};
}

// the fp16 gradient of the staged image at its working scale -> fp32 [n_pixels, 3], times 1 / S (exact)
__global__ __launch_bounds__(kBlock) void image_grad_kernel(const _Float16* __restrict__ g, const float* __restrict__ state,
                                                            int64_t n_pixels, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= 3 * n_pixels) return;
  const int64_t pix = t / 3;
  const int c = (int)(t - 3 * pix);
  const float inv = 1.f / state[1];
  out[t] = (float)g[pix * kImgC + c] * inv;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace nrhip

using namespace nrhip;

extern "C" int nrhip_conv3x3_plan(int64_t n_pixels, int32_t cin, int32_t cout, int32_t plan, int32_t* pixel_blocks,
                                  int32_t* channel_blocks, int64_t* waves) {
  NR_REQUIRE(pixel_blocks && channel_blocks && waves, NRHIP_ERR_INVALID_ARG, "conv3x3_plan: NULL out-pointer");
  Plan p;
  if (int rc = resolve_plan("conv3x3_plan", n_pixels, cin, cout, plan, p)) return rc;
  *pixel_blocks = p.mt, *channel_blocks = p.nt, *waves = p.waves;
  return NRHIP_OK;
}

extern "C" int nrhip_conv3x3_pack_bytes(int32_t cout, int32_t cin, int32_t mode, int64_t* bytes) {
  NR_REQUIRE(bytes, NRHIP_ERR_INVALID_ARG, "conv3x3_pack_bytes: bytes is NULL");
  NR_REQUIRE(mode == 0 || mode == 1, NRHIP_ERR_INVALID_ARG, "conv3x3_pack_bytes: mode %d not in {0, 1}", mode);
  NR_REQUIRE(vgg_channels(cin) && vgg_channels(cout) && !(cin == 3 && cout == 3), NRHIP_ERR_UNSUPPORTED,
             "conv3x3_pack_bytes: weight [%d, %d, 3, 3] unsupported (each of 3, 64, 128, 256, 512; not 3 x 3)", cout, cin);
  const int k = stored_channels(mode == 0 ? cin : cout), n = stored_channels(mode == 0 ? cout : cin);
  *bytes = (int64_t)9 * (k / 16) * ((n + 31) / 32) * 64 * 16;
  return NRHIP_OK;
}

extern "C" int nrhip_conv3x3_pack(const float* weight, int32_t cout, int32_t cin, int32_t mode, void* wfrag, void* stream) {
  int64_t bytes = 0;
  if (int rc = nrhip_conv3x3_pack_bytes(cout, cin, mode, &bytes)) return rc;
  NR_REQUIRE(weight && wfrag, NRHIP_ERR_INVALID_ARG, "conv3x3_pack: NULL pointer");
  NR_REQUIRE(aligned16(wfrag), NRHIP_ERR_INVALID_ARG, "conv3x3_pack: wfrag is not 16-byte aligned");
  const int k = stored_channels(mode == 0 ? cin : cout), n = stored_channels(mode == 0 ? cout : cin);
  const int64_t threads = bytes / 16;
  conv3_pack_kernel<<<grid_for(threads, kBlock), kBlock, 0, (hipStream_t)stream>>>(weight, cout, cin, mode, k / 16,
                                                                                    (n + 31) / 32, (uint4*)wfrag);
  return check_launch("conv3x3_pack");
}

extern "C" int nrhip_conv3x3(const void* in, const void* wfrag, const float* bias, const void* mask, const float* in_state,
                             float* out_state, void* out, int32_t b, int32_t h, int32_t w, int32_t cin, int32_t cout,
                             int32_t relu, int32_t plan, void* stream) {
  NR_REQUIRE(b >= 0 && h >= 1 && w >= 1, NRHIP_ERR_INVALID_ARG, "conv3x3: bad shape %d x %d x %d", b, h, w);
  const int64_t m = (int64_t)b * h * w;
  Plan p;
  if (int rc = resolve_plan("conv3x3", m, cin, cout, plan, p)) return rc;
  NR_REQUIRE(!(bias && cout == 3), NRHIP_ERR_UNSUPPORTED, "conv3x3: no bias on the 3-channel output");
  if (m == 0) return NRHIP_OK;
  NR_REQUIRE(in && wfrag && out, NRHIP_ERR_INVALID_ARG, "conv3x3: NULL pointer");
  NR_REQUIRE(aligned16(in) && aligned16(wfrag), NRHIP_ERR_INVALID_ARG, "conv3x3: in / wfrag not 16-byte aligned");
  const int cin_s = stored_channels(cin), cout_s = stored_channels(cout);
  NR_REQUIRE(m * (cin_s > cout_s ? cin_s : cout_s) < (INT64_C(1) << 40), NRHIP_ERR_UNSUPPORTED, "conv3x3: tensor too large");
  const unsigned blocks = (unsigned)((p.waves + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
#define NR_CONV3_KU(MT, NT, KU)                                                                                           \
  conv3_kernel<MT, NT, KU><<<blocks, kBlock, 0, st>>>((const _Float16*)in, (const uint4*)wfrag, bias,                     \
                                                      (const _Float16*)mask, in_state, out_state, (_Float16*)out, h, w,   \
                                                      cin_s, cout_s, p.nb_n, relu ? 1 : 0, m)
#define NR_CONV3(MT, NT)                      \
  do {                                        \
    if ((cin_s / 16) % kKU == 0)              \
      NR_CONV3_KU(MT, NT, kKU);               \
    else                                      \
      NR_CONV3_KU(MT, NT, 1);                 \
  } while (0)
  if (p.mt == 2 && p.nt == 2) NR_CONV3(2, 2);
  else if (p.mt == 1 && p.nt == 2) NR_CONV3(1, 2);
  else if (p.mt == 2) NR_CONV3(2, 1);
  else NR_CONV3(1, 1);
#undef NR_CONV3
#undef NR_CONV3_KU
  return check_launch("conv3x3");
}

static int pool_args(const char* who, const void* a, const void* b2, int64_t b, int32_t h, int32_t w, int32_t c) {
  NR_REQUIRE(b >= 0 && h >= 1 && w >= 1 && c >= 8 && c % 8 == 0, NRHIP_ERR_INVALID_ARG,
             "%s: bad shape %lld x %d x %d x %d (channels must be a multiple of 8)", who, (long long)b, h, w, c);
  NR_REQUIRE(b * h * w < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "%s: >= 2^31 pixels", who);
  if (b == 0) return NRHIP_OK;
  NR_REQUIRE(a && b2, NRHIP_ERR_INVALID_ARG, "%s: NULL pointer", who);
  NR_REQUIRE(aligned16(a) && aligned16(b2), NRHIP_ERR_INVALID_ARG, "%s: tensor not 16-byte aligned", who);
  return NRHIP_OK;
}

extern "C" int nrhip_maxpool2_fwd(const void* in, void* out, int64_t b, int32_t h, int32_t w, int32_t c, void* stream) {
  if (int rc = pool_args("maxpool2_fwd", in, out, b, h, w, c)) return rc;
  const int64_t threads = b * (h / 2) * (w / 2) * (c / 8);
  if (threads == 0) return NRHIP_OK;
  maxpool_fwd_kernel<<<grid_for(threads, kBlock), kBlock, 0, (hipStream_t)stream>>>((const _Float16*)in, (_Float16*)out, b, h, w,
                                                                                     c);
  return check_launch("maxpool2_fwd");
}

extern "C" int nrhip_maxpool2_bwd(const void* in, const void* grad_out, const float* in_state, float* out_state, void* grad_in,
                                  int64_t b, int32_t h, int32_t w, int32_t c, void* stream) {
  if (int rc = pool_args("maxpool2_bwd", in, grad_in, b, h, w, c)) return rc;
  if (b == 0) return NRHIP_OK;
  NR_REQUIRE((grad_out && aligned16(grad_out)) || h < 2 || w < 2, NRHIP_ERR_INVALID_ARG,
             "maxpool2_bwd: grad_out is NULL or not 16-byte aligned");
  const int64_t threads = b * ((h + 1) / 2) * ((w + 1) / 2) * (c / 8);
  maxpool_bwd_kernel<<<grid_for(threads, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      (const _Float16*)in, (const _Float16*)grad_out, in_state, out_state, (_Float16*)grad_in, b, h, w, c);
  return check_launch("maxpool2_bwd");
}

extern "C" int nrhip_l1_feature_workspace(int64_t n, int64_t* bytes) {
  NR_REQUIRE(bytes, NRHIP_ERR_INVALID_ARG, "l1_feature_workspace: bytes is NULL");
  NR_REQUIRE(n >= 0, NRHIP_ERR_INVALID_ARG, "l1_feature_workspace: negative count");
  *bytes = (n + kL1Items - 1) / kL1Items * 8;
  return NRHIP_OK;
}

extern "C" int nrhip_l1_feature_fwd(const void* fx, const void* fy, int64_t n, float weight, const float* accum,
                                    void* workspace, int64_t workspace_bytes, float* out, void* stream) {
  NR_REQUIRE(n >= 1 && n < (INT64_C(1) << 40), NRHIP_ERR_INVALID_ARG, "l1_feature_fwd: %lld elements outside [1, 2^40)",
             (long long)n);
  NR_REQUIRE(fx && fy && out, NRHIP_ERR_INVALID_ARG, "l1_feature_fwd: NULL pointer");
  const int64_t nparts = (n + kL1Items - 1) / kL1Items;
  NR_REQUIRE(workspace && workspace_bytes >= nparts * 8 && ((uintptr_t)workspace & 7) == 0, NRHIP_ERR_INVALID_ARG,
             "l1_feature_fwd: workspace is NULL, misaligned or smaller than nrhip_l1_feature_workspace asks for");
  hipStream_t st = (hipStream_t)stream;
  const int vec = aligned16(fx) && aligned16(fy);
  l1_partial_kernel<<<(unsigned)nparts, kBlock, 0, st>>>((const _Float16*)fx, (const _Float16*)fy, n, vec, (double*)workspace);
  l1_final_kernel<<<1, kBlock, 0, st>>>((const double*)workspace, nparts, n, weight, accum, out);
  return check_launch("l1_feature_fwd");
}

extern "C" int nrhip_l1_feature_bwd(const void* fx, const void* fy, int64_t n, float weight, const float* grad_loss,
                                    int32_t mask_fx, const void* above, const float* above_state, float* out_state,
                                    void* grad_fx, void* stream) {
  NR_REQUIRE(n >= 1 && n < (INT64_C(1) << 40), NRHIP_ERR_INVALID_ARG, "l1_feature_bwd: %lld elements outside [1, 2^40)",
             (long long)n);
  NR_REQUIRE(fx && fy && grad_loss && grad_fx, NRHIP_ERR_INVALID_ARG, "l1_feature_bwd: NULL pointer");
  NR_REQUIRE(!above || above_state, NRHIP_ERR_INVALID_ARG, "l1_feature_bwd: `above` without its state");
  const int vec = aligned16(fx) && aligned16(fy) && aligned16(grad_fx) && (!above || aligned16(above));
  const int64_t nparts = (n + kL1Items - 1) / kL1Items;
  l1_bwd_kernel<<<(unsigned)nparts, kBlock, 0, (hipStream_t)stream>>>((const _Float16*)fx, (const _Float16*)fy, n, weight,
                                                                        grad_loss, mask_fx ? 1 : 0, (const _Float16*)above,
                                                                        above_state, vec, out_state, (_Float16*)grad_fx);
  return check_launch("l1_feature_bwd");
}

extern "C" int nrhip_vgg_stage_images(const float* x, const float* y, int64_t n_pixels, void* out, void* stream) {
  NR_REQUIRE(n_pixels >= 0 && n_pixels < (INT64_C(1) << 30), NRHIP_ERR_INVALID_ARG, "vgg_stage_images: bad pixel count");
  if (n_pixels == 0) return NRHIP_OK;
  NR_REQUIRE(x && y && out && aligned16(out), NRHIP_ERR_INVALID_ARG, "vgg_stage_images: NULL or misaligned pointer");
  stage_kernel<<<grid_for(2 * n_pixels, kBlock), kBlock, 0, (hipStream_t)stream>>>(x, y, n_pixels, (_Float16*)out);
  return check_launch("vgg_stage_images");
}

extern "C" int nrhip_vgg_image_grad(const void* grad16, const float* state, int64_t n_pixels, float* grad, void* stream) {
  NR_REQUIRE(n_pixels >= 0 && n_pixels < (INT64_C(1) << 30), NRHIP_ERR_INVALID_ARG, "vgg_image_grad: bad pixel count");
  if (n_pixels == 0) return NRHIP_OK;
  NR_REQUIRE(grad16 && state && grad, NRHIP_ERR_INVALID_ARG, "vgg_image_grad: NULL pointer");
  image_grad_kernel<<<grid_for(3 * n_pixels, kBlock), kBlock, 0, (hipStream_t)stream>>>((const _Float16*)grad16, state, n_pixels,
                                                                                        grad);
  return check_launch("vgg_image_grad");
}
