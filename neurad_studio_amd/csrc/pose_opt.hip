// Camera pose correction (`camera_optimizer.mode = "SO3xR3"`, cameras/camera_optimizers.py:139-182 with
// cameras/lie_groups.py:24-58): per ray a gather of its camera's six parameters, the exponential map of SO(3) x R^3 and a
// 3 x 3 product -- in the reference about 25 small launches forwards, and backwards the same ops ending in an index
// backward that lands tens of thousands of rays on a few hundred rows.  Here:
//
//   pose_apply_kernel     forward, lane = ray: a = fl32(pose[c] * weights), R = f1 K + f2 K^2 + I in the reference's fp32
//                         operation order (rotation() below; -ffp-contract=off), o' = o + a[0:3], d' = R d.
//   pose_clear_kernel     backward pass 1: zeroes the workspace [n_cameras, 16] 64-bit words (the FIRST pass clears; nothing
//                         has to be left clean for a next call, so a fresh allocation per call is fine).
//   pose_max_kernel       pass 2: per camera the largest finite |term| of its rays as an unsigned integer max on the bits of
//                         the non-negative float (word 12), an integer OR of "a ray of this camera has a non-finite term"
//                         (word 13).  The twelve terms of a ray are g_o[0..2] and g_d[i] d[j]; their largest magnitude is
//                         max(max|g_o|, max|g_d| max|d|), taken in double and rounded UP to fp32.
//   pose_accumulate_kernel pass 3: every term in double (the product of two fp32 is exact there) times the exact power of two
//                         2^(B - e_c), rounded to the nearest int64, added with a 64-bit integer atomic add (words 0..11).
//                         2^(e_c) is the smallest power of two above the camera's max, B = 62 - ceil(log2 max(r, 2)): |q| <=
//                         2^B and r of them cannot overflow.  Integer sums: any order of the rays gives the same bits.
//   pose_finish_kernel    pass 4, lane = camera: the sums back to double, the chain through the exponential map in double from
//                         the fp32 parameters, times weights, rounded to fp32 once.  No ray: exact zeros.  Flag set: six NaN.
//   pose_input_grad_kernel (only when asked for) lane = ray: grad_o_in = g_o, grad_d_in = R^T g_d.
//
// The atomics (guide: shape an atomic wave-instruction as whole 128-byte rows): a wave whose 64 rays share one camera -- patch
// batches have runs of 1024 -- reduces the twelve integers inside the wave (wave_scan.h) and issues ONE 128-byte row of adds;
// a mixed wave (lidar rays) passes its 64 x 12 integers through LDS so that the twelve slots of a ray sit in neighbouring
// lanes: four rays = four whole rows per wave-instruction, sixteen instructions per wave, instead of one lane per row.
// No float atomics, no host read, no allocation, capturable in a graph.  A camera index outside [0, n_cameras) is a
// precondition violation; such a ray is neither read from nor written to the parameter rows or the workspace: it passes
// through unchanged and contributes nothing.
#include <cmath>

#include "common.h"
#include "wave_scan.h"

namespace nrhip {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRowWords = 16;  // one 128-byte row per camera
constexpr int kTerms = 12;     // g_o[0..2], then g_d[i] d[j] at 3 + 3 i + j
constexpr int kMaxWord = 12, kFlagWord = 13;
constexpr float kClamp = 1e-4f;  // torch.clamp(nrms, 1e-4) on an fp32 tensor

struct MaxOp {
  template <class T>
  static __device__ __forceinline__ T id() { return T(0); }
  template <class T>
  static __device__ __forceinline__ T op(T a, T b) { return a > b ? a : b; }
};

__device__ __forceinline__ bool camera_ok(int64_t c, int32_t n_cameras) { return (uint64_t)c < (uint64_t)n_cameras; }

__device__ __forceinline__ void load_adjustment(const float* __restrict__ pose, const float* __restrict__ weights, int64_t c,
                                                float (&a)[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) a[k] = weights ? __fmul_rn(pose[c * 6 + k], weights[k]) : pose[c * 6 + k];
}

// the fp32 squared norm both directions decide the clamp on
__device__ __forceinline__ float sq_norm(float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
}

// lie_groups.py:35-56 in its own order.  K = skew(w): K v = w x v; K^2 as the reference's bmm(skews, skews) forms it
__device__ __forceinline__ void rotation(float x, float y, float z, float (&R)[9]) {
  const float nrms = sq_norm(x, y, z);
  const float th = sqrtf(nrms < kClamp ? kClamp : nrms);  // (a NaN stays one, as in torch.clamp)
  const float inv = 1.0f / th;
  const float f1 = inv * sinf(th);
  const float f2 = inv * inv * (1.0f - cosf(th));
  const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
  const float K2[9] = {-(z * z) - y * y, x * y, z * x, x * y, -(z * z) - x * x, z * y, x * z, y * z, -(y * y) - x * x};
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (f1 * K[i] + f2 * K2[i]) + (i % 4 == 0 ? 1.f : 0.f);
}

__global__ __launch_bounds__(kBlock) void pose_apply_kernel(const float* __restrict__ pose, const float* __restrict__ weights,
                                                            int32_t n_cameras, const int64_t* __restrict__ idx,
                                                            const float* __restrict__ o, const float* __restrict__ d, int64_t r,
                                                            float* __restrict__ oo, float* __restrict__ od) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= r) return;
  const int64_t c = idx[i];
  float ox = o[i * 3], oy = o[i * 3 + 1], oz = o[i * 3 + 2];
  float dx = d[i * 3], dy = d[i * 3 + 1], dz = d[i * 3 + 2];
  if (camera_ok(c, n_cameras)) {
    float a[6], R[9];
    load_adjustment(pose, weights, c, a);
    rotation(a[3], a[4], a[5], R);
    ox = ox + a[0], oy = oy + a[1], oz = oz + a[2];
    const float nx = (R[0] * dx + R[1] * dy) + R[2] * dz;
    const float ny = (R[3] * dx + R[4] * dy) + R[5] * dz;
    const float nz = (R[6] * dx + R[7] * dy) + R[8] * dz;
    dx = nx, dy = ny, dz = nz;
  }
  oo[i * 3] = ox, oo[i * 3 + 1] = oy, oo[i * 3 + 2] = oz;
  od[i * 3] = dx, od[i * 3 + 1] = dy, od[i * 3 + 2] = dz;
}

__global__ __launch_bounds__(kBlock) void pose_clear_kernel(unsigned long long* __restrict__ ws, int64_t n_words) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n_words) ws[i] = 0ull;
}

// one ray's share of the backward: its camera (-1: out of range, or no ray in this lane), its nine inputs, whether all of its
// terms are finite and representable (|term| <= FLT_MAX), and the largest |term|
struct RayTerms {
  int64_t c;
  float go[3], gd[3], d[3];
  bool finite;
  double amax;
};
__device__ __forceinline__ RayTerms load_terms(int64_t i, int64_t r, int32_t n_cameras, const int64_t* __restrict__ idx,
                                               const float* __restrict__ d, const float* __restrict__ g_o,
                                               const float* __restrict__ g_d) {
  RayTerms t;
  t.c = -1, t.finite = true, t.amax = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) t.go[k] = t.gd[k] = t.d[k] = 0.f;
  if (i < r) {
    const int64_t c = idx[i];
    if (camera_ok(c, n_cameras)) {
      t.c = c;
      float mo = 0.f, mg = 0.f, md = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        t.go[k] = g_o[i * 3 + k], t.gd[k] = g_d[i * 3 + k], t.d[k] = d[i * 3 + k];
        t.finite = t.finite && isfinite(t.go[k]) && isfinite(t.gd[k]) && isfinite(t.d[k]);
        mo = fmaxf(mo, fabsf(t.go[k])), mg = fmaxf(mg, fabsf(t.gd[k])), md = fmaxf(md, fabsf(t.d[k]));
      }
      t.amax = fmax((double)mo, (double)mg * (double)md);
      t.finite = t.finite && t.amax <= 3.4028234663852886e38;
    }
  }
  return t;
}

// the wave's rays all belong to one valid camera (lanes past the end of the batch do not count)?  -> that camera, or -1
__device__ __forceinline__ int64_t wave_camera(int64_t c, bool in_range) {
  const int64_t c0 = (int64_t)wscan::first((long long)c);
  return __ballot(in_range && c != c0) == 0ull ? c0 : -1;
}

__global__ __launch_bounds__(kBlock) void pose_max_kernel(int32_t n_cameras, const int64_t* __restrict__ idx,
                                                          const float* __restrict__ d, const float* __restrict__ g_o,
                                                          const float* __restrict__ g_d, int64_t r,
                                                          unsigned long long* __restrict__ ws) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const RayTerms t = load_terms(i, r, n_cameras, idx, d, g_o, g_d);
  const bool bad = t.c >= 0 && !t.finite;
  uint32_t key = 0u;
  if (t.c >= 0 && t.finite) {  // amax rounded UP to fp32 (amax <= FLT_MAX: the step cannot leave the finite range)
    const float f = (float)t.amax;
    key = __float_as_uint(f) + ((double)f < t.amax ? 1u : 0u);
  }
  const int64_t cw = wave_camera(t.c, i < r);
  if (cw >= 0) {
    const uint32_t wkey = wscan::reduce<MaxOp>(key);
    const bool wbad = __ballot(bad) != 0ull;
    if (lane == 0) {
      if (wkey) atomicMax(ws + cw * kRowWords + kMaxWord, (unsigned long long)wkey);
      if (wbad) atomicOr(ws + cw * kRowWords + kFlagWord, 1ull);
    }
  } else if (t.c >= 0) {
    if (key) atomicMax(ws + t.c * kRowWords + kMaxWord, (unsigned long long)key);
    if (bad) atomicOr(ws + t.c * kRowWords + kFlagWord, 1ull);
  }
}

// 2^p as a double, p inside the normal range
__device__ __forceinline__ double pow2(int p) { return __longlong_as_double((long long)(p + 1023) << 52); }
// e_c of a max cell: the key's float is below 2^(E - 126), E its biased exponent (E = 0: zero or a denormal, below 2^-126)
__device__ __forceinline__ int cell_exponent(unsigned long long cell) { return (int)((uint32_t)cell >> 23) - 126; }

__global__ __launch_bounds__(kBlock) void pose_accumulate_kernel(int32_t n_cameras, const int64_t* __restrict__ idx,
                                                                 const float* __restrict__ d, const float* __restrict__ g_o,
                                                                 const float* __restrict__ g_d, int64_t r, int B,
                                                                 unsigned long long* __restrict__ ws) {
  __shared__ long long sq[kWaves][64][kTerms];
  __shared__ long long sc[kWaves][64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RayTerms t = load_terms(i, r, n_cameras, idx, d, g_o, g_d);
  const bool live = t.c >= 0 && t.finite;
  long long q[kTerms];
#pragma unroll
  for (int k = 0; k < kTerms; ++k) q[k] = 0;
  if (live) {
    const double scale = pow2(B - cell_exponent(ws[t.c * kRowWords + kMaxWord]));
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = __double2ll_rn((double)t.go[k] * scale);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) q[3 + 3 * a + b] = __double2ll_rn((double)t.gd[a] * (double)t.d[b] * scale);
  }
  const int64_t cw = wave_camera(t.c, i < r);
  if (cw >= 0) {
    long long mine = 0;
#pragma unroll
    for (int k = 0; k < kTerms; ++k) {
      const long long total = wscan::reduce<wscan::Add>(q[k]);
      mine = lane == k ? total : mine;
    }
    if (lane < kTerms && mine != 0) atomicAdd(ws + cw * kRowWords + lane, (unsigned long long)mine);
  } else if (__ballot(live) != 0ull) {
#pragma unroll
    for (int k = 0; k < kTerms; ++k) sq[wave][lane][k] = q[k];
    sc[wave][lane] = live ? t.c : -1;
    wave_fence();
    const int slot = lane & 15;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int ray = it * 4 + (lane >> 4);
      const long long c = sc[wave][ray];
      if (slot < kTerms && c >= 0) {
        const long long v = sq[wave][ray][slot];
        if (v != 0) atomicAdd(ws + c * kRowWords + slot, (unsigned long long)v);
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void pose_finish_kernel(const float* __restrict__ pose, const float* __restrict__ weights,
                                                             int32_t n_cameras, int B,
                                                             const unsigned long long* __restrict__ ws,
                                                             float* __restrict__ grad_pose) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_cameras) return;
  const unsigned long long* row = ws + c * kRowWords;
  float* out = grad_pose + c * 6;
  if (row[kFlagWord]) {
    const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = nan;
    return;
  }
  const double unit = pow2(cell_exponent(row[kMaxWord]) - B);
  double S[kTerms];
#pragma unroll
  for (int k = 0; k < kTerms; ++k) S[k] = (double)(long long)row[k] * unit;
  float a[6];
  load_adjustment(pose, weights, c, a);
  const bool clamped = sq_norm(a[3], a[4], a[5]) < kClamp;  // the forward's own decision
  const double w[3] = {(double)a[3], (double)a[4], (double)a[5]};
  const double* A = S + 3;  // A[3 i + j] = sum g_d[i] d[j] = dL/dR_ij
  const double n = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double th = clamped ? sqrt((double)kClamp) : sqrt(n);
  const double s = sin(th), co = cos(th);
  const double f1 = s / th, f2 = (1.0 - co) / (th * th);
  // d f1 / d theta, d f2 / d theta: torch's clamp passes the gradient at nrms >= min, below it the factors are constants
  const double d1 = clamped ? 0.0 : (th * co - s) / (th * th);
  const double d2 = clamped ? 0.0 : (th * s - 2.0 * (1.0 - co)) / (th * th * th);
  // <A, K> = w . u;  <A, K^2> = w^T A w - n tr A, K^2 = w w^T - n I
  const double u[3] = {A[7] - A[5], A[2] - A[6], A[3] - A[1]};
  const double tr = A[0] + A[4] + A[8];
  double Aw[3], Atw[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Aw[k] = A[3 * k] * w[0] + A[3 * k + 1] * w[1] + A[3 * k + 2] * w[2];
    Atw[k] = A[k] * w[0] + A[3 + k] * w[1] + A[6 + k] * w[2];
  }
  const double wu = w[0] * u[0] + w[1] * u[1] + w[2] * u[2];
  const double wAw = w[0] * Aw[0] + w[1] * Aw[1] + w[2] * Aw[2];
  const double radial = clamped ? 0.0 : (d1 * wu + d2 * (wAw - n * tr)) / th;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double G = radial * w[k] + f1 * u[k] + f2 * (Aw[k] + Atw[k] - 2.0 * w[k] * tr);
    const double wt = weights ? (double)weights[k] : 1.0, wr = weights ? (double)weights[3 + k] : 1.0;
    out[k] = (float)(S[k] * wt) + 0.f;  // (+ 0: a camera without a ray gets +0, never -0)
    out[3 + k] = (float)(G * wr) + 0.f;
  }
}

__global__ __launch_bounds__(kBlock) void pose_input_grad_kernel(const float* __restrict__ pose,
                                                                 const float* __restrict__ weights, int32_t n_cameras,
                                                                 const int64_t* __restrict__ idx, const float* __restrict__ g_o,
                                                                 const float* __restrict__ g_d, int64_t r,
                                                                 float* __restrict__ gi_o, float* __restrict__ gi_d) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= r) return;
  if (gi_o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) gi_o[i * 3 + k] = g_o[i * 3 + k];
  }
  if (!gi_d) return;
  const int64_t c = idx[i];
  float gx = g_d[i * 3], gy = g_d[i * 3 + 1], gz = g_d[i * 3 + 2];
  if (camera_ok(c, n_cameras)) {
    float a[6], R[9];
    load_adjustment(pose, weights, c, a);
    rotation(a[3], a[4], a[5], R);
    const float nx = (R[0] * gx + R[3] * gy) + R[6] * gz;
    const float ny = (R[1] * gx + R[4] * gy) + R[7] * gz;
    const float nz = (R[2] * gx + R[5] * gy) + R[8] * gz;
    gx = nx, gy = ny, gz = nz;
  }
  gi_d[i * 3] = gx, gi_d[i * 3 + 1] = gy, gi_d[i * 3 + 2] = gz;
}

int validate_sizes(const char* who, int64_t r, int32_t n_cameras) {
  NR_REQUIRE(r >= 0 && n_cameras >= 0, NRHIP_ERR_INVALID_ARG, "%s: bad argument (r = %lld, n_cameras = %d)", who, (long long)r,
             n_cameras);
  NR_REQUIRE(r < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "%s: r >= 2^31", who);
  return NRHIP_OK;
}

unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace
}  // namespace nrhip

using namespace nrhip;

extern "C" int nrhip_pose_apply(const float* pose, const float* weights, int32_t n_cameras, const int64_t* camera_indices,
                                const float* origins, const float* directions, int64_t r, float* out_origins,
                                float* out_directions, void* stream) {
  if (int rc = validate_sizes("pose_apply", r, n_cameras)) return rc;
  if (r == 0 || n_cameras == 0) return NRHIP_OK;
  NR_REQUIRE(pose && camera_indices && origins && directions && out_origins && out_directions, NRHIP_ERR_INVALID_ARG,
             "pose_apply: a buffer is NULL");
  pose_apply_kernel<<<blocks(r), kBlock, 0, (hipStream_t)stream>>>(pose, weights, n_cameras, camera_indices, origins,
                                                                  directions, r, out_origins, out_directions);
  return check_launch("pose_apply");
}

extern "C" int nrhip_pose_apply_bwd_workspace(int64_t r, int32_t n_cameras, int64_t* bytes) {
  NR_REQUIRE(bytes, NRHIP_ERR_INVALID_ARG, "pose_apply_bwd_workspace: bytes is NULL");
  if (int rc = validate_sizes("pose_apply_bwd_workspace", r, n_cameras)) return rc;
  *bytes = (int64_t)n_cameras * kRowWords * 8;
  return NRHIP_OK;
}

extern "C" int nrhip_pose_apply_bwd(const float* pose, const float* weights, int32_t n_cameras, const int64_t* camera_indices,
                                    const float* directions, const float* grad_origins, const float* grad_directions, int64_t r,
                                    void* workspace, float* grad_pose, float* grad_in_origins, float* grad_in_directions,
                                    void* stream) {
  if (int rc = validate_sizes("pose_apply_bwd", r, n_cameras)) return rc;
  if (r == 0 || n_cameras == 0) return NRHIP_OK;
  NR_REQUIRE(pose && camera_indices && directions && grad_origins && grad_directions && grad_pose, NRHIP_ERR_INVALID_ARG,
             "pose_apply_bwd: a buffer is NULL");
  NR_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, NRHIP_ERR_INVALID_ARG,
             "pose_apply_bwd: workspace is NULL or not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* ws = (unsigned long long*)workspace;
  int lg = 1;  // ceil(log2 max(r, 2))
  while ((INT64_C(1) << lg) < r) ++lg;
  const int B = 62 - lg;
  const int64_t n_words = (int64_t)n_cameras * kRowWords;
  pose_clear_kernel<<<blocks(n_words), kBlock, 0, st>>>(ws, n_words);
  pose_max_kernel<<<blocks(r), kBlock, 0, st>>>(n_cameras, camera_indices, directions, grad_origins, grad_directions, r, ws);
  pose_accumulate_kernel<<<blocks(r), kBlock, 0, st>>>(n_cameras, camera_indices, directions, grad_origins, grad_directions, r,
                                                      B, ws);
  pose_finish_kernel<<<blocks(n_cameras), kBlock, 0, st>>>(pose, weights, n_cameras, B, ws, grad_pose);
  if (grad_in_origins || grad_in_directions)
    pose_input_grad_kernel<<<blocks(r), kBlock, 0, st>>>(pose, weights, n_cameras, camera_indices, grad_origins,
                                                        grad_directions, r, grad_in_origins, grad_in_directions);
  return check_launch("pose_apply_bwd");
}
