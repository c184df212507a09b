// Lidar scan evaluation: brute-force nearest neighbour and the chamfer distance of two point clouds
// (utils/math.py:745-798, called by NeuRADModel.get_image_metrics_and_images, models/neurad.py:614-618).
// The reference walks [1000, M] blocks of torch.cdist in its |a|^2 + |b|^2 - 2ab form: a few hundred launches per scan and
// a cancellation error of the order of the nearest squared distances themselves.  Here:
//
//   nearest_kernel<Q>   one lane owns Q query points in registers; the targets stream through LDS in tiles of kTile
//                       {x, y, z, pad} (16 bytes each).  Every lane of a wave reads the same LDS address (one broadcast
//                       ds_read_b128 per target) and spends 7 Q VALU operations on it: dx = qx - tx, dy, dz (three rounded
//                       subtractions), d = fma(dz, dz, fma(dy, dy, dx * dx)), best = fminf(best, d).  Never |a|^2 + |b|^2 - 2ab.
//                       An invalid target, and the tail of the last tile, is staged as x = +inf: its distance is +inf (NaN
//                       against an infinite query) and fminf never takes it.  A NaN distance (NaN in either point) is
//                       dropped by fminf too, so a NaN target is ignored by every query and a NaN query stays at +inf.
//   split               when the queries alone cannot fill the chip, blockIdx.y splits the target range into `split` runs of
//                       whole tiles.  The partial minima are combined with an unsigned atomicMin on the float's bit
//                       pattern (non-negative floats and +inf order as their bits do: the trick of occgrid_update.h's max),
//                       after an init pass that writes +inf / 0.  A minimum does not depend on order, so every plan
//                       (Q, split) gives bit-identical values, as does any permutation of the targets.
//   chamfer             both directions, then sum_kernel (per-block float64 partials and valid counts in a slab) and
//                       final_kernel (fixed-order final sum, one rounding to fp32).  No float atomics, no host read.
#include "common.h"

namespace nrhip {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = NRHIP_NEAREST_TILE;  // targets per LDS tile
constexpr int kSumItems = 2048;            // points per block of the chamfer sum: 8 rounds of 256 threads
constexpr int kMaxSplit = 64;
constexpr uint32_t kInfBits = 0x7f800000u;

template <int Q>
__global__ __launch_bounds__(kBlock) void nearest_kernel(const float* __restrict__ query, int stride_q,
                                                         const uint8_t* __restrict__ query_valid, int n,
                                                         const float* __restrict__ target, int stride_t,
                                                         const uint8_t* __restrict__ target_valid, int m,
                                                         int tiles_per_split, bool combine, float* __restrict__ out) {
  __shared__ float4 tile[kTile];
  const float inf = __uint_as_float(kInfBits);
  float qx[Q], qy[Q], qz[Q], best[Q];
  bool live[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int64_t i = ((int64_t)blockIdx.x * Q + q) * kBlock + threadIdx.x;
    live[q] = i < n && (!query_valid || query_valid[i] != 0);
    qx[q] = qy[q] = qz[q] = 0.f;
    if (live[q]) {
      const float* p = query + i * stride_q;
      qx[q] = p[0], qy[q] = p[1], qz[q] = p[2];
    }
    best[q] = inf;
  }
  const int64_t j_begin = (int64_t)blockIdx.y * tiles_per_split * kTile;
  const int64_t j_end = min(j_begin + (int64_t)tiles_per_split * kTile, (int64_t)m);
  for (int64_t base = j_begin; base < j_end; base += kTile) {
    __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
    for (int k = 0; k < kTile / kBlock; ++k) {
      const int slot = k * kBlock + threadIdx.x;
      const int64_t j = base + slot;
      float4 t = make_float4(inf, 0.f, 0.f, 0.f);
      if (j < j_end && (!target_valid || target_valid[j] != 0)) {
        const float* p = target + j * stride_t;
        t.x = p[0], t.y = p[1], t.z = p[2];
      }
      tile[slot] = t;
    }
    __syncthreads();
    const int count = (int)min((int64_t)kTile, j_end - base);
    const int full = (count + 3) & ~3;  // the tail is padded with +inf up to the tile's end: whole groups of 4 are safe
    for (int s = 0; s < full; s += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 t = tile[s + u];  // the same address in every lane: an LDS broadcast
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const float dx = __fsub_rn(qx[q], t.x), dy = __fsub_rn(qy[q], t.y), dz = __fsub_rn(qz[q], t.z);
          best[q] = fminf(best[q], fmaf(dz, dz, fmaf(dy, dy, __fmul_rn(dx, dx))));
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int64_t i = ((int64_t)blockIdx.x * Q + q) * kBlock + threadIdx.x;
    if (i >= n) continue;
    if (!combine) {
      out[i] = live[q] ? best[q] : 0.f;
    } else if (live[q]) {  // (the init pass wrote +inf, or 0 for an invalid query)
      atomicMin(reinterpret_cast<uint32_t*>(out) + i, __float_as_uint(best[q]));
    }
  }
}

__global__ __launch_bounds__(kBlock) void nearest_init_kernel(const uint8_t* __restrict__ valid, int n,
                                                              float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = (!valid || valid[i] != 0) ? __uint_as_float(kInfBits) : 0.f;
}

// (a, b, c, d) summed as ((a + b) + c) + d over the four waves, lanes by a fixed shuffle tree: one order, every run
__device__ __forceinline__ void block_sum_fixed(double s, long long c, double* sh_s, long long* sh_c, double& out_s,
                                                long long& out_c) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_down(s, off, 64);
    c += __shfl_down(c, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh_s[wave] = s, sh_c[wave] = c;
  __syncthreads();
  out_s = ((sh_s[0] + sh_s[1]) + sh_s[2]) + sh_s[3];
  out_c = sh_c[0] + sh_c[1] + sh_c[2] + sh_c[3];
}

// blocks [0, nb_a) sum a[0..n_a), blocks [nb_a, nb_a + nb_b) sum b[0..n_b): valid entries only, float64, plus their count
__global__ __launch_bounds__(kBlock) void sum_kernel(const float* __restrict__ a, const uint8_t* __restrict__ a_valid, int n_a,
                                                     int nb_a, const float* __restrict__ b,
                                                     const uint8_t* __restrict__ b_valid, int n_b,
                                                     double* __restrict__ psum, long long* __restrict__ pcnt) {
  __shared__ double sh_s[4];
  __shared__ long long sh_c[4];
  const bool first = (int)blockIdx.x < nb_a;
  const float* v = first ? a : b;
  const uint8_t* ok = first ? a_valid : b_valid;
  const int n = first ? n_a : n_b;
  const int64_t base = (int64_t)(first ? blockIdx.x : blockIdx.x - nb_a) * kSumItems;
  double s = 0.0;
  long long c = 0;
#pragma unroll
  for (int k = 0; k < kSumItems / kBlock; ++k) {
    const int64_t i = base + k * kBlock + threadIdx.x;
    if (i < n && (!ok || ok[i] != 0)) s += (double)v[i], ++c;
  }
  double bs;
  long long bc;
  block_sum_fixed(s, c, sh_s, sh_c, bs, bc);
  if (threadIdx.x == 0) psum[blockIdx.x] = bs, pcnt[blockIdx.x] = bc;
}

__global__ __launch_bounds__(kBlock) void final_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                       int nb_a, int nb_b, int normalize, float* __restrict__ result) {
  __shared__ double sh_s[4];
  __shared__ long long sh_c[4];
  double s = 0.0, t = 0.0;
  long long cs = 0, ct = 0;
  for (int i = threadIdx.x; i < nb_a; i += kBlock) s += psum[i], cs += pcnt[i];
  for (int i = threadIdx.x; i < nb_b; i += kBlock) t += psum[nb_a + i], ct += pcnt[nb_a + i];
  double s2t, t2s;
  long long n_s, n_t;
  block_sum_fixed(s, cs, sh_s, sh_c, s2t, n_s);
  __syncthreads();
  block_sum_fixed(t, ct, sh_s, sh_c, t2s, n_t);
  if (threadIdx.x == 0) *result = (float)((s2t + t2s) / (normalize ? (double)n_t : 1.0));  // IEEE: inf, or NaN for 0 / 0
}

struct Plan {
  int q, split, tiles_per_split;
};

// Q and the split from N and M alone.  A lane with 4 queries spends 28 VALU operations on every LDS read; fewer only where
// the queries do not fill a workgroup.  The split brings the grid to ~4 workgroups per CU (1024), in runs of whole tiles.
Plan auto_plan(int64_t n, int64_t m) {
  Plan p;
  p.q = n >= 4 * kBlock ? 4 : (n >= 2 * kBlock ? 2 : 1);
  const int64_t blocks = (n + (int64_t)kBlock * p.q - 1) / ((int64_t)kBlock * p.q);
  const int64_t tiles = (m + kTile - 1) / kTile;
  int64_t split = blocks >= 1024 ? 1 : (1024 + blocks - 1) / (blocks > 0 ? blocks : 1);
  split = split < kMaxSplit ? split : kMaxSplit;
  split = split < tiles ? split : tiles;
  p.split = (int)(split > 1 ? split : 1);
  return p;
}

int resolve_plan(const char* who, int32_t plan, int64_t n, int64_t m, Plan& p) {
  p = auto_plan(n, m);
  if (plan != 0) {
    p.q = plan & 0xff, p.split = (plan >> 8) & 0xffff;
    NR_REQUIRE((p.q == 1 || p.q == 2 || p.q == 4) && p.split >= 1 && p.split <= kMaxSplit && (plan >> 24) == 0,
               NRHIP_ERR_INVALID_ARG, "%s: plan 0x%x is not Q | split << 8 with Q in {1,2,4} and split in [1,%d]", who, plan,
               kMaxSplit);
  }
  const int64_t tiles = (m + kTile - 1) / kTile;
  p.tiles_per_split = (int)((tiles + p.split - 1) / p.split);
  if (p.tiles_per_split < 1) p.tiles_per_split = 1;
  return NRHIP_OK;
}

void launch_nearest(const Plan& p, const float* query, int stride_q, const uint8_t* query_valid, int64_t n,
                    const float* target, int stride_t, const uint8_t* target_valid, int64_t m, float* out,
                    hipStream_t st) {
  if (n == 0) return;
  const bool combine = p.split > 1;
  if (combine) nearest_init_kernel<<<grid_for(n, kBlock), kBlock, 0, st>>>(query_valid, (int)n, out);
  const dim3 grid((unsigned)((n + (int64_t)kBlock * p.q - 1) / ((int64_t)kBlock * p.q)), (unsigned)p.split);
#define NR_NEAREST(QQ)                                                                                                   \
  nearest_kernel<QQ><<<grid, kBlock, 0, st>>>(query, stride_q, query_valid, (int)n, target, stride_t, target_valid, (int)m, \
                                              p.tiles_per_split, combine, out)
  if (p.q == 4) NR_NEAREST(4);
  else if (p.q == 2) NR_NEAREST(2);
  else NR_NEAREST(1);
#undef NR_NEAREST
}

struct ChamferScratch {
  int64_t nb_s, nb_t, off_psum, off_pcnt, off_s, off_t, bytes;
};
ChamferScratch chamfer_layout(int64_t n, int64_t m) {
  ChamferScratch c;
  c.nb_s = (n + kSumItems - 1) / kSumItems, c.nb_t = (m + kSumItems - 1) / kSumItems;
  int64_t o = 0;
  c.off_psum = o, o += (c.nb_s + c.nb_t) * 8;  // double [nb_s + nb_t]
  c.off_pcnt = o, o += (c.nb_s + c.nb_t) * 8;  // int64  [nb_s + nb_t]
  c.off_s = o, o += (n + 3) / 4 * 16;          // float  [n]: per-point values where the caller keeps none
  c.off_t = o, o += (m + 3) / 4 * 16;          // float  [m]
  c.bytes = o;
  return c;
}

}  // namespace
}  // namespace nrhip

using namespace nrhip;

extern "C" int nrhip_nearest_sq_dist(const float* query, int32_t stride_q, const uint8_t* query_valid, int64_t n,
                                     const float* target, int32_t stride_t, const uint8_t* target_valid, int64_t m,
                                     int32_t plan, float* out, void* stream) {
  if (int rc = validate_points("nearest_sq_dist: query", query, stride_q, n)) return rc;
  if (int rc = validate_points("nearest_sq_dist: target", target, stride_t, m)) return rc;
  NR_REQUIRE(out || n == 0, NRHIP_ERR_INVALID_ARG, "nearest_sq_dist: out is NULL");
  Plan p;
  if (int rc = resolve_plan("nearest_sq_dist", plan, n, m, p)) return rc;
  if (n == 0) return NRHIP_OK;
  launch_nearest(p, query, stride_q, query_valid, n, target, stride_t, target_valid, m, out, (hipStream_t)stream);
  return check_launch("nearest_sq_dist");
}

extern "C" int nrhip_nearest_plan(int64_t n, int64_t m, int32_t* q, int32_t* split) {
  NR_REQUIRE(q && split, NRHIP_ERR_INVALID_ARG, "nearest_plan: NULL out-pointer");
  NR_REQUIRE(n >= 0 && m >= 0, NRHIP_ERR_INVALID_ARG, "nearest_plan: negative count");
  const Plan p = auto_plan(n, m);
  *q = p.q, *split = p.split;
  return NRHIP_OK;
}

extern "C" int nrhip_chamfer_workspace(int64_t n, int64_t m, int64_t* bytes) {
  NR_REQUIRE(bytes, NRHIP_ERR_INVALID_ARG, "chamfer_workspace: bytes is NULL");
  NR_REQUIRE(n >= 0 && m >= 0, NRHIP_ERR_INVALID_ARG, "chamfer_workspace: negative count");
  NR_REQUIRE(n < (INT64_C(1) << 31) && m < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "chamfer_workspace: count >= 2^31");
  *bytes = chamfer_layout(n, m).bytes;
  return NRHIP_OK;
}

extern "C" int nrhip_chamfer_distance(const float* source, int32_t stride_s, const uint8_t* source_valid, int64_t n,
                                      const float* target, int32_t stride_t, const uint8_t* target_valid, int64_t m,
                                      int32_t normalize_with_target, int32_t plan, float* result, float* source_sq_dist,
                                      float* target_sq_dist, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = validate_points("chamfer_distance: source", source, stride_s, n)) return rc;
  if (int rc = validate_points("chamfer_distance: target", target, stride_t, m)) return rc;
  NR_REQUIRE(result, NRHIP_ERR_INVALID_ARG, "chamfer_distance: result is NULL");
  const ChamferScratch c = chamfer_layout(n, m);
  NR_REQUIRE(c.bytes == 0 || (workspace && workspace_bytes >= c.bytes), NRHIP_ERR_INVALID_ARG,
             "chamfer_distance: workspace is NULL or smaller than nrhip_chamfer_workspace asks for (%lld < %lld)",
             (long long)workspace_bytes, (long long)c.bytes);
  NR_REQUIRE(c.bytes == 0 || ((uintptr_t)workspace & 15) == 0, NRHIP_ERR_INVALID_ARG,
             "chamfer_distance: workspace is not 16-byte aligned");
  Plan ps, pt;
  if (int rc = resolve_plan("chamfer_distance", plan, n, m, ps)) return rc;
  if (int rc = resolve_plan("chamfer_distance", plan, m, n, pt)) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* ds = source_sq_dist ? source_sq_dist : (float*)(ws + c.off_s);
  float* dt = target_sq_dist ? target_sq_dist : (float*)(ws + c.off_t);
  launch_nearest(ps, source, stride_s, source_valid, n, target, stride_t, target_valid, m, ds, st);
  launch_nearest(pt, target, stride_t, target_valid, m, source, stride_s, source_valid, n, dt, st);
  double* psum = (double*)(ws + c.off_psum);
  long long* pcnt = (long long*)(ws + c.off_pcnt);
  if (c.nb_s + c.nb_t > 0)
    sum_kernel<<<(unsigned)(c.nb_s + c.nb_t), kBlock, 0, st>>>(ds, source_valid, (int)n, (int)c.nb_s, dt, target_valid, (int)m,
                                                               psum, pcnt);
  final_kernel<<<1, kBlock, 0, st>>>(psum, pcnt, (int)c.nb_s, (int)c.nb_t, normalize_with_target ? 1 : 0, result);
  return check_launch("chamfer_distance");
}
