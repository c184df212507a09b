// Occupancy-grid maintenance: the update rule, invisible-cell marking and the multi-level grid the march walks.
// Modelled on nerfacc 0.5 OccGridEstimator._update / mark_invisible_cells.  nerfacc is un-vendored (on no machine this
// was written on), so -- like the march (row S6) -- this is a STATED rule with a CPU restatement
// (tests/occgrid_update_restatement.py); parity with nerfacc itself is unpinned.
//
// Grid state.  aabbs [L,6]: level l is the level-0 box scaled by 2^l about its centre (the caller passes all L boxes).
//   occs fp32 [L*res^3], binaries uint8 [L,res,res,res], cell id c = (ix*res + iy)*res + iz.  Cells with occs < 0 are
//   INVISIBLE: never evaluated, never occupied.  A cell is OCCUPIED iff binaries != 0 and occs >= 0.
//
// Candidates (nrhip_occgrid_update_candidates), n draws per level:
//   warm-up       every visible cell of every level, ascending cell id                      capacity res^3 per level
//   afterwards    (a) the n uniform draws cell_draws[l, :], draws on invisible cells dropped, order kept,
//                 (b) the level's occupied cells in ascending order -- all of them when n_occ <= n, otherwise n draws with
//                     replacement, occupied[min(int(sel_draws[l, j] * n_occ), n_occ - 1)] in fp32        capacity 2 n per level
//   Each level has a device-side count; slots behind it hold cell id -1 and the centre of the level's box, and whatever is
//   evaluated for them is ignored.  Both lists come from an ORDERED compaction (per-block ballot/popcount counts ->
//   exclusive scan -> write), never from an atomic append: the selection must not depend on arrival order.
// Positions: x = (cell_xyz + jitter[l, slot]) / res, p = lo_l + x * (hi_l - lo_l), each step rounded to fp32.
//
// EMA (nrhip_occgrid_update_apply): m_c = max of the evaluated values over all candidates of cell c (unsigned-integer max
//   atomics on an order-preserving key of the float: independent of arrival order, negative values order correctly);
//   occs[c] = max(occs[c] * ema_decay, m_c), the decay applied ONCE per touched cell; untouched cells keep their bits.
//   Non-finite values: a candidate whose value is NaN is ignored as if it were absent (a cell with no other candidate is
//   untouched, not decayed); +-inf take part in the max like any number.  A NaN already in occs fails occs >= 0 and is
//   therefore treated as invisible: never evaluated, never written, not part of the mean.
// Threshold: mean = mean of occs over the visible cells of all levels, accumulated in float64 in a fixed order (per-block
//   partials in a slab, fixed-order final reduction), rounded to fp32 once; thre = min(mean, occ_thre);
//   binaries = occs > thre.  Without a visible cell every binary is cleared.  No float atomic sum anywhere.
//
// mark_invisible (nrhip_occgrid_mark_invisible): cell point x = lo_l + idx / (res - 1) * (hi_l - lo_l); OpenCV cameras:
//   cam = R^T (x - t), h = K cam, z = h[2], u = h[0] / z, v = h[1] / z (fp32, sums left to right).  The cell is in a
//   camera's image iff z >= 0, 0 <= u < width, 0 <= v < height.  Visible iff some camera has it in the image at
//   z >= near_plane and none has it in the image at z < near_plane.  Visible: occs = 0; invisible: occs = -1 and the
//   binary is cleared (never occupied).  One thread per cell, camera matrices wave-uniform.
//
// No kernel here allocates, reads back to the host or sizes anything by data: graph-capturable, bitwise reproducible.
#pragma once
#include "common.h"

namespace nrhip {
namespace occ {

constexpr int kMaxLevels = NRHIP_OCCGRID_MAX_LEVELS;
constexpr int kCompactItems = 1024;  // source elements per block of the ordered compaction: 4 rounds of 256 threads
constexpr int kSumItems = 2048;      // cells per block of the EMA-apply / visible-sum pass: 8 rounds of 256 threads

struct LevelsDev {
  int L, res;
  float lo[kMaxLevels][3], hi[kMaxLevels][3];
  uint8_t* bin;
};

// ---- scratch layout (bytes), one place for the size query and the kernels -----------------------------------------------
struct Scratch {
  int64_t cells, n_blk, n_part;
  int64_t off_psum, off_pcnt, off_thre, off_keys, off_list, off_bcnt, off_tot, bytes;
};
inline Scratch scratch_layout(int L, int res) {
  Scratch s;
  s.cells = (int64_t)res * res * res;
  s.n_blk = (s.cells + kCompactItems - 1) / kCompactItems;
  s.n_part = ((int64_t)L * s.cells + kSumItems - 1) / kSumItems;
  int64_t o = 0;
  s.off_psum = o, o += s.n_part * 8;            // double  [n_part]
  s.off_pcnt = o, o += s.n_part * 8;            // int64   [n_part]
  s.off_thre = o, o += 8;                       // float   threshold
  s.off_keys = o, o += (int64_t)L * s.cells * 4;  // uint32  [L*cells] max keys, all zero between calls
  s.off_list = o, o += (int64_t)L * s.cells * 4;  // int32   [L, cells] ordered occupied cells
  s.off_bcnt = o, o += 2 * L * s.n_blk * 4;     // int32   [2, L, n_blk] block counts -> exclusive offsets
  s.off_tot = o, o += 2 * L * 4;                // int32   [2, L] totals
  s.bytes = (o + 15) / 16 * 16;
  return s;
}

// order-preserving key of a float: a < b  <=>  key(a) < key(b) as unsigned; 0 is below every float's key except that of
// the NaN with all bits set, and marks "no candidate"
__device__ __forceinline__ uint32_t float_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- ordered compaction ------------------------------------------------------------------------------------------------
enum { kVisibleCells = 0, kOccupiedCells = 1, kVisibleDraws = 2 };
struct CompactArgs {
  int mode[2];         // per part
  int64_t n_src[2];    // source elements per level
  int64_t dst_stride[2];
  int32_t* dst[2];     // [L, dst_stride]
  int32_t* block_counts;  // [parts, L, n_blk]
  int32_t* totals;        // [parts, L]
  const float* occs;
  const uint8_t* bin;
  const int64_t* draws;  // [L, n]
  int64_t cells;
  int n, n_blk, L;
};

__device__ __forceinline__ bool compact_flag(const CompactArgs& a, int part, int l, int64_t i, int32_t& v) {
  if (i >= a.n_src[part]) return false;
  int64_t c = i;
  if (a.mode[part] == kVisibleDraws) {
    c = a.draws[(int64_t)l * a.n + i];
    if (c < 0 || c >= a.cells) return false;
  }
  v = (int32_t)c;
  const int64_t g = (int64_t)l * a.cells + c;
  const bool visible = a.occs[g] >= 0.f;
  return a.mode[part] == kOccupiedCells ? (visible && a.bin[g] != 0) : visible;
}

// WRITE=false: block_counts[part][l][block]; WRITE=true: the flagged values at their ranks (block_counts now holds offsets)
template <bool WRITE>
__global__ __launch_bounds__(256) void compact_kernel(CompactArgs a) {
  __shared__ int cnt[16];
  const int part = blockIdx.z, l = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * kCompactItems;
  if (base >= a.n_src[part]) {  // (uniform) nothing of this part in this block
    if (!WRITE && threadIdx.x == 0) a.block_counts[((int64_t)part * a.L + l) * a.n_blk + blockIdx.x] = 0;
    return;
  }
  bool f[4];
  int32_t v[4];
  unsigned long long mk[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    v[r] = 0;
    f[r] = compact_flag(a, part, l, base + r * 256 + threadIdx.x, v[r]);
    mk[r] = __ballot(f[r]);
    if (lane == 0) cnt[r * 4 + wave] = __popcll(mk[r]);
  }
  __syncthreads();
  if (!WRITE) {
    if (threadIdx.x == 0) {
      int t = 0;
      for (int k = 0; k < 16; ++k) t += cnt[k];
      a.block_counts[((int64_t)part * a.L + l) * a.n_blk + blockIdx.x] = t;
    }
    return;
  }
  int off = a.block_counts[((int64_t)part * a.L + l) * a.n_blk + blockIdx.x];
  int32_t* dst = a.dst[part] + (int64_t)l * a.dst_stride[part];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int before = 0;
    for (int w = 0; w < 4; ++w) {
      const int c = cnt[r * 4 + w];
      before += w < wave ? c : 0;
    }
    if (f[r]) dst[off + before + __popcll(mk[r] & ((1ull << lane) - 1ull))] = v[r];
    off += cnt[r * 4] + cnt[r * 4 + 1] + cnt[r * 4 + 2] + cnt[r * 4 + 3];
  }
}

// one block per (level, part): block_counts -> exclusive offsets in place, totals[part][l]
__global__ __launch_bounds__(256) void compact_scan_kernel(int32_t* __restrict__ block_counts, int32_t* __restrict__ totals,
                                                           int n_blk, int L) {
  __shared__ int part_sum[256];
  const int l = blockIdx.x, part = blockIdx.y, t = threadIdx.x;
  int32_t* c = block_counts + ((int64_t)part * L + l) * n_blk;
  const int per = (n_blk + 255) / 256, b = t * per, e = min(b + per, n_blk);
  int s = 0;
  for (int i = b; i < e; ++i) s += c[i];
  part_sum[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) {
      const int x = part_sum[i];
      part_sum[i] = run, run += x;
    }
    totals[part * L + l] = run;
  }
  __syncthreads();
  int run = part_sum[t];
  for (int i = b; i < e; ++i) {
    const int x = c[i];
    c[i] = run, run += x;
  }
}

// slot -> cell id (selection of the occupied part), per-level count, position
__global__ __launch_bounds__(256) void candidates_finalize_kernel(LevelsDev g, int warmup, int n, int64_t cap,
                                                                  const int32_t* __restrict__ totals,
                                                                  const int32_t* __restrict__ occ_list, int64_t cells,
                                                                  const float* __restrict__ sel_draws,
                                                                  const float* __restrict__ jitter,
                                                                  int32_t* __restrict__ cell_ids,
                                                                  int32_t* __restrict__ counts,
                                                                  float* __restrict__ positions) {
  const int l = blockIdx.y;
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= cap) return;
  const int na = totals[l];
  int cnt = na;
  int32_t cell = -1;
  int32_t* ids = cell_ids + (int64_t)l * cap;
  if (warmup) {
    if (s < na) cell = ids[s];
  } else {
    const int n_occ = totals[g.L + l], m = min(n_occ, n);
    cnt = na + m;
    if (s < na) {
      cell = ids[s];
    } else if (s - na < m) {
      const int j = (int)(s - na);
      const int k = n_occ <= n ? j : max(min((int)(sel_draws[(int64_t)l * n + j] * (float)n_occ), n_occ - 1), 0);
      cell = occ_list[(int64_t)l * cells + k];
    }
  }
  ids[s] = cell;
  if (s == 0) counts[l] = cnt;
  float* p = positions + ((int64_t)l * cap + s) * 3;
  if (cell < 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = (g.lo[l][a] + g.hi[l][a]) * 0.5f;
    return;
  }
  const int idx[3] = {cell / (g.res * g.res), (cell / g.res) % g.res, cell % g.res};
  const float* jit = jitter + ((int64_t)l * cap + s) * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = ((float)idx[a] + jit[a]) / (float)g.res;
    p[a] = g.lo[l][a] + x * (g.hi[l][a] - g.lo[l][a]);
  }
}

// ---- EMA and threshold -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ema_max_kernel(int64_t cap, int64_t cells, const int32_t* __restrict__ cell_ids,
                                                      const int32_t* __restrict__ counts,
                                                      const float* __restrict__ occ_values, uint32_t* __restrict__ keys) {
  const int l = blockIdx.y;
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= cap || s >= counts[l]) return;
  const int32_t c = cell_ids[(int64_t)l * cap + s];
  const float v = occ_values[(int64_t)l * cap + s];
  if (c < 0 || c >= cells || v != v) return;  // a NaN value counts as no candidate
  atomicMax(&keys[(int64_t)l * cells + c], float_key(v));
}

__device__ __forceinline__ void block_sum_fixed(double s, long long n, double* sh_s, long long* sh_n, double& out_s,
                                                long long& out_n) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_down(s, off, 64);
    n += __shfl_down(n, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh_s[wave] = s, sh_n[wave] = n;
  __syncthreads();
  out_s = ((sh_s[0] + sh_s[1]) + sh_s[2]) + sh_s[3];
  out_n = sh_n[0] + sh_n[1] + sh_n[2] + sh_n[3];
}

// touched cells: occs = max(occs * decay, m), key cleared; every block: float64 sum and count of its visible cells
__global__ __launch_bounds__(256) void ema_apply_sum_kernel(int64_t total, float decay, float* __restrict__ occs,
                                                            uint32_t* __restrict__ keys, double* __restrict__ psum,
                                                            long long* __restrict__ pcnt) {
  __shared__ double sh_s[4];
  __shared__ long long sh_n[4];
  const int64_t base = (int64_t)blockIdx.x * kSumItems;
  double s = 0.0;
  long long n = 0;
#pragma unroll
  for (int j = 0; j < kSumItems / 256; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i >= total) break;
    const uint32_t k = keys[i];
    float o = occs[i];
    if (k) {
      if (o >= 0.f) {
        o = fmaxf(o * decay, key_float(k));
        occs[i] = o;
      }
      keys[i] = 0u;
    }
    if (o >= 0.f) s += (double)o, ++n;
  }
  double bs;
  long long bn;
  block_sum_fixed(s, n, sh_s, sh_n, bs, bn);
  if (threadIdx.x == 0) psum[blockIdx.x] = bs, pcnt[blockIdx.x] = bn;
}

__global__ __launch_bounds__(256) void mean_final_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                         int64_t n_part, float occ_thre, float* __restrict__ thre) {
  __shared__ double sh_s[4];
  __shared__ long long sh_n[4];
  double s = 0.0;
  long long n = 0;
  for (int64_t i = threadIdx.x; i < n_part; i += 256) s += psum[i], n += pcnt[i];
  double bs;
  long long bn;
  block_sum_fixed(s, n, sh_s, sh_n, bs, bn);
  if (threadIdx.x == 0) *thre = bn > 0 ? fminf((float)(bs / (double)bn), occ_thre) : __uint_as_float(0x7f800000u);
}

__global__ __launch_bounds__(256) void threshold_kernel(int64_t total, const float* __restrict__ occs,
                                                        const float* __restrict__ thre, uint8_t* __restrict__ bin) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) bin[i] = occs[i] > *thre ? 1 : 0;
}

// ---- invisible cells ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mark_invisible_kernel(LevelsDev g, const float* __restrict__ K, int k_stride,
                                                             const float* __restrict__ c2w, int n_cams, float width,
                                                             float height, float near_plane, float* __restrict__ occs) {
  const int l = blockIdx.y;
  const int64_t cells = (int64_t)g.res * g.res * g.res;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const int idx[3] = {(int)(c / ((int64_t)g.res * g.res)), (int)((c / g.res) % g.res), (int)(c % g.res)};
  const float denom = (float)max(g.res - 1, 1);
  float x[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) x[a] = g.lo[l][a] + ((float)idx[a] / denom) * (g.hi[l][a] - g.lo[l][a]);
  bool seen = false, too_near = false;
  for (int n = 0; n < n_cams; ++n) {  // (uniform index: the matrices come through scalar loads)
    const float* M = c2w + (int64_t)n * 12;
    const float* Kn = K + (int64_t)n * k_stride;
    const float d0 = x[0] - M[3], d1 = x[1] - M[7], d2 = x[2] - M[11];
    float cam[3], h[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) cam[i] = (M[i] * d0 + M[4 + i] * d1) + M[8 + i] * d2;
#pragma unroll
    for (int i = 0; i < 3; ++i) h[i] = (Kn[3 * i] * cam[0] + Kn[3 * i + 1] * cam[1]) + Kn[3 * i + 2] * cam[2];
    const float z = h[2], u = h[0] / z, v = h[1] / z;
    const bool in_image = z >= 0.f && u >= 0.f && u < width && v >= 0.f && v < height;
    seen |= in_image && z >= near_plane;
    too_near |= in_image && z < near_plane;
  }
  const bool visible = seen && !too_near;
  const int64_t gi = (int64_t)l * cells + c;
  occs[gi] = visible ? 0.f : -1.f;
  if (!visible) g.bin[gi] = 0;
}

}  // namespace occ
}  // namespace nrhip
