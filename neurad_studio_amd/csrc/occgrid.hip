// S6: occupancy-grid ray march with wavefront ballot / prefix-popcount compaction.
// (VolumetricSampler.forward -> nerfacc OccGridEstimator.sampling, model_components/ray_samplers.py:483-566.)
// nerfacc is un-vendored and nothing in neurad-studio instantiates VolumetricSampler, so the marching rule is stated
// here (and restated in oracle/neurad_oracle.py:occgrid_march) -- parity unpinned, see DESIGN.md:
//   * the ray is clipped to [max(near_plane, t_min), min(far_plane, t_max)] and to the grid's AABB;
//   * candidate intervals tile that range back to back: dt = max(t * cone_angle, step)  (uniform when cone_angle = 0);
//     a ray has at most max_candidates of them, k = 0 .. max_candidates - 1, counted before the occupancy test;
//   * a candidate is kept iff the cell containing its midpoint is occupied; kept intervals are emitted in order as
//     packed (ray_index, t_start, t_end).
// Multi-level grids (nrhip_occgrid_march_levels; the state and its update rule: occgrid_update.h): the ray is clipped to the
// outermost box; a candidate's level is the first l whose (closed) box contains its midpoint -- the outermost level when
// rounding puts it outside all of them -- and it is kept iff binaries[l] is set at the cell the same floor-and-clamp rule
// gives in that level; step sizes do not depend on the level.  One level: exactly the single-grid march.
// Dynamic actors (nrhip_occgrid_march_levels_actors): the grid is a time-independent world-space grid built from static
// densities, so the cells inside an actor's box at a ray's time are empty to it.  The box-aware march generates the same
// candidates and keeps one iff its cell is set (the test above, unchanged) OR its sample position -- sample_gaussian's mean,
// t0 + (t1 - t0) / 2, the position the field evaluates -- lies strictly inside the box of one of the ray's candidate
// actors (box_contains, common.h: the function find_hit calls).  March and field agree on every sample bit for bit.
// One wavefront marches one ray 64 candidates at a time: ballot(occupied) -> popcount prefix -> compacted store.
#include "common.h"
#include "occgrid_update.h"
#include "packed_composite.h"

namespace nrhip {

using OccDev = occ::LevelsDev;

struct March {
  float t0, t_far, step, c, t1;
  int k1;  // number of uniform steps before the cone takes over
  __device__ __forceinline__ float at(int k) const {
    if (c <= 0.f || k < k1) return t0 + (float)k * step;
    return t1 * powf(1.f + c, (float)(k - k1));
  }
};

__device__ __forceinline__ bool setup_march(const OccDev& g, const float* o, const float* d, float near, float far,
                                            float step, float cone, March& m) {
  float tn = near, tf = far;
  const float* lo = g.lo[g.L - 1];
  const float* hi = g.hi[g.L - 1];
#pragma unroll
  for (int a = 0; a < 3; ++a) {  // slab test against the (outermost) grid AABB
    const float inv = 1.f / d[a];
    float ta = (lo[a] - o[a]) * inv, tb = (hi[a] - o[a]) * inv;
    if (d[a] == 0.f) {
      if (o[a] < lo[a] || o[a] > hi[a]) return false;
      continue;
    }
    if (ta > tb) { const float s = ta; ta = tb; tb = s; }
    tn = fmaxf(tn, ta), tf = fminf(tf, tb);
  }
  if (!(tn < tf)) return false;
  m.t0 = tn, m.t_far = tf, m.step = step, m.c = cone, m.k1 = 0, m.t1 = tn;
  if (cone > 0.f && tn * cone < step) {
    m.k1 = (int)ceilf((step / cone - tn) / step);
    m.t1 = tn + (float)m.k1 * step;
  }
  return true;
}

__device__ __forceinline__ bool occupied(const OccDev& g, const float* o, const float* d, float tm) {
  const float p[3] = {o[0] + d[0] * tm, o[1] + d[1] * tm, o[2] + d[2] * tm};
  int lvl = g.L - 1;
  for (int l = g.L - 2; l >= 0; --l) {  // boxes are nested: the last hit going inwards is the first level containing p
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) in = in && p[a] >= g.lo[l][a] && p[a] <= g.hi[l][a];
    lvl = in ? l : lvl;
  }
  int idx = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float u = (p[a] - g.lo[lvl][a]) / (g.hi[lvl][a] - g.lo[lvl][a]);
    const int i = min(max((int)floorf(u * (float)g.res), 0), g.res - 1);
    idx = idx * g.res + i;
  }
  return g.bin[(int64_t)lvl * g.res * g.res * g.res + idx] != 0;
}

// The candidate boxes of the box-aware march (nrhip_occgrid_march_levels_actors): the per-ray lists of nrhip_actor_prepare
// and the actors' half sizes.  All NULL / 0 in the plain march.
struct MarchBoxes {
  const int32_t* cand_count;  // [R]
  const int32_t* cand_actor;  // [R, K]
  const float* cand_w2b;      // [R, K, 12]
  const float* bounds;        // [A, 3]
  int K, A;
};

// Is the sample [ts, te] of the ray inside the box of one of its first n candidates?  The field's own position and test:
// sample_gaussian's mean (the pixel area only enters the std, which nothing here reads) and box_contains, which find_hit
// calls too.  n <= K and the actor index is clamped into [0, A): every read stays inside the lists.
__device__ __forceinline__ bool in_candidate_box(const MarchBoxes& b, int64_t ray, int n, const float* o, const float* d,
                                                 float ts, float te) {
  const SamplePos g = sample_gaussian(o[0], o[1], o[2], d[0], d[1], d[2], 0.f, ts, te);
  bool in = false;
  for (int c = 0; c < n; ++c) {
    const int64_t e = ray * b.K + c;
    const int act = min(max(b.cand_actor[e], 0), b.A - 1);
    float bx, by, bz;
    in = box_contains(b.cand_w2b + e * 12, b.bounds + 3 * act, g.x, g.y, g.z, bx, by, bz) || in;
  }
  return in;
}

// One wavefront marches one ray.  WRITE=false: counts[ray] ; WRITE=true: packed outputs at offsets[ray].  BOXES: a candidate
// interval whose cell is empty is still kept when its sample lies inside a candidate actor's box.
template <bool WRITE, bool BOXES>
__device__ __forceinline__ void march_ray(const OccDev& g, const MarchBoxes& mb, const float* __restrict__ origins,
                                          const float* __restrict__ dirs, const float* __restrict__ t_min,
                                          const float* __restrict__ t_max, const float* __restrict__ t_rand, int64_t R,
                                          float step, float near_plane, float far_plane, float cone, int max_candidates,
                                          int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                          int64_t* __restrict__ ray_indices, float* __restrict__ t_starts,
                                          float* __restrict__ t_ends) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= R) return;
  const float o[3] = {origins[3 * ray], origins[3 * ray + 1], origins[3 * ray + 2]};
  const float d[3] = {dirs[3 * ray], dirs[3 * ray + 1], dirs[3 * ray + 2]};
  float near = fmaxf(near_plane, t_min ? t_min[ray] : near_plane);
  const float far = fminf(far_plane, t_max ? t_max[ray] : far_plane);
  if (t_rand) near += t_rand[ray] * step;  // stratified=True (nerfacc shifts the near plane by U(0,1)*step)
  int nbox = 0;
  if constexpr (BOXES) nbox = min(max(mb.cand_count[ray], 0), mb.K);
  March m;
  int total = 0;
  if (setup_march(g, o, d, near, far, step, cone, m)) {
    for (int k0 = 0; k0 < max_candidates; k0 += 64) {
      const int k = k0 + lane;
      const float ts = m.at(k);
      const float te = fminf(m.at(k + 1), m.t_far);
      const bool in_range = k < max_candidates && ts < m.t_far && te > ts;  // (the ballot below then ends the loop too)
      bool keep = in_range && occupied(g, o, d, 0.5f * (ts + te));
      if constexpr (BOXES) keep = keep || (in_range && nbox > 0 && in_candidate_box(mb, ray, nbox, o, d, ts, te));
      const unsigned long long mk = __ballot(keep);
      if (WRITE && keep) {
        const int64_t pos = offsets[ray] + total + __popcll(mk & ((1ull << lane) - 1ull));
        ray_indices[pos] = ray;
        t_starts[pos] = ts;
        t_ends[pos] = te;
      }
      total += __popcll(mk);
      if (__ballot(in_range) != ~0ull) break;  // ran past t_far: done (early termination of the wave)
    }
  }
  if (!WRITE && lane == 0) counts[ray] = total;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void occgrid_march_kernel(OccDev g, const float* __restrict__ origins,
                                                            const float* __restrict__ dirs,
                                                            const float* __restrict__ t_min,
                                                            const float* __restrict__ t_max,
                                                            const float* __restrict__ t_rand, int64_t R, float step,
                                                            float near_plane, float far_plane, float cone,
                                                            int max_candidates, int32_t* __restrict__ counts,
                                                            const int64_t* __restrict__ offsets,
                                                            int64_t* __restrict__ ray_indices,
                                                            float* __restrict__ t_starts, float* __restrict__ t_ends) {
  march_ray<WRITE, false>(g, MarchBoxes{}, origins, dirs, t_min, t_max, t_rand, R, step, near_plane, far_plane, cone,
                          max_candidates, counts, offsets, ray_indices, t_starts, t_ends);
}

template <bool WRITE>
__global__ __launch_bounds__(256) void occgrid_march_actors_kernel(OccDev g, MarchBoxes mb, const float* __restrict__ origins,
                                                                   const float* __restrict__ dirs,
                                                                   const float* __restrict__ t_min,
                                                                   const float* __restrict__ t_max,
                                                                   const float* __restrict__ t_rand, int64_t R, float step,
                                                                   float near_plane, float far_plane, float cone,
                                                                   int max_candidates, int32_t* __restrict__ counts,
                                                                   const int64_t* __restrict__ offsets,
                                                                   int64_t* __restrict__ ray_indices,
                                                                   float* __restrict__ t_starts, float* __restrict__ t_ends) {
  march_ray<WRITE, true>(g, mb, origins, dirs, t_min, t_max, t_rand, R, step, near_plane, far_plane, cone, max_candidates,
                         counts, offsets, ray_indices, t_starts, t_ends);
}

static int to_dev(const nrhip_occgrid* g, OccDev& d) {
  NR_REQUIRE(g && g->binaries && g->resolution >= 1 && g->resolution <= 1024, NRHIP_ERR_INVALID_ARG,
             "occgrid: NULL grid or resolution outside [1,1024]");
  d = OccDev{};
  for (int a = 0; a < 3; ++a) {
    d.lo[0][a] = g->aabb[a], d.hi[0][a] = g->aabb[3 + a];
    NR_REQUIRE(d.hi[0][a] > d.lo[0][a], NRHIP_ERR_INVALID_ARG, "occgrid: empty AABB");
  }
  d.L = 1, d.res = g->resolution, d.bin = const_cast<uint8_t*>(g->binaries);
  return NRHIP_OK;
}

static int to_dev(const nrhip_occgrid_levels* g, OccDev& d) {
  NR_REQUIRE(g && g->binaries, NRHIP_ERR_INVALID_ARG, "occgrid: NULL grid or NULL binaries");
  NR_REQUIRE(g->levels >= 1 && g->levels <= NRHIP_OCCGRID_MAX_LEVELS, NRHIP_ERR_INVALID_ARG,
             "occgrid: %d levels outside [1,%d]", g->levels, NRHIP_OCCGRID_MAX_LEVELS);
  NR_REQUIRE(g->resolution >= 1 && g->resolution <= 1024, NRHIP_ERR_INVALID_ARG, "occgrid: resolution outside [1,1024]");
  d = OccDev{};
  for (int l = 0; l < g->levels; ++l)
    for (int a = 0; a < 3; ++a) {
      d.lo[l][a] = g->aabbs[l][a], d.hi[l][a] = g->aabbs[l][3 + a];
      NR_REQUIRE(d.hi[l][a] > d.lo[l][a], NRHIP_ERR_INVALID_ARG, "occgrid: empty AABB at level %d", l);
      NR_REQUIRE(l == 0 || (d.lo[l][a] <= d.lo[l - 1][a] && d.hi[l][a] >= d.hi[l - 1][a]), NRHIP_ERR_INVALID_ARG,
                 "occgrid: the box of level %d does not contain that of level %d", l, l - 1);
    }
  d.L = g->levels, d.res = g->resolution, d.bin = g->binaries;
  return NRHIP_OK;
}

static int march(const OccDev& d, const float* origins, const float* directions, const float* t_min, const float* t_max,
                 const float* t_rand, int64_t r, float render_step_size, float near_plane, float far_plane,
                 float cone_angle, int32_t max_candidates, int32_t* counts, const int64_t* offsets, int64_t* ray_indices,
                 float* t_starts, float* t_ends, void* stream, const MarchBoxes* boxes = nullptr) {
  NR_REQUIRE(r >= 0 && render_step_size > 0.f && cone_angle >= 0.f && max_candidates >= 1, NRHIP_ERR_INVALID_ARG,
             "occgrid_march: bad argument");
  if (r == 0) return NRHIP_OK;
  NR_REQUIRE(origins && directions, NRHIP_ERR_INVALID_ARG, "occgrid_march: null rays");
  const int blocks = (int)((r + 3) / 4);
  const hipStream_t st = (hipStream_t)stream;
  if (!offsets) {
    NR_REQUIRE(counts, NRHIP_ERR_INVALID_ARG, "occgrid_march: counting pass needs `counts`");
    if (boxes)
      occgrid_march_actors_kernel<false><<<blocks, 256, 0, st>>>(d, *boxes, origins, directions, t_min, t_max, t_rand, r,
                                                                 render_step_size, near_plane, far_plane, cone_angle,
                                                                 max_candidates, counts, nullptr, nullptr, nullptr, nullptr);
    else
      occgrid_march_kernel<false><<<blocks, 256, 0, st>>>(d, origins, directions, t_min, t_max, t_rand, r,
                                                          render_step_size, near_plane, far_plane, cone_angle,
                                                          max_candidates, counts, nullptr, nullptr, nullptr, nullptr);
  } else {
    NR_REQUIRE(ray_indices && t_starts && t_ends, NRHIP_ERR_INVALID_ARG, "occgrid_march: write pass needs outputs");
    if (boxes)
      occgrid_march_actors_kernel<true><<<blocks, 256, 0, st>>>(d, *boxes, origins, directions, t_min, t_max, t_rand, r,
                                                                render_step_size, near_plane, far_plane, cone_angle,
                                                                max_candidates, nullptr, offsets, ray_indices, t_starts,
                                                                t_ends);
    else
      occgrid_march_kernel<true><<<blocks, 256, 0, st>>>(d, origins, directions, t_min, t_max, t_rand, r,
                                                         render_step_size, near_plane, far_plane, cone_angle,
                                                         max_candidates, nullptr, offsets, ray_indices, t_starts,
                                                         t_ends);
  }
  return check_launch("occgrid_march");
}

}  // namespace nrhip

using namespace nrhip;

extern "C" int nrhip_occgrid_march(const nrhip_occgrid* grid, const float* origins, const float* directions,
                                   const float* t_min, const float* t_max, const float* t_rand, int64_t r,
                                   float render_step_size, float near_plane, float far_plane, float cone_angle,
                                   int32_t max_candidates, int32_t* counts, const int64_t* offsets,
                                   int64_t* ray_indices, float* t_starts, float* t_ends, void* stream) {
  OccDev d;
  if (int e = to_dev(grid, d)) return e;
  return march(d, origins, directions, t_min, t_max, t_rand, r, render_step_size, near_plane, far_plane, cone_angle,
               max_candidates, counts, offsets, ray_indices, t_starts, t_ends, stream);
}

extern "C" int nrhip_occgrid_march_levels(const nrhip_occgrid_levels* grid, const float* origins, const float* directions,
                                          const float* t_min, const float* t_max, const float* t_rand, int64_t r,
                                          float render_step_size, float near_plane, float far_plane, float cone_angle,
                                          int32_t max_candidates, int32_t* counts, const int64_t* offsets,
                                          int64_t* ray_indices, float* t_starts, float* t_ends, void* stream) {
  OccDev d;
  if (int e = to_dev(grid, d)) return e;
  return march(d, origins, directions, t_min, t_max, t_rand, r, render_step_size, near_plane, far_plane, cone_angle,
               max_candidates, counts, offsets, ray_indices, t_starts, t_ends, stream);
}

// The box-aware march: nrhip_occgrid_march_levels, and a candidate interval whose cell is empty is kept all the same when its
// sample position lies inside the box of one of the ray's candidate actors (the lists of nrhip_actor_prepare at the ray's
// time).  With every cand_count zero the outputs are those of nrhip_occgrid_march_levels bit for bit.
extern "C" int nrhip_occgrid_march_levels_actors(const nrhip_occgrid_levels* grid, const nrhip_actors* actors,
                                                 const int32_t* cand_count, const int32_t* cand_actor,
                                                 const float* cand_w2b, const float* origins, const float* directions,
                                                 const float* t_min, const float* t_max, const float* t_rand, int64_t r,
                                                 float render_step_size, float near_plane, float far_plane,
                                                 float cone_angle, int32_t max_candidates, int32_t* counts,
                                                 const int64_t* offsets, int64_t* ray_indices, float* t_starts,
                                                 float* t_ends, void* stream) {
  OccDev d;
  if (int e = to_dev(grid, d)) return e;
  NR_REQUIRE(actors && actors->n_actors >= 1 && actors->bounds, NRHIP_ERR_INVALID_ARG,
             "occgrid_march_levels_actors: NULL actors descriptor, no actor or NULL bounds");
  NR_REQUIRE(r == 0 || (cand_count && cand_actor && cand_w2b), NRHIP_ERR_INVALID_ARG,
             "occgrid_march_levels_actors: NULL candidate list");
  const MarchBoxes mb{cand_count, cand_actor, cand_w2b, actors->bounds,
                      actors->max_candidates > 0 ? actors->max_candidates : NRHIP_DEFAULT_ACTOR_CANDIDATES, actors->n_actors};
  return march(d, origins, directions, t_min, t_max, t_rand, r, render_step_size, near_plane, far_plane, cone_angle,
               max_candidates, counts, offsets, ray_indices, t_starts, t_ends, stream, &mb);
}

// ---- grid maintenance (occgrid_update.h) ---------------------------------------------------------------------------------
extern "C" int nrhip_occgrid_update_workspace(int32_t levels, int32_t resolution, int64_t* bytes) {
  NR_REQUIRE(bytes, NRHIP_ERR_INVALID_ARG, "occgrid_update_workspace: bytes is NULL");
  NR_REQUIRE(levels >= 1 && levels <= NRHIP_OCCGRID_MAX_LEVELS && resolution >= 1 && resolution <= 1024,
             NRHIP_ERR_INVALID_ARG, "occgrid_update_workspace: levels outside [1,%d] or resolution outside [1,1024]",
             NRHIP_OCCGRID_MAX_LEVELS);
  *bytes = occ::scratch_layout(levels, resolution).bytes;
  return NRHIP_OK;
}

#define OCC_WS(NAME)                                                                                              \
  const occ::Scratch ws = occ::scratch_layout(d.L, d.res);                                                        \
  NR_REQUIRE(workspace && workspace_bytes >= ws.bytes, NRHIP_ERR_INVALID_ARG,                                    \
             NAME ": workspace is NULL or smaller than nrhip_occgrid_update_workspace asks for (%lld < %lld)",    \
             (long long)workspace_bytes, (long long)ws.bytes);                                                    \
  char* const wsp = (char*)workspace

extern "C" int nrhip_occgrid_update_candidates(const nrhip_occgrid_levels* grid, const float* occs, int32_t warmup,
                                               int32_t n, const int64_t* cell_draws, const float* sel_draws,
                                               const float* jitter, int32_t* cell_ids, int32_t* counts, float* positions,
                                               void* workspace, int64_t workspace_bytes, void* stream) {
  OccDev d;
  if (int e = to_dev(grid, d)) return e;
  const int64_t n_cells = (int64_t)d.res * d.res * d.res;
  NR_REQUIRE(n >= 0 && n <= n_cells, NRHIP_ERR_INVALID_ARG, "occgrid_update_candidates: n = %d outside [0, res^3]", n);
  const int64_t cap = warmup ? n_cells : 2 * (int64_t)n;
  if (cap == 0) return NRHIP_OK;  // nothing to do: no pointer is read, the workspace included
  OCC_WS("occgrid_update_candidates");
  NR_REQUIRE(occs && jitter && cell_ids && counts && positions, NRHIP_ERR_INVALID_ARG,
             "occgrid_update_candidates: NULL occs, jitter or output");
  NR_REQUIRE(warmup || (cell_draws && sel_draws), NRHIP_ERR_INVALID_ARG,
             "occgrid_update_candidates: the draws are NULL after warm-up");
  const hipStream_t st = (hipStream_t)stream;
  occ::CompactArgs a{};
  const int parts = warmup ? 1 : 2;
  a.mode[0] = warmup ? occ::kVisibleCells : occ::kVisibleDraws, a.mode[1] = occ::kOccupiedCells;
  a.n_src[0] = warmup ? ws.cells : n, a.n_src[1] = ws.cells;
  a.dst[0] = cell_ids, a.dst_stride[0] = cap;
  a.dst[1] = (int32_t*)(wsp + ws.off_list), a.dst_stride[1] = ws.cells;
  a.block_counts = (int32_t*)(wsp + ws.off_bcnt), a.totals = (int32_t*)(wsp + ws.off_tot);
  a.occs = occs, a.bin = d.bin, a.draws = cell_draws, a.cells = ws.cells, a.n = n, a.n_blk = (int)ws.n_blk, a.L = d.L;
  const dim3 cg((unsigned)ws.n_blk, d.L, parts);
  occ::compact_kernel<false><<<cg, 256, 0, st>>>(a);
  occ::compact_scan_kernel<<<dim3(d.L, parts), 256, 0, st>>>(a.block_counts, a.totals, a.n_blk, d.L);
  occ::compact_kernel<true><<<cg, 256, 0, st>>>(a);
  occ::candidates_finalize_kernel<<<dim3((unsigned)grid_for(cap, 256), d.L), 256, 0, st>>>(
      d, warmup, n, cap, a.totals, a.dst[1], ws.cells, sel_draws, jitter, cell_ids, counts, positions);
  return check_launch("occgrid_update_candidates");
}

extern "C" int nrhip_occgrid_update_apply(const nrhip_occgrid_levels* grid, float* occs, int64_t capacity,
                                          const int32_t* cell_ids, const int32_t* counts, const float* occ_values,
                                          float ema_decay, float occ_thre, void* workspace, int64_t workspace_bytes,
                                          void* stream) {
  OccDev d;
  if (int e = to_dev(grid, d)) return e;
  OCC_WS("occgrid_update_apply");
  NR_REQUIRE(capacity >= 0 && capacity <= ws.cells, NRHIP_ERR_INVALID_ARG,
             "occgrid_update_apply: capacity %lld outside [0, res^3]", (long long)capacity);
  NR_REQUIRE(occs, NRHIP_ERR_INVALID_ARG, "occgrid_update_apply: occs is NULL");
  NR_REQUIRE(capacity == 0 || (cell_ids && counts && occ_values), NRHIP_ERR_INVALID_ARG,
             "occgrid_update_apply: NULL candidates or values");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)d.L * ws.cells;
  uint32_t* keys = (uint32_t*)(wsp + ws.off_keys);
  double* psum = (double*)(wsp + ws.off_psum);
  long long* pcnt = (long long*)(wsp + ws.off_pcnt);
  float* thre = (float*)(wsp + ws.off_thre);
  if (capacity)
    occ::ema_max_kernel<<<dim3((unsigned)grid_for(capacity, 256), d.L), 256, 0, st>>>(capacity, ws.cells, cell_ids, counts,
                                                                                      occ_values, keys);
  occ::ema_apply_sum_kernel<<<(unsigned)ws.n_part, 256, 0, st>>>(total, ema_decay, occs, keys, psum, pcnt);
  occ::mean_final_kernel<<<1, 256, 0, st>>>(psum, pcnt, ws.n_part, occ_thre, thre);
  occ::threshold_kernel<<<(unsigned)grid_for(total, 256), 256, 0, st>>>(total, occs, thre, d.bin);
  return check_launch("occgrid_update_apply");
}

extern "C" int nrhip_occgrid_mark_invisible(const nrhip_occgrid_levels* grid, const float* K, int32_t n_k,
                                            const float* c2w, int32_t n_cams, int32_t width, int32_t height,
                                            float near_plane, float* occs, void* stream) {
  OccDev d;
  if (int e = to_dev(grid, d)) return e;
  NR_REQUIRE(n_cams >= 0 && (n_k == 1 || n_k == n_cams), NRHIP_ERR_INVALID_ARG,
             "occgrid_mark_invisible: %d intrinsics for %d cameras (one each, or one for all)", n_k, n_cams);
  NR_REQUIRE(width >= 1 && height >= 1, NRHIP_ERR_INVALID_ARG, "occgrid_mark_invisible: empty image");
  NR_REQUIRE(occs && (n_cams == 0 || (K && c2w)), NRHIP_ERR_INVALID_ARG, "occgrid_mark_invisible: NULL pointer");
  const int64_t cells = (int64_t)d.res * d.res * d.res;
  occ::mark_invisible_kernel<<<dim3((unsigned)grid_for(cells, 256), d.L), 256, 0, (hipStream_t)stream>>>(
      d, K, n_k == 1 ? 0 : 9, c2w, n_cams, (float)width, (float)height, near_plane, occs);
  return check_launch("occgrid_mark_invisible");
}

namespace nrhip {
// nerfacc render_visibility_from_alpha (packed): keep sample i of a ray iff T_i >= early_stop_eps and
// alpha_i >= alpha_thre, T_i = prod_{j<i}(1 - alpha_j) over the ray's packed segment [seg[r], seg[r+1]).
__global__ __launch_bounds__(256) void packed_visibility_kernel(const float* __restrict__ alphas,
                                                                const int64_t* __restrict__ seg, int64_t R,
                                                                float early_stop_eps, float alpha_thre,
                                                                uint8_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= R) return;
  const int64_t b = seg[ray], e = seg[ray + 1];
  float carry = 1.f;
  for (int64_t i0 = b; i0 < e; i0 += 64) {
    const int64_t i = i0 + lane;
    const float a = i < e ? alphas[i] : 0.f;
    float incl = 1.f - a;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float u = __shfl_up(incl, off, 64);
      if (lane >= off) incl *= u;
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 1.f;
    const float T = carry * excl;
    if (i < e) mask[i] = (T >= early_stop_eps && a >= alpha_thre) ? 1 : 0;
    carry *= __shfl(incl, 63, 64);
    if (carry < early_stop_eps) {  // everything behind is invisible: early ray termination
      for (int64_t k = i0 + 64 + lane; k < e; k += 64) mask[k] = 0;
      break;
    }
  }
}
}  // namespace nrhip

extern "C" int nrhip_packed_visibility_from_alpha(const float* alphas, const int64_t* segments, int64_t r,
                                                  float early_stop_eps, float alpha_thre, uint8_t* mask,
                                                  void* stream) {
  NR_REQUIRE(r >= 0, NRHIP_ERR_INVALID_ARG, "packed_visibility: negative r");
  if (r == 0) return NRHIP_OK;
  NR_REQUIRE(alphas && segments && mask, NRHIP_ERR_INVALID_ARG, "packed_visibility: null pointer");
  nrhip::packed_visibility_kernel<<<(int)((r + 3) / 4), 256, 0, (hipStream_t)stream>>>(alphas, segments, r,
                                                                                       early_stop_eps, alpha_thre, mask);
  return nrhip::check_launch("packed_visibility_from_alpha");
}

// ---- packed compositing (packed_composite.h): nerfacc's packed render_weight_from_* / accumulate_along_rays and their
// fusion.  Validation on the host; r == 0 is a no-op that reads no pointer; a batch whose segments are all empty launches
// (the per-ray outputs are zeroed) and touches no sample pointer.
#define PACKED_COMMON(NAME, r_, segments_, c_)                                                       \
  NR_REQUIRE((r_) >= 0, NRHIP_ERR_INVALID_ARG, NAME ": negative ray count");                          \
  NR_REQUIRE((c_) >= 1, NRHIP_ERR_INVALID_ARG, NAME ": channel count %d < 1", (int)(c_));             \
  if ((r_) == 0) return NRHIP_OK;                                                                    \
  NR_REQUIRE((segments_), NRHIP_ERR_INVALID_ARG, NAME ": segments is NULL")

#define PACKED_LAUNCH(KERNEL, r_, stream, ...) \
  nrhip::packed::KERNEL<<<nrhip::packed::blocks_for(r_), 64 * nrhip::packed::kWaves, 0, (hipStream_t)stream>>>(__VA_ARGS__)

extern "C" int nrhip_packed_segments(const int64_t* ray_indices, int64_t m, int64_t r, int64_t* segments, void* stream) {
  NR_REQUIRE(r >= 0 && m >= 0, NRHIP_ERR_INVALID_ARG, "packed_segments: negative ray or sample count");
  NR_REQUIRE(segments, NRHIP_ERR_INVALID_ARG, "packed_segments: segments is NULL");
  NR_REQUIRE(m == 0 || ray_indices, NRHIP_ERR_INVALID_ARG, "packed_segments: ray_indices is NULL");
  int blocks = grid_for(r + 1, 256);
  blocks = blocks > 4096 ? 4096 : blocks;
  nrhip::packed::segments_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(ray_indices, m, r, segments);
  return check_launch("packed_segments");
}

extern "C" int nrhip_packed_weight_from_density(const float* t_starts, const float* t_ends, const float* sigmas,
                                                const int64_t* segments, int64_t r, float* weights, float* trans,
                                                float* alphas, void* stream) {
  PACKED_COMMON("packed_weight_from_density", r, segments, 1);
  PACKED_LAUNCH(fwd_kernel<nrhip::packed::kDensity>, r, stream, t_starts, t_ends, sigmas, nullptr, segments, r, 1, 1, 0,
                nullptr, nullptr, nullptr, weights, trans, alphas);
  return check_launch("packed_weight_from_density");
}

extern "C" int nrhip_packed_weight_from_density_bwd(const float* t_starts, const float* t_ends, const float* sigmas,
                                                    const int64_t* segments, const float* grad_w, int64_t r,
                                                    float* grad_sigmas, void* stream) {
  PACKED_COMMON("packed_weight_from_density_bwd", r, segments, 1);
  PACKED_LAUNCH(bwd_kernel<nrhip::packed::kDensity>, r, stream, t_starts, t_ends, sigmas, nullptr, segments, nullptr,
                nullptr, nullptr, grad_w, nullptr, r, 1, 1, 0, grad_sigmas, nullptr);
  return check_launch("packed_weight_from_density_bwd");
}

extern "C" int nrhip_packed_weight_from_alpha(const float* alphas, const int64_t* segments, int64_t r, float* weights,
                                              float* trans, void* stream) {
  PACKED_COMMON("packed_weight_from_alpha", r, segments, 1);
  PACKED_LAUNCH(fwd_kernel<nrhip::packed::kAlpha>, r, stream, nullptr, nullptr, alphas, nullptr, segments, r, 1, 1, 0,
                nullptr, nullptr, nullptr, weights, trans, nullptr);
  return check_launch("packed_weight_from_alpha");
}

extern "C" int nrhip_packed_weight_from_alpha_bwd(const float* alphas, const int64_t* segments, const float* grad_w,
                                                  const float* grad_t, int64_t r, float* grad_alphas, void* stream) {
  PACKED_COMMON("packed_weight_from_alpha_bwd", r, segments, 1);
  PACKED_LAUNCH(bwd_kernel<nrhip::packed::kAlpha>, r, stream, nullptr, nullptr, alphas, nullptr, segments, nullptr, nullptr,
                nullptr, grad_w, grad_t, r, 1, 1, 0, grad_alphas, nullptr);
  return check_launch("packed_weight_from_alpha_bwd");
}

extern "C" int nrhip_packed_accumulate(const float* weights, const float* values, const int64_t* segments, int64_t r,
                                       int32_t c, float* out, void* stream) {
  PACKED_COMMON("packed_accumulate", r, segments, c);
  NR_REQUIRE(out, NRHIP_ERR_INVALID_ARG, "packed_accumulate: out is NULL");
  NR_REQUIRE(values || c == 1, NRHIP_ERR_INVALID_ARG, "packed_accumulate: values is NULL (a plain sum) but c = %d", c);
  const nrhip::packed::Plan p = nrhip::packed::plan_for(c, values, out, nullptr);
  if (values)
    PACKED_LAUNCH(fwd_kernel<nrhip::packed::kWeights>, r, stream, nullptr, nullptr, weights, values, segments, r, c, p.lp,
                  p.k, out, nullptr, nullptr, nullptr, nullptr, nullptr);
  else
    PACKED_LAUNCH(fwd_kernel<nrhip::packed::kWeights>, r, stream, nullptr, nullptr, weights, nullptr, segments, r, 1, 1, 0,
                  nullptr, nullptr, out, nullptr, nullptr, nullptr);
  return check_launch("packed_accumulate");
}

extern "C" int nrhip_packed_accumulate_bwd(const float* weights, const float* values, const float* g_out,
                                           const int64_t* segments, int64_t r, int32_t c, float* grad_weights,
                                           float* grad_values, void* stream) {
  PACKED_COMMON("packed_accumulate_bwd", r, segments, c);
  NR_REQUIRE(g_out, NRHIP_ERR_INVALID_ARG, "packed_accumulate_bwd: g_out is NULL");
  NR_REQUIRE(values || (c == 1 && !grad_values), NRHIP_ERR_INVALID_ARG,
             "packed_accumulate_bwd: values is NULL (a plain sum) but c != 1 or grad_values is asked for");
  if (!grad_weights && !grad_values) return NRHIP_OK;
  const nrhip::packed::Plan p = nrhip::packed::plan_for(c, values, g_out, grad_values);
  if (values)
    PACKED_LAUNCH(bwd_kernel<nrhip::packed::kWeights>, r, stream, nullptr, nullptr, weights, values, segments, g_out,
                  nullptr, nullptr, nullptr, nullptr, r, c, p.lp, p.k, grad_weights, grad_values);
  else
    PACKED_LAUNCH(bwd_kernel<nrhip::packed::kWeights>, r, stream, nullptr, nullptr, weights, nullptr, segments, nullptr,
                  nullptr, g_out, nullptr, nullptr, r, 1, 1, 0, grad_weights, nullptr);
  return check_launch("packed_accumulate_bwd");
}

extern "C" int nrhip_packed_composite_fwd(const float* t_starts, const float* t_ends, const float* sigmas_or_alphas,
                                          const float* features, const int64_t* segments, int64_t r, int32_t c,
                                          int32_t mode, float* out_features, float* out_depth, float* out_accumulation,
                                          float* out_weights, void* stream) {
  PACKED_COMMON("packed_composite_fwd", r, segments, c);
  NR_REQUIRE(mode == 0 || mode == 1, NRHIP_ERR_INVALID_ARG, "packed_composite_fwd: mode %d not 0 (alphas) or 1 (sigmas)",
             mode);
  NR_REQUIRE(out_features && out_depth && out_accumulation, NRHIP_ERR_INVALID_ARG,
             "packed_composite_fwd: a per-ray output is NULL");
  const nrhip::packed::Plan p = nrhip::packed::plan_for(c, features, out_features, nullptr);
  if (mode == 1)
    PACKED_LAUNCH(fwd_kernel<nrhip::packed::kDensity>, r, stream, t_starts, t_ends, sigmas_or_alphas, features, segments,
                  r, c, p.lp, p.k, out_features, out_depth, out_accumulation, out_weights, nullptr, nullptr);
  else
    PACKED_LAUNCH(fwd_kernel<nrhip::packed::kAlpha>, r, stream, t_starts, t_ends, sigmas_or_alphas, features, segments, r,
                  c, p.lp, p.k, out_features, out_depth, out_accumulation, out_weights, nullptr, nullptr);
  return check_launch("packed_composite_fwd");
}

extern "C" int nrhip_packed_composite_bwd(const float* t_starts, const float* t_ends, const float* sigmas_or_alphas,
                                          const float* features, const int64_t* segments, const float* g_features,
                                          const float* g_depth, const float* g_accumulation, const float* g_weights,
                                          int64_t r, int32_t c, int32_t mode, float* grad_sigmas_or_alphas,
                                          float* grad_features, void* stream) {
  PACKED_COMMON("packed_composite_bwd", r, segments, c);
  NR_REQUIRE(mode == 0 || mode == 1, NRHIP_ERR_INVALID_ARG, "packed_composite_bwd: mode %d not 0 (alphas) or 1 (sigmas)",
             mode);
  NR_REQUIRE(g_features, NRHIP_ERR_INVALID_ARG, "packed_composite_bwd: g_features is NULL");
  if (!grad_sigmas_or_alphas && !grad_features) return NRHIP_OK;
  const nrhip::packed::Plan p = nrhip::packed::plan_for(c, features, g_features, grad_features);
  if (mode == 1)
    PACKED_LAUNCH(bwd_kernel<nrhip::packed::kDensity>, r, stream, t_starts, t_ends, sigmas_or_alphas, features, segments,
                  g_features, g_depth, g_accumulation, g_weights, nullptr, r, c, p.lp, p.k, grad_sigmas_or_alphas,
                  grad_features);
  else
    PACKED_LAUNCH(bwd_kernel<nrhip::packed::kAlpha>, r, stream, t_starts, t_ends, sigmas_or_alphas, features, segments,
                  g_features, g_depth, g_accumulation, g_weights, nullptr, r, c, p.lp, p.k, grad_sigmas_or_alphas,
                  grad_features);
  return check_launch("packed_composite_bwd");
}

// ---- head + packed compositing for training (packed_composite.h: head_fwd_kernel / head_bwd_kernel): the packed sibling
// of nrhip_sdf_render_fwd / _bwd.  `beta` is a device pointer to the raw parameter (NULL: the density head).
extern "C" int nrhip_sdf_render_packed_fwd(const float* geo_out, const float* beta, float beta_min, const float* features,
                                           const float* t_starts, const float* t_ends, const int64_t* segments, int64_t r,
                                           int32_t c, float* alpha, float* weights, float* out_features, float* out_depth,
                                           float* out_accumulation, void* stream) {
  PACKED_COMMON("sdf_render_packed_fwd", r, segments, c);
  NR_REQUIRE(out_features && out_depth && out_accumulation, NRHIP_ERR_INVALID_ARG,
             "sdf_render_packed_fwd: a per-ray output is NULL");
  const nrhip::packed::Plan p = nrhip::packed::plan_for(c, features, out_features, nullptr);
  PACKED_LAUNCH(head_fwd_kernel, r, stream, t_starts, t_ends, geo_out, beta, beta_min, features, segments, r, c, p.lp, p.k,
                alpha, weights, out_features, out_depth, out_accumulation);
  return check_launch("sdf_render_packed_fwd");
}

extern "C" int nrhip_sdf_render_packed_bwd_workspace(int64_t r, int64_t* floats) {
  NR_REQUIRE(floats && r >= 0, NRHIP_ERR_INVALID_ARG, "sdf_render_packed_bwd_workspace: bad argument");
  *floats = (int64_t)nrhip::packed::blocks_for(r) * nrhip::packed::kWaves;  // one partial of d beta per wave
  return NRHIP_OK;
}

extern "C" int nrhip_sdf_render_packed_bwd(const float* geo_out, const float* beta, float beta_min, const float* alpha,
                                           const float* features, const float* t_starts, const float* t_ends,
                                           const int64_t* segments, const float* g_features, const float* g_depth,
                                           const float* g_accumulation, const float* g_weights, int64_t r, int32_t c,
                                           float* grad_features, float* grad_geo_out, float* grad_beta, float* workspace,
                                           void* stream) {
  NR_REQUIRE(r >= 0, NRHIP_ERR_INVALID_ARG, "sdf_render_packed_bwd: negative ray count");
  NR_REQUIRE(c >= 1, NRHIP_ERR_INVALID_ARG, "sdf_render_packed_bwd: channel count %d < 1", (int)c);
  NR_REQUIRE(grad_beta || !beta, NRHIP_ERR_INVALID_ARG, "sdf_render_packed_bwd: grad_beta is NULL");
  hipStream_t st = (hipStream_t)stream;
  if (r == 0) {
    if (grad_beta && hipMemsetAsync(grad_beta, 0, sizeof(float), st) != hipSuccess) return check_launch("sdf_render_packed_bwd");
    return NRHIP_OK;
  }
  NR_REQUIRE(segments, NRHIP_ERR_INVALID_ARG, "sdf_render_packed_bwd: segments is NULL");
  NR_REQUIRE(grad_features && grad_geo_out && workspace, NRHIP_ERR_INVALID_ARG,
             "sdf_render_packed_bwd: a gradient output or the workspace is NULL");
  const nrhip::packed::Plan p = nrhip::packed::plan_for(c, features, g_features, grad_features);
  // (g_features == NULL: no feature term upstream; grad_features = w gF is then left to the caller -- it is zero)
  PACKED_LAUNCH(head_bwd_kernel, r, stream, t_starts, t_ends, geo_out, beta, beta_min, alpha, g_features ? features : nullptr,
                segments, g_features, g_depth, g_accumulation, g_weights, r, c, p.lp, p.k, grad_geo_out, grad_features,
                workspace);
  if (beta)
    nrhip::packed::beta_reduce_kernel<<<1, 64, 0, st>>>(workspace, nrhip::packed::blocks_for(r) * nrhip::packed::kWaves, beta,
                                                        grad_beta);
  return check_launch("sdf_render_packed_bwd");
}
