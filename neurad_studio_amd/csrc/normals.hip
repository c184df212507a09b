// Surface normals from the geometry head: g = d geo_out / d x at the gaussian mean x = o + d (t0 + t1) / 2 of every sample,
// geo_out = the first output of the geometry MLP (the SDF, or the pre-exp logit in density mode); the contract, the sign and
// the error bound are stated in include/neurad_hip.h at nrhip_field_normals.  The operator route composes it from four
// kernels (encode_fwd -> mlp_fwd -> mlp_bwd of a unit cotangent -> encode_bwd_rays on [N,1] rays): two [N, L*F] round trips,
// weight gradients nobody wants and 8 L gathers per sample twice.  Here one thread carries one sample through the chain:
//
//   primal    sample_gaussian -> contract_gaussian -> per level hash_corners, 8 gathers, the forward's lerp tree and
//             rescale weight: position, cells, offsets and the encoding row are the bits nrhip_field_fwd computes.
//   ONE WALK  the corners are gathered once.  Beside the level's value the walk keeps d lerp / d offset per feature
//             (3 L F registers) instead of the 8 L F corner values; the rescaled value doubles as the d / d std factor
//             (enc = w val, so sum g val = sum g enc / w).  No second walk, no re-gather.
//   MLP       fp32 VALU: z_j = b0_j + W0_j . enc as an fma chain over the encoding columns, geo = b1_0 + sum_j w1_0j relu(z_j),
//             d geo / d enc = sum_j [z_j > 0] w1_0j W0_j as an fma chain over j -- only row 0 of the last layer is read, no
//             weight gradient is formed.  The weight rows are read at wave-uniform addresses (scalar loads, no LDS).
//   backward  the level sums contracted with the kept derivatives, the std term where clamp_min passes (2 scal_l s >= 1), the
//             contraction's backward with torch's inf-norm tie split: the arithmetic of encode_bwd_rays_kernel
//             (hashgrid_dx.hip), whose [N,1]-ray origin gradient this is.
//
// Thread mapping as encode_bwd_rays_kernel: a group of G lanes per ray, lane `sub` takes the samples sub, sub + G, ... of the
// ray in that order; with weights the lanes' partial sums of w n meet in an xor butterfly and lane 0 WRITES the ray's row.  No
// atomics, nothing allocated, no host synchronisation: every output element has one writer and the launch can be captured.
// A ray's row depends on its own samples and on G alone.  One kernel body for dense ([R,S] with a row stride) and packed
// (segments) samples through the ray_sample_* accessors of common.h.
#include "actors_dev.h"
#include "render_variants.h"
#include <type_traits>

namespace nrhip {
namespace {

// What a lane of the actor form walks instead of the static table when its sample lies in a box: that actor's table, the
// actor grid (La <= L levels; its scalings are zero from La on, so those levels add nothing) and the actor scale.
struct BoxWalk {
  bool in;
  const void* table;
  float scale;
};

// (The actor form's zero scratch rests on this barrier and on how one compiler version treats it: after a compiler upgrade
//  re-check the table of profiles/LEDGER.md with -Rpass-analysis=kernel-resource-usage.)
template <class T>
__device__ __forceinline__ T pin_uniform(T v) {  // a wave-uniform value, held in a scalar register from here on
  asm volatile("" : "+s"(v));
  return v;
}

// d geo / d mean of one sample and geo itself.  w0 [H, L*F], b0 [H], w1 [H] = row 0 of the last layer, b1 its bias: all read
// at wave-uniform addresses.  ACT: the lane's table, scalings, table size and scale are selected per lane by bw.in (the
// static form ignores bw); gs is then the box-frame position with the sample's own std, and g the box-frame gradient.
template <int L, int F, int H, bool HALF, bool ACT>
__device__ __forceinline__ void normals_of_sample(const GridDev& grid, const void* __restrict__ table_, float scale_,
                                                  const float* __restrict__ w0, const float* __restrict__ b0,
                                                  const float* __restrict__ w1, const float* __restrict__ b1,
                                                  const SamplePos& gs, const GridDev& agrid, const BoxWalk& bw, float& geo,
                                                  float (&g)[3]) {
  constexpr int LF = L * F;
  const bool box = ACT && bw.in;
  // (the actor grid's members are pinned in scalar registers before the select: left alone, the compiler selects between
  //  the two ADDRESSES in the kernel arguments and loads once, for which it copies every argument to scratch)
  const int log2T = box ? pin_uniform(agrid.log2T) : grid.log2T;
  const void* table = box ? bw.table : table_;
  const float scale = box ? bw.scale : scale_;
  const int La = box ? pin_uniform(agrid.L) : L;  // (levels from La on are not gathered: F.pad's zero columns)
  auto scal = [&](int l) { return box ? pin_uniform(agrid.scal[l]) : grid.scal[l]; };
  const uint32_t mask = (1u << log2T) - 1u;
  const SamplePos p = contract_gaussian(gs.x, gs.y, gs.z, gs.std, scale);
  float enc[LF], Dx[LF], Dy[LF], Dz[LF];
  // the gathers of LG levels are in flight together (64 result registers; 32 at F = 2, where 16 levels' index registers
  // come on top and 64 cost the second wave per SIMD); the scheduling barrier keeps the compiler from hoisting every level's
  // 8 F loads in front of the first blend, which costs more registers than there are
  constexpr int kInFlight = F == 2 ? 32 : 64;
  constexpr int LG = 8 * F >= kInFlight ? 1 : (kInFlight / (8 * F) < L ? kInFlight / (8 * F) : L);
#pragma unroll
  for (int l0 = 0; l0 < L; l0 += LG) {
    Corners c[LG];
    float f[LG][8][F];
#pragma unroll
    for (int i = 0; i < LG; ++i) {
      if (l0 + i >= L) break;
      c[i] = hash_corners(p.x, p.y, p.z, scal(l0 + i), mask);
      if (ACT && l0 + i >= La) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
          for (int q = 0; q < F; ++q) f[i][k][q] = 0.f;
        continue;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) Entry<F, HALF>::load(table, ((uint32_t)(l0 + i) << log2T) + c[i].idx[k], f[i][k]);
    }
#pragma unroll
    for (int i = 0; i < LG; ++i) {
      if (l0 + i >= L) break;
      const int l = l0 + i;
      const float ox = c[i].ox, oy = c[i].oy, oz = c[i].oz, mx = 1.f - ox, my = 1.f - oy, mz = 1.f - oz;
      const float rw = rescale_weight(scal(l), p.std);
#pragma unroll
      for (int q = 0; q < F; ++q) {
        const float(&v)[8][F] = f[i];
        // the value: lerp_corners' tree, so the encoding row has the forward's bits
        const float f03 = fmaf(v[0][q], ox, v[3][q] * mx), f12 = fmaf(v[1][q], ox, v[2][q] * mx);
        const float f56 = fmaf(v[5][q], ox, v[6][q] * mx), f47 = fmaf(v[4][q], ox, v[7][q] * mx);
        const float f0312 = fmaf(f03, oy, f12 * my), f4756 = fmaf(f47, oy, f56 * my);
        enc[l * F + q] = fmaf(f0312, oz, f4756 * mz) * rw;
        // d value / d offset (corner order: 0 ccc, 1 cfc, 2 ffc, 3 fcc, 4 ccf, 5 cff, 6 fff, 7 fcf)
        const float d03 = v[0][q] - v[3][q], d12 = v[1][q] - v[2][q], d56 = v[5][q] - v[6][q], d47 = v[4][q] - v[7][q];
        Dx[l * F + q] = (d03 * oy + d12 * my) * oz + (d47 * oy + d56 * my) * mz;
        Dy[l * F + q] = (f03 - f12) * oz + (f47 - f56) * mz;
        Dz[l * F + q] = f0312 - f4756;
        // (the results are pinned here: left alone, the compiler sinks the blend behind the MLP loop and keeps every corner)
        asm volatile("" : "+v"(enc[l * F + q]), "+v"(Dx[l * F + q]), "+v"(Dy[l * F + q]), "+v"(Dz[l * F + q]));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // geometry layer 0, the ReLU mask, row 0 of the last layer, and back to d geo / d enc
  float ge[LF];
#pragma unroll
  for (int k = 0; k < LF; ++k) ge[k] = 0.f;
  geo = b1[0];
#pragma unroll 2
  for (int j = 0; j < H; ++j) {
    float wr[LF];
#pragma unroll
    for (int k = 0; k < LF; ++k) wr[k] = w0[j * LF + k];
    float z = b0[j];
#pragma unroll
    for (int k = 0; k < LF; ++k) z = fmaf(wr[k], enc[k], z);
    const float w1j = w1[j];
    geo = fmaf(w1j, fmaxf(z, 0.f), geo);
    const float a = z > 0.f ? w1j : 0.f;  // ReLU'(0) = 0
#pragma unroll
    for (int k = 0; k < LF; ++k) ge[k] = fmaf(a, wr[k], ge[k]);
  }
  // the level sums: d geo / d x01 and d geo / d (contracted std)
  float gx = 0.f, gy = 0.f, gz = 0.f, gstd = 0.f;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const float sc = scal(l);
    float dx = 0.f, dy = 0.f, dz = 0.f, dv = 0.f;
#pragma unroll
    for (int q = 0; q < F; ++q) {
      const float gq = ge[l * F + q];
      dx += gq * Dx[l * F + q], dy += gq * Dy[l * F + q], dz += gq * Dz[l * F + q], dv += gq * enc[l * F + q];
    }
    const float a2 = sc * 2.f * p.std;
    const float w = rescale_weight(sc, p.std);
    gx += (sc * w) * dx, gy += (sc * w) * dy, gz += (sc * w) * dz;
    if (a2 >= 1.f) gstd -= dv * (2.f * sc) * w;  // clamp_min passes the gradient at equality; dv carries one w already
  }
  // contraction backward: (gx, gy, gz) = d geo / d x01, gstd = d geo / d cstd  ->  d geo / d mean
  const float u[3] = {gs.x / scale, gs.y / scale, gs.z / scale};
  const float au[3] = {fabsf(u[0]), fabsf(u[1]), fabsf(u[2])};
  const float mag = fmaxf(fmaxf(au[0], au[1]), au[2]);
  float gm[3] = {gx / 4.f, gy / 4.f, gz / 4.f};
  if (!(mag < 1.f)) {
    const float k = 2.f / mag - 1.f / (mag * mag), dk = -2.f / (mag * mag) + 2.f / (mag * mag * mag);
    const float cr = cbrtf(2.f * mag - 1.f), rr = cr / mag;
    const float dq = 2.f * rr * ((2.f / 3.f) / (cr * cr * mag) - cr / (mag * mag));
    const float g_mag = (gm[0] * u[0] + gm[1] * u[1] + gm[2] * u[2]) * dk + gstd * (gs.std / scale) * dq / 4.f;
    inf_norm_bwd(u, au, mag, k, g_mag, gm);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = gm[c] / scale;
}

__device__ __forceinline__ int64_t weight_index(const RaysDev& r, int64_t ray, int s, int wstride) {
  return ray * wstride + s;
}
__device__ __forceinline__ int64_t weight_index(const PackedRaysDev& r, int64_t ray, int s, int) {
  return ray_sample_row(r, ray, s);
}

// The actor form's extra arguments: the per-RAY candidate lists of nrhip_actor_prepare (a.K entries a row), the actors
// (a.flip: the per-ray x flip or NULL) and the two optional per-sample outputs.  The static form carries none of it.
struct NoActors {};
struct ActorArgs {
  ActorsDev a;
  const int32_t* cand_count;
  const int32_t* cand_actor;
  const float* cand_w2b;
  int32_t* hit;   // [N] or NULL
  float* boxpos;  // [N,3] or NULL
};

__device__ __forceinline__ bool actor_outputs(const NoActors&) { return false; }
__device__ __forceinline__ bool actor_outputs(const ActorArgs& a) { return a.hit || a.boxpos; }

// L, F, H: a `PerSample, Static, F32` row of render_variants.h; HALF: fp16 table; Rays: RaysDev or PackedRaysDev.
// sign: +1 (SDF: the normal points towards free space) or -1 (density mode).  weights (optional) with its row stride (dense),
// geo / grad / nrm / ray_nrm: optional outputs.  G: lanes per ray, a power of two <= 64.
// Act: NoActors (the static form) or ActorArgs -- the actor form, an instantiation of its own (the (L, F, H) of a
// `Composite, Actors, F32` row of render_variants.h), so the static kernels keep their registers.
template <int L, int F, int H, bool HALF, class Rays, class Act>
__global__ __launch_bounds__(256) void field_normals_kernel(
    GridDev grid, const void* __restrict__ table, float scale, const float* __restrict__ w0, const float* __restrict__ b0,
    const float* __restrict__ w1, const float* __restrict__ b1, float sign, Rays r, const int32_t* __restrict__ order,
    const float* __restrict__ weights, int wstride, int G, float* __restrict__ geo, float* __restrict__ grad,
    float* __restrict__ nrm, float* __restrict__ ray_nrm, Act act) {
  constexpr bool ACT = !std::is_same<Act, NoActors>::value;
  const int lane = threadIdx.x & 63;
  const int sub = lane & (G - 1);
  const int64_t slot = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const bool live_ray = slot < r.R;
  const bool per_sample = geo || grad || nrm || actor_outputs(act);
  float acc[3] = {0.f, 0.f, 0.f};
  int64_t ray = slot;
  if (live_ray) {
    if (order) {  // a locality hint: the slot's ray, clamped into the batch
      const int64_t q = order[slot];
      ray = q < 0 ? 0 : (q < r.R ? q : r.R - 1);
    }
    const float ox_ = r.o[3 * ray], oy_ = r.o[3 * ray + 1], oz_ = r.o[3 * ray + 2];
    const float dx_ = r.d[3 * ray], dy_ = r.d[3 * ray + 1], dz_ = r.d[3 * ray + 2];
    const float area = r.area[ray];
    const int n = ray_sample_count(r, ray);
    int ncand = 0;
    if constexpr (ACT) ncand = act.cand_count[ray];
    for (int s = sub; s < n; s += G) {
      float w = 0.f;
      if (weights) {
        w = weights[weight_index(r, ray, s, wstride)];
        if (w == 0.f && !per_sample) continue;  // no gathers, no contribution -- not even a NaN
      }
      const int64_t ti = ray_sample_interval(r, ray, s);
      const SamplePos gs = sample_gaussian(ox_, oy_, oz_, dx_, dy_, dz_, area, r.starts[ti], r.ends[ti]);
      float v, g[3];
      int hit_actor = -1;
      float bp[3] = {0.f, 0.f, 0.f};
      if constexpr (ACT) {
        // actors.hip's hit test on the ray's candidates; an in-box lane walks its actor's table at the box-frame position
        // (the sample's own std), and its box-frame gradient goes back through the flip and W^T
        ActorHit h;
        h.actor = -1, h.dx = dx_, h.dy = dy_, h.dz = dz_;
        const float* wsel = ncand ? find_hit_core(act.a, ray, ncand, gs, act.cand_actor, act.cand_w2b, h) : nullptr;
        const bool in_box = h.actor >= 0;
        SamplePos q = gs;
        if (in_box) q.x = h.px, q.y = h.py, q.z = h.pz;
        const BoxWalk bw{in_box, in_box ? act.a.tables[h.actor] : nullptr, act.a.scale};
        normals_of_sample<L, F, H, HALF, true>(grid, table, scale, w0, b0, w1, b1, q, act.a.grid, bw, v, g);
        if (in_box) {
          const float bx = act.a.flip ? g[0] * act.a.flip[ray] : g[0], by = g[1], bz = g[2];
#pragma unroll
          for (int c = 0; c < 3; ++c) g[c] = wsel[c] * bx + wsel[4 + c] * by + wsel[8 + c] * bz;
          bp[0] = h.px, bp[1] = h.py, bp[2] = h.pz;
        }
        hit_actor = h.actor;
      } else {
        normals_of_sample<L, F, H, HALF, false>(grid, table, scale, w0, b0, w1, b1, gs, grid, BoxWalk{}, v, g);
      }
      const float len = fmaxf(sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), 1e-12f);
      const float nx = sign * g[0] / len, ny = sign * g[1] / len, nz = sign * g[2] / len;
      const int64_t i = ray_sample_row(r, ray, s);
      if (geo) geo[i] = v;
      if (grad) grad[3 * i] = g[0], grad[3 * i + 1] = g[1], grad[3 * i + 2] = g[2];
      if (nrm) nrm[3 * i] = nx, nrm[3 * i + 1] = ny, nrm[3 * i + 2] = nz;
      if constexpr (ACT) {
        if (act.hit) act.hit[i] = hit_actor;
        if (act.boxpos && hit_actor >= 0) act.boxpos[3 * i] = bp[0], act.boxpos[3 * i + 1] = bp[1], act.boxpos[3 * i + 2] = bp[2];
      }
      if (w != 0.f) acc[0] += w * nx, acc[1] += w * ny, acc[2] += w * nz;
    }
  }
  if (!ray_nrm) return;  // (the same in every thread)
  for (int off = 1; off < G; off <<= 1)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += __shfl_xor(acc[c], off, 64);
  if (live_ray && sub == 0)
#pragma unroll
    for (int c = 0; c < 3; ++c) ray_nrm[3 * ray + c] = acc[c];
}

struct NormalsLaunch {
  const nrhip_field* f;
  const ActorArgs* act;  // NULL: the static form
  const int32_t* order;
  const float* weights;
  int wstride, G;
  float *geo, *grad, *nrm, *ray_nrm;
  hipStream_t st;
};

template <int L, int F, int H, bool HALF, class Rays>
void launch_normals(const NormalsLaunch& a, const Rays& rd) {
  const nrhip_mlp& m = a.f->geo;
  const int blocks = grid_for(rd.R * a.G, 256);
  field_normals_kernel<L, F, H, HALF, Rays, NoActors><<<blocks, 256, 0, a.st>>>(
      to_dev(a.f->grid), a.f->table, a.f->static_scale, m.weight[0], m.bias[0], m.weight[1], m.bias[1],
      a.f->use_sdf ? 1.f : -1.f, rd, a.order, a.weights, a.wstride, a.G, a.geo, a.grad, a.nrm, a.ray_nrm, NoActors{});
}

template <int L, int F, int H, bool HALF, class Rays>
void launch_normals_actors(const NormalsLaunch& a, const Rays& rd) {
  const nrhip_mlp& m = a.f->geo;
  const int blocks = grid_for(rd.R * a.G, 256);
  field_normals_kernel<L, F, H, HALF, Rays, ActorArgs><<<blocks, 256, 0, a.st>>>(
      to_dev(a.f->grid), a.f->table, a.f->static_scale, m.weight[0], m.bias[0], m.weight[1], m.bias[1],
      a.f->use_sdf ? 1.f : -1.f, rd, a.order, a.weights, a.wstride, a.G, a.geo, a.grad, a.nrm, a.ray_nrm, *a.act);
}

// The instantiations: the (L, F, H) of every `PerSample, Static, F32` row of render_variants.h, fp32 and fp16 tables, both
// sample layouts.  The other rows of the table select the empty specialisation.
constexpr bool normals_row(Out out, Src src, Prod prod) {
  return out == Out::PerSample && src == Src::Static && prod == Prod::F32;
}
// ... and the actor form: the (L, F, H) of every `Composite, Actors, F32` row (the shapes the fused eval render covers)
constexpr bool normals_actors_row(Out out, Src src, Prod prod) {
  return out == Out::Composite && src == Src::Actors && prod == Prod::F32;
}
template <int L, int F, int H, bool ROW>
struct NormalsRow {
  template <class Rays>
  static void go(const NormalsLaunch&, const Rays&) {}
};
template <int L, int F, int H>
struct NormalsRow<L, F, H, true> {
  template <class Rays>
  static void go(const NormalsLaunch& a, const Rays& rd) {
    if (a.f->grid.param_dtype == 1) launch_normals<L, F, H, true, Rays>(a, rd);
    else launch_normals<L, F, H, false, Rays>(a, rd);
  }
};

template <int L, int F, int H, bool ROW>
struct NormalsActorsRow {
  template <class Rays>
  static void go(const NormalsLaunch&, const Rays&) {}
};
template <int L, int F, int H>
struct NormalsActorsRow<L, F, H, true> {
  template <class Rays>
  static void go(const NormalsLaunch& a, const Rays& rd) {
    if (a.f->grid.param_dtype == 1) launch_normals_actors<L, F, H, true, Rays>(a, rd);
    else launch_normals_actors<L, F, H, false, Rays>(a, rd);
  }
};

bool normals_actors_shape(int L, int F, int H) {
#define X(L_, F_, H_, O_, S_, P_) \
  if (normals_actors_row(Out::O_, Src::S_, Prod::P_) && L == L_ && F == F_ && H == H_) return true;
  NRHIP_RENDER_VARIANTS(X)
#undef X
  return false;
}

bool normals_shape(int L, int F, int H) {
#define X(L_, F_, H_, O_, S_, P_) \
  if (normals_row(Out::O_, Src::S_, Prod::P_) && L == L_ && F == F_ && H == H_) return true;
  NRHIP_RENDER_VARIANTS(X)
#undef X
  return false;
}

template <class Rays>
int dispatch_normals(const char* who, const NormalsLaunch& a, const Rays& rd) {
  const int L = a.f->grid.num_levels, F = a.f->grid.n_features, H = a.f->geo.hidden_dim;
#define X(L_, F_, H_, O_, S_, P_)                                                                       \
  if (a.act && normals_actors_row(Out::O_, Src::S_, Prod::P_) && L == L_ && F == F_ && H == H_) {       \
    NormalsActorsRow<L_, F_, H_, normals_actors_row(Out::O_, Src::S_, Prod::P_)>::go(a, rd);            \
    return check_launch(who);                                                                           \
  }
  NRHIP_RENDER_VARIANTS(X)
#undef X
#define X(L_, F_, H_, O_, S_, P_)                                                            \
  if (!a.act && normals_row(Out::O_, Src::S_, Prod::P_) && L == L_ && F == F_ && H == H_) {            \
    NormalsRow<L_, F_, H_, normals_row(Out::O_, Src::S_, Prod::P_)>::go(a, rd);              \
    return check_launch(who);                                                                \
  }
  NRHIP_RENDER_VARIANTS(X)
#undef X
  set_error("%s: no instantiation for L=%d F=%d H=%d", who, L, F, H);
  return NRHIP_ERR_UNSUPPORTED;
}

// what every entry point checks of the field and of the outputs, before any count is looked at.  actors: the actor form
// (shapes: the `Composite, Actors, F32` rows; extra: whether one of its own outputs, hit / box_position, is asked for)
int validate_normals(const char* who, const nrhip_field* f, const float* geo, const float* grad, const float* nrm,
                     const float* ray_nrm, bool actors = false, bool extra = false) {
  NR_REQUIRE(f, NRHIP_ERR_INVALID_ARG, "%s: field descriptor is NULL", who);
  if (int e = validate_grid(&f->grid)) return e;
  NR_REQUIRE(f->table && f->static_scale > 0.f, NRHIP_ERR_INVALID_ARG, "%s: NULL table or non-positive scale", who);
  const nrhip_mlp& m = f->geo;
  const int L = f->grid.num_levels, F = f->grid.n_features;
  NR_REQUIRE(m.num_layers == 2 && m.in_dim == L * F && m.out_dim >= 1 &&
                 (actors ? normals_actors_shape(L, F, m.hidden_dim) : normals_shape(L, F, m.hidden_dim)),
             NRHIP_ERR_UNSUPPORTED,
             "%s: no instantiation for L=%d F=%d and a geometry MLP %d -> %d -> %d of %d layers (the `%s, F32` rows of "
             "csrc/render_variants.h, 2 layers); compose the operators instead",
             who, L, F, m.in_dim, m.hidden_dim, m.out_dim, m.num_layers, actors ? "Composite, Actors" : "PerSample, Static");
  NR_REQUIRE(m.weight[0] && m.weight[1], NRHIP_ERR_INVALID_ARG, "%s: a geometry weight is NULL", who);
  NR_REQUIRE(m.bias[0] && m.bias[1], NRHIP_ERR_UNSUPPORTED, "%s: the geometry MLP has a layer without bias; compose the operators instead", who);
  NR_REQUIRE(geo || grad || nrm || ray_nrm || extra, NRHIP_ERR_INVALID_ARG, "%s: every output is NULL", who);
  return NRHIP_OK;
}

// the actor form's own checks, after validate_normals: descriptors and candidate pointers, then the actor grid against the
// static one (the condition of the fused eval render: the same F and storage type, La <= L)
int validate_normals_actors(const char* who, const nrhip_field* f, const nrhip_actors* actors, const int32_t* cand_count,
                            const int32_t* cand_actor, const float* cand_w2b, const float* ray_flip, int32_t* hit,
                            float* boxpos, ActorArgs& act) {
  if (int e = to_dev(actors, act.a)) return e;
  NR_REQUIRE(cand_count && cand_actor && cand_w2b, NRHIP_ERR_INVALID_ARG, "%s: a candidate list is NULL", who);
  if (int e = validate_grid(&actors->grid)) return e;
  NR_REQUIRE(actors->tables && actors->actor_scale > 0.f, NRHIP_ERR_INVALID_ARG, "%s: NULL actor tables or non-positive actor scale", who);
  NR_REQUIRE(actors->grid.n_features == f->grid.n_features && actors->grid.param_dtype == f->grid.param_dtype &&
                 actors->grid.num_levels <= f->grid.num_levels,
             NRHIP_ERR_UNSUPPORTED,
             "%s: the actor grid (L=%d F=%d dtype %d) must share the static grid's F=%d and storage type %d with at most its "
             "L=%d levels; compose the operators instead",
             who, actors->grid.num_levels, actors->grid.n_features, actors->grid.param_dtype, f->grid.n_features,
             f->grid.param_dtype, f->grid.num_levels);
  act.a.flip = ray_flip;
  act.cand_count = cand_count, act.cand_actor = cand_actor, act.cand_w2b = cand_w2b;
  act.hit = hit, act.boxpos = boxpos;
  return NRHIP_OK;
}

int lanes_per_ray(int64_t samples_per_ray) {  // the power of two >= the count, in [1, 64]
  int g = 1;
  while (g < 64 && g < samples_per_ray) g <<= 1;
  return g;
}

}  // namespace
}  // namespace nrhip

using namespace nrhip;

// the dense and the packed entry body, once for the static form (act == NULL) and the actor form
static int normals_dense(const char* who, const nrhip_field* f, const ActorArgs* act, const nrhip_rays* rays,
                         const float* weights, int32_t weight_stride, float* geo, float* gradient, float* normals,
                         float* ray_normals, void* stream) {
  if (int e = validate_rays(rays)) return e;
  const int64_t R = rays->n_rays;
  const int S = rays->n_samples;
  NR_REQUIRE(weight_stride == 0 || weight_stride >= S, NRHIP_ERR_INVALID_ARG, "%s: weight_stride %d < n_samples %d", who,
             weight_stride, S);
  // (a batch without samples has no weights to point to: its rows are zeros)
  NR_REQUIRE(weights || !ray_normals || R == 0 || S == 0, NRHIP_ERR_INVALID_ARG, "%s: ray_normals without weights", who);
  if (R == 0) return NRHIP_OK;
  const hipStream_t st = (hipStream_t)stream;
  if (S == 0) {  // rays without samples: rows of zeros, no launch
    if (ray_normals && hipMemsetAsync(ray_normals, 0, (size_t)R * 3 * sizeof(float), st) != hipSuccess)
      return check_launch(who);
    return NRHIP_OK;
  }
  const NormalsLaunch a{f,   act,      rays->order, weights,     weight_stride ? weight_stride : S, lanes_per_ray(S),
                        geo, gradient, normals,     ray_normals, st};
  return dispatch_normals(who, a, to_dev(*rays));
}

static int normals_packed(const char* who, const nrhip_field* f, const ActorArgs* act, const nrhip_packed_rays* rays,
                          const float* weights, float* geo, float* gradient, float* normals, float* ray_normals,
                          void* stream) {
  if (int e = validate_packed_rays(who, rays, true)) return e;
  const int64_t R = rays->n_rays, M = rays->n_samples;
  NR_REQUIRE(M == 0 || R > 0, NRHIP_ERR_INVALID_ARG, "%s: samples without rays", who);
  NR_REQUIRE(weights || !ray_normals || M == 0, NRHIP_ERR_INVALID_ARG, "%s: ray_normals without weights", who);
  if (R == 0) return NRHIP_OK;
  const hipStream_t st = (hipStream_t)stream;
  if (M == 0) {  // no ray has a sample: rows of zeros, no sample pointer is read
    if (ray_normals && hipMemsetAsync(ray_normals, 0, (size_t)R * 3 * sizeof(float), st) != hipSuccess)
      return check_launch(who);
    return NRHIP_OK;
  }
  // the dense rule on the mean count (both are shapes: no device read)
  const NormalsLaunch a{f,   act,      rays->order, weights,     0, lanes_per_ray((M + R - 1) / R),
                        geo, gradient, normals,     ray_normals, st};
  return dispatch_normals(who, a, to_dev(*rays));
}

extern "C" int nrhip_field_normals(const nrhip_field* f, const nrhip_rays* rays, const float* weights,
                                   int32_t weight_stride, float* geo, float* gradient, float* normals, float* ray_normals,
                                   void* stream) {
  const char* who = "field_normals";
  if (int e = validate_normals(who, f, geo, gradient, normals, ray_normals)) return e;
  return normals_dense(who, f, nullptr, rays, weights, weight_stride, geo, gradient, normals, ray_normals, stream);
}

extern "C" int nrhip_field_normals_packed(const nrhip_field* f, const nrhip_packed_rays* rays, const float* weights,
                                          float* geo, float* gradient, float* normals, float* ray_normals, void* stream) {
  const char* who = "field_normals_packed";
  if (int e = validate_normals(who, f, geo, gradient, normals, ray_normals)) return e;
  return normals_packed(who, f, nullptr, rays, weights, geo, gradient, normals, ray_normals, stream);
}

extern "C" int nrhip_field_normals_actors(const nrhip_field* f, const nrhip_actors* actors, const nrhip_rays* rays,
                                          const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                                          const float* ray_flip, const float* weights, int32_t weight_stride, float* geo,
                                          float* gradient, float* normals, float* ray_normals, int32_t* hit,
                                          float* box_position, void* stream) {
  const char* who = "field_normals_actors";
  ActorArgs act;
  if (int e = validate_normals(who, f, geo, gradient, normals, ray_normals, true, hit || box_position)) return e;
  if (int e = validate_normals_actors(who, f, actors, cand_count, cand_actor, cand_w2b, ray_flip, hit, box_position, act))
    return e;
  return normals_dense(who, f, &act, rays, weights, weight_stride, geo, gradient, normals, ray_normals, stream);
}

extern "C" int nrhip_field_normals_packed_actors(const nrhip_field* f, const nrhip_actors* actors,
                                                 const nrhip_packed_rays* rays, const int32_t* cand_count,
                                                 const int32_t* cand_actor, const float* cand_w2b, const float* ray_flip,
                                                 const float* weights, float* geo, float* gradient, float* normals,
                                                 float* ray_normals, int32_t* hit, float* box_position, void* stream) {
  const char* who = "field_normals_packed_actors";
  ActorArgs act;
  if (int e = validate_normals(who, f, geo, gradient, normals, ray_normals, true, hit || box_position)) return e;
  if (int e = validate_normals_actors(who, f, actors, cand_count, cand_actor, cand_w2b, ray_flip, hit, box_position, act))
    return e;
  return normals_packed(who, f, &act, rays, weights, geo, gradient, normals, ray_normals, stream);
}
