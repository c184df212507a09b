// The per-sample geometry of the dynamic actors, shared by actors.hip (encode, density, hits, the packed find) and
// normals.hip (the actor-aware normals): the device view of nrhip_actors, the per-sample hit and the one walk over a ray's
// candidate list that decides it.  One body, so every kernel that asks "which box holds this sample" gets the same bits.
#pragma once
#include "common.h"

namespace nrhip {

struct ActorsDev {
  int A, Tn;
  const float* ts;
  const float* pos;
  const float* rot6;
  const uint8_t* present;
  const float* bounds;
  GridDev grid;
  const void* const* tables;
  float scale;
  const float* flip;  // [R] +-1 per ray (training-mode x flip, neurad_encoding.py:212-219) or NULL
  int K;              // row length of the per-ray candidate lists (nrhip_actors.max_candidates; == A: no ray overflows)
};

// shared per-sample part: which actor (if any) contains the sample; box-frame position/direction
struct ActorHit {
  int actor;  // -1: none
  float px, py, pz, std, dx, dy, dz;
};

// The walk over the n > 0 candidates of `ray` for a sample with gaussian g: h.actor / h.px.. / h.std, the box-frame view
// direction (h.dx.. hold the ray's world direction on entry) and the flip.  -> the winner's world2box row (NULL: no hit).
__device__ __forceinline__ const float* find_hit_core(const ActorsDev& a, int64_t ray, int n, const SamplePos& g,
                                                      const int32_t* cand_actor, const float* cand_w2b, ActorHit& h) {
  h.std = g.std;
  const float* wsel = nullptr;
  for (int c = 0; c < n; ++c) {  // ascending actor index; the LAST hit wins (neurad_encoding.py:184-185 on CPU)
    const float* w = cand_w2b + (ray * a.K + c) * 12;
    const int act = cand_actor[ray * a.K + c];
    float bx, by, bz;
    if (box_contains(w, a.bounds + 3 * act, g.x, g.y, g.z, bx, by, bz)) {
      h.actor = act, h.px = bx, h.py = by, h.pz = bz, wsel = w;
    }
  }
  if (h.actor >= 0) {
    float ddx = wsel[0] * h.dx + wsel[1] * h.dy + wsel[2] * h.dz;
    float ddy = wsel[4] * h.dx + wsel[5] * h.dy + wsel[6] * h.dz;
    float ddz = wsel[8] * h.dx + wsel[9] * h.dy + wsel[10] * h.dz;
    const float nn = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz) + 1e-7f;  // neurad_encoding.py:207
    h.dx = ddx / nn, h.dy = ddy / nn, h.dz = ddz / nn;
    if (a.flip) {
      const float f = a.flip[ray];
      h.px *= f, h.dx *= f;
    }
  }
  return wsel;
}

// RD: RaysDev (row i = ray * S + s) or PackedRaysDev (row i = packed sample index, its ray from ray_of): one body, so the two
// layouts agree bit for bit on every sample (common.h: ray_sample_ray_of_row / ray_sample_interval_of_row)
template <class RD>
__device__ __forceinline__ ActorHit find_hit(const ActorsDev& a, const RD& r, const int64_t* ray_of, int64_t i,
                                             const int32_t* cand_count, const int32_t* cand_actor,
                                             const float* cand_w2b) {
  ActorHit h;
  h.actor = -1;
  const int64_t ray = ray_sample_ray_of_row(r, ray_of, i);
  const int n = cand_count[ray];
  h.dx = r.d[3 * ray], h.dy = r.d[3 * ray + 1], h.dz = r.d[3 * ray + 2];
  if (n == 0) return h;
  const int64_t iv = ray_sample_interval_of_row(r, ray, i);
  const SamplePos g = sample_gaussian(r.o[3 * ray], r.o[3 * ray + 1], r.o[3 * ray + 2], h.dx, h.dy, h.dz, r.area[ray],
                                      r.starts[iv], r.ends[iv]);
  find_hit_core(a, ray, n, g, cand_actor, cand_w2b, h);
  return h;
}

inline int to_dev(const nrhip_actors* a, ActorsDev& d) {
  NR_REQUIRE(a, NRHIP_ERR_INVALID_ARG, "actors descriptor is NULL");
  NR_REQUIRE(a->n_actors >= 1 && a->n_times >= 1, NRHIP_ERR_INVALID_ARG, "actors: need >= 1 actor and timestamp");
  NR_REQUIRE(a->timestamps && a->positions && a->rotations_6d && a->present && a->bounds, NRHIP_ERR_INVALID_ARG,
             "actors descriptor has a NULL pointer");
  d.A = a->n_actors, d.Tn = a->n_times;
  d.K = a->max_candidates > 0 ? a->max_candidates : NRHIP_DEFAULT_ACTOR_CANDIDATES;
  d.ts = a->timestamps, d.pos = a->positions, d.rot6 = a->rotations_6d, d.present = a->present, d.bounds = a->bounds;
  d.grid = to_dev(a->grid);
  d.tables = a->tables;
  d.scale = a->actor_scale;
  d.flip = nullptr;
  return NRHIP_OK;
}

}  // namespace nrhip
