"""Scenes and a float64 reference for exact tests of the occupancy march (march_ray, csrc/occgrid.hip) -- TEST INFRASTRUCTURE
ONLY, written from the rule stated at the top of that file, not from the kernel and not from the fp32 restatements
(oracle/occgrid_oracle.py:occgrid_march, tests/occgrid_update_restatement.py:march_levels).

The march uses +, *, /, floor, min and max (powf in the cone branch only).  On a dyadic lattice every intermediate is exact
in fp32, so the fp32 result IS the float64 result, with or without FMA contraction, also when a midpoint lies exactly on a
cell face or on a level's box face:
  * boxes: level l is [-4 * 2^l, 4 * 2^l]^3, res = 8: cells 1, 2 and 4 wide.  The single grid is the outermost of them,
    [-16, 16]^3, so that one set of rays has the same candidate intervals at L = 1 and at L = 3;
  * direction components from {0, -0.0, +-1, +-0.5, +-0.25} (not unit length: the kernel does not ask for it), 1 / d exact;
  * origins, t_min, t_max and near_plane multiples of 1/8, t_rand from {0, 0.25, 0.5, 0.984375}, step 0.25 or 0.5.
The kernel must match march64 bit for bit: no tolerance, no excluded band.  tests/test_march_exact_refs_host.py proves the
design (march64 == both fp32 restatements, bit for bit) and asserts every property of the scenes the GPU test leans on."""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64

RES, LEVELS = 8, 3
NEAR, FAR = 0.5, 64.0
STEPS = (0.25, 0.5)
RAY_COUNTS = (1, 2, 3, 5, 61)  # prefixes of the 61 rays; one workgroup marches 4 rays: 1, 2, 3, 5 and 61 all end ragged
CAPS = (1, 63, 64, 65, 100, 127, 128, 129, 200)
T_RANDS = (0.0, 0.25, 0.5, 0.984375)
DIR_COMPONENTS = (0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25)


def level_boxes(levels=LEVELS):
    """fp32 [levels, 6]; levels = 1: the single grid, the OUTERMOST box of the three-level grid"""
    halves = [4.0 * 2 ** l for l in range(LEVELS)]
    halves = halves[-1:] if levels == 1 else halves[:levels]
    return np.array([[-h, -h, -h, h, h, h] for h in halves], f32)


def random_binaries(seed=3):
    """bool [3, 8, 8, 8], about one half set; the single grid takes level 2's"""
    return np.random.default_rng(seed).random((LEVELS, RES, RES, RES)) < 0.5


def binaries_for(kind, levels):
    b = {"random": random_binaries(), "ones": np.ones((LEVELS, RES, RES, RES), bool),
         "zeros": np.zeros((LEVELS, RES, RES, RES), bool)}[kind]
    return b[-1:] if levels == 1 else b[:levels]


# ---- the designed rays.  Outermost box [-16, 16]^3, near_plane 0.5, far_plane 64; n25 / n50: the candidate count at step 0.25
# / 0.5 WITH the ray's t_min, t_max and t_rand, worked out by hand: ceil((t_far - t_near) / step) ----------------------------
def _ray(name, o, d, t_min, t_max, n25, n50, t_rand=0.0):
    return dict(name=name, o=o, d=d, t_min=t_min, t_max=t_max, t_rand=t_rand, n25=n25, n50=n50)


DESIGNED_HEAD = [
    # x slab [-36, -4]: behind the origin
    _ray("away", (20, .5, .5), (1, .5, .25), 0, 40, 0, 0),
    # enters at t = 4, leaves at 36: 32 / 0.25 = 128, 32 / 0.5 = 64
    _ray("axis_128", (-20, .5, .5), (1, 0, 0), 0, 40, 128, 64),
    # d[1] == 0 and o[1] = -16.125 < lo[1]: 1/8 outside the face "lo_face" slides along
    _ray("eighth_outside", (.5, -16.125, -20), (-0.0, 0, 1), 0, 40, 0, 0),
    # [4, min(36, t_max = 20)]: 16 / 0.25 = 64, 16 / 0.5 = 32
    _ray("axis_64", (-20, -.5, 2.5), (1, 0, 0), 0, 20, 64, 32),
    # x slab [-8, 56]; [near = 0.5, min(far = 64, t_max = 100, 56)]: 55.5 / 0.25 = 222, 55.5 / 0.5 = 111
    _ray("long_222", (-12, 1.5, -2.5), (.5, 0, 0), 0, 100, 222, 111),
    # d[0] == 0, o[0] == hi[0] = 16: u = 1, floor(8) = 8 clamps to 7.  [4, t_max = 12]: 32, 16
    _ray("hi_face", (16, -20, .5), (0, 1, 0), 0, 12, 32, 16),
    # x slab [2, 34], y and z slabs [-30, 2]: t_near == t_far == 2, the corner (-16, -16, -16) alone
    _ray("corner", (-18, -14, -14), (1, -1, -1), 0, 40, 0, 0),
    # d[0] = -0.0, d[1] == 0 and o[1] == lo[1] = -16.  z slab [4, 36]; [t_min = 30, 36]: 6 / 0.25 = 24, 12
    _ray("lo_face", (.5, -16, -20), (-0.0, 0, 1), 30, 40, 24, 12),
    # x == 4: on the hi face of level 0's box while |y| <= 4 (level 0, cell 8 -> 7), on a cell face of level 1 and 2 beyond.
    # [t_min = 14, 36]: 22 / 0.25 = 88, 44
    _ray("inner_hi_face", (4, -20, .5), (0, 1, 0), 14, 40, 88, 44),
    # y == 8: on the hi face of level 1's box while |z| <= 8 (level 1, cell 8 -> 7), in level 2 beyond.  z slab [4, 36];
    # [t_min = 10, t_max = 30]: 80, 40
    _ray("l1_hi_face", (.5, 8, -20), (0, 0, 1), 10, 30, 80, 40),
    # x == -8, d[0] = -0.0: on the lo face of level 1's box throughout (cell 0).  y slab [4, 36]; [12, 28]: 64, 32
    _ray("l1_lo_face", (-8, -20, 1.5), (-0.0, 1, 0), 12, 28, 64, 32),
    # origin in level 0.  x slab [-33, 31], y [-58, 70], z [-13.5, 18.5]; t_rand = 0.5: near = 0.5 + 0.5 * step.
    # step 0.25: 17.875 / 0.25 = 71.5 -> 72; step 0.5: 17.75 / 0.5 = 35.5 -> 36.  The last one is cut: t_end == t_far = 18.5
    _ray("inside_l0", (.5, -1.5, 2.5), (.5, .25, -1), 0, 40, 72, 36, t_rand=.5),
    # origin in level 1 only (x = 6.5).  x slab [-9.5, 22.5], y [-21, 43]: [0.5, 22.5]: 88, 44
    _ray("inside_l1", (6.5, -5.5, .5), (-1, .5, 0), 0, 40, 88, 44),
    # origin outside every box.  x and y slabs [4, 36]; [4, t_max = 10]: 24, 12
    _ray("outside_all", (-20, -20, 3.5), (1, 1, 0), 0, 10, 24, 12),
    # t_min = 0.125 < near_plane: [0.5, t_max = 8]: 30, 15
    _ray("t_min_below_near", (.5, .5, -2.5), (0, 0, 1), .125, 8, 30, 15),
    # t_min = 3.125 > near_plane: 4.875 / 0.25 = 19.5 -> 20, 9.75 -> 10; the last one is cut
    _ray("t_min_above_near", (.5, .5, -2.5), (0, 0, 1), 3.125, 8, 20, 10),
    # t_max = 100 > far_plane; x slab [-2, 126]: [t_min = 56, far = 64]: 32, 16
    _ray("t_max_beyond_far", (-15.5, .5, .5), (.25, 0, 0), 56, 100, 32, 16),
    # t_max = 5 < t_min = 10
    _ray("t_max_below_t_min", (.5, .5, .5), (1, 0, 0), 10, 5, 0, 0),
    # [2, 5.125]: 3.125 / 0.25 = 12.5 -> 13, 6.25 -> 7; the last candidate has t_end == t_far = 5.125
    _ray("cut_by_t_far", (-2.5, 1.5, .5), (1, 0, 0), 2, 5.125, 13, 7),
]
# the last of the 61 rays: y slab [-36, -4], behind the origin
DESIGNED_TAIL = [_ray("away_last", (.5, 20, .5), (0, 1, .25), 0, 40, 0, 0)]
N_RAYS = 61


@functools.lru_cache(maxsize=None)
def dyadic_rays(seed=11):
    """-> dict of fp32 arrays o [61,3], d [61,3], t_min, t_max, t_rand [61] and names (None for a drawn ray): the designed
    rays first -- empty, non-empty, empty, non-empty, non-empty, ... -- then the seeded draw, then one more empty ray"""
    rng = np.random.default_rng(seed)
    n_draw = N_RAYS - len(DESIGNED_HEAD) - len(DESIGNED_TAIL)
    drawn = []
    for _ in range(n_draw):
        half = (4, 8, 16, 20)[rng.integers(4)]  # origins in level 0, in level 1, in level 2, some outside every box
        o = rng.integers(-8 * half, 8 * half + 1, 3) / 8.0
        d = np.zeros(3)
        while not np.any(d != 0):
            d = np.asarray(DIR_COMPONENTS)[rng.integers(len(DIR_COMPONENTS), size=3)]
        drawn.append(dict(name=None, o=o, d=d, t_min=rng.integers(0, 33) / 8.0, t_max=rng.integers(16, 401) / 8.0,
                          t_rand=T_RANDS[rng.integers(len(T_RANDS))]))
    rays = DESIGNED_HEAD + drawn + DESIGNED_TAIL
    out = {k: np.array([r[k] for r in rays], f32) for k in ("o", "d", "t_min", "t_max", "t_rand")}
    out["names"] = [r["name"] for r in rays]
    return out


# ---- cone scenes: cone = 2^-6, step 0.25 (step / cone = 16), near_plane 0, no far plane.  The rays start inside level 2 and
# enter at t_near = t_min; the uniform part has k1 = ceil((16 - t_near) / 0.25) candidates, whose t are exact.  The origins sit
# 3/1024 off the lattice, so that no midpoint of the uniform part lies within 1e-4 cells of a face --------------------------
CONE, CONE_STEP = 2.0 ** -6, 0.25
_OFF = 3.0 / 1024.0
CONE_RAYS = [
    # (o, d, t_near = t_min, t_max, k1)
    ((20, .5, .5), (1, .5, .25), 0.0, 64.0, None),                      # points away: no samples, in the first slot
    ((-15.5, -3.5, .5), (.125, .0625, 0), 2.0, 64.0, 56),               # the cone takes over inside chunk 0
    ((-15.5, 3.5, -2.5), (.125, -.0625, .03125), 0.0, 64.0, 64),        # exactly at the chunk boundary
    ((15.5, -1.5, 1.5), (-.125, .03125, -.0625), 0.25, 64.0, 63),       # one before it
    ((-15.5, -7.5, 6.5), (.125, .0625, -.0625), 16.0, 160.0, 0),        # t_near * cone == step: cone from the start
    ((15.5, 9.5, -10.5), (-.125, -.0625, .0625), 20.0, 200.0, 0),       # t_near * cone > step: the same
]


@functools.lru_cache(maxsize=None)
def cone_rays():
    o = np.array([np.asarray(r[0], f64) + (_OFF if r[4] is not None else 0.0) for r in CONE_RAYS], f32)
    return dict(o=o, d=np.array([r[1] for r in CONE_RAYS], f32), t_min=np.array([r[2] for r in CONE_RAYS], f32),
                t_max=np.array([r[3] for r in CONE_RAYS], f32), k1=[r[4] for r in CONE_RAYS])


def cone_tolerance():
    """the three-level test's bound on t: 4 * 2^-23 * t_far, there for powf (here t_far is at most 200)"""
    return 4 * 2.0 ** -23 * float(max(r[3] for r in CONE_RAYS))


# ---- the float64 reference -------------------------------------------------------------------------------------------------
def march64(aabbs, res, origins, dirs, step, near_plane=0.0, far_plane=1e10, t_min=None, t_max=None, t_rand=None,
            cone_angle=0.0, max_candidates=1 << 16, margin=None, broken=None):
    """Every candidate interval of every ray, in order, in float64 (python floats) on the fp32 inputs.
    ``broken``: the rule with one line changed (MUTATIONS), for the host test that shows the scenes tell the two apart.
    -> dict: ray, k int64 [n]; t_start, t_end float64 [n]; level int64 [n]; cell int64 [n] (flat index in its level);
       on_cell_face bool [n]: the midpoint lies exactly on a face of its level's cell lattice; on_box_face bool [n, L]: it
       lies exactly on the surface of level l's box; ambiguous bool [n] (``margin`` given): the midpoint is within ``margin``
       of a cell face of its level or of some level's box face, in cells, as march_levels of the restatement defines it;
       k1 [R] (None where the ray misses), t_near, t_far [R] (nan where it misses)"""
    aabbs = np.asarray(aabbs, f32).reshape(-1, 6)
    L = aabbs.shape[0]
    lo = [[float(v) for v in b[:3]] for b in aabbs]
    hi = [[float(v) for v in b[3:]] for b in aabbs]
    step, cone = float(f32(step)), float(f32(cone_angle))
    R = origins.shape[0]
    cols = dict(ray=[], k=[], t_start=[], t_end=[], level=[], cell=[], on_cell_face=[], on_box_face=[], ambiguous=[])
    k1s, t_nears, t_fars = [None] * R, [math.nan] * R, [math.nan] * R
    for r in range(R):
        o = [float(v) for v in np.asarray(origins[r], f32)]
        d = [float(v) for v in np.asarray(dirs[r], f32)]
        near = max(float(f32(near_plane)), float(f32(t_min[r]))) if t_min is not None else float(f32(near_plane))
        far = min(float(f32(far_plane)), float(f32(t_max[r]))) if t_max is not None else float(f32(far_plane))
        if t_rand is not None:
            near += float(f32(t_rand[r])) * step
        tn, tf, miss = near, far, False
        for a in range(3):  # the slab clip against the outermost box
            if d[a] == 0.0:  # -0.0 too: the ray runs in the plane o[a]; closed test
                miss |= o[a] < lo[-1][a] or (o[a] >= hi[-1][a] if broken == "open_hi_slab" else o[a] > hi[-1][a])
                continue
            ta, tb = (lo[-1][a] - o[a]) / d[a], (hi[-1][a] - o[a]) / d[a]
            tn, tf = max(tn, min(ta, tb)), min(tf, max(ta, tb))
        if miss or not tn < tf:
            continue
        k1, t1 = 0, tn
        if cone > 0.0 and tn * cone < step:
            k1 = int(math.ceil((step / cone - tn) / step))
            t1 = tn + k1 * step
        k1s[r], t_nears[r], t_fars[r] = k1, tn, tf

        def at(k):
            return tn + k * step if cone <= 0.0 or k < k1 else t1 * (1.0 + cone) ** (k - k1)

        for k in range(max_candidates):
            ts = at(k)
            if not ts < tf:
                break
            te = min(at(k + 1), tf)
            if not te > ts:
                continue
            tm = 0.5 * (ts + te)
            p = [o[a] + d[a] * tm for a in range(3)]
            inside = [all(lo[l][a] <= p[a] <= hi[l][a] for a in range(3)) for l in range(L)]
            lvl = next((l for l in range(L - 1) if inside[l]), L - 1)  # the first closed box; the outermost when none
            if broken == "open_level_box_hi":  # p <= hi to p < hi
                lvl = next((l for l in range(L - 1) if all(lo[l][a] <= p[a] < hi[l][a] for a in range(3))), L - 1)
            if broken == "open_level_box_lo":  # p >= lo to p > lo
                lvl = next((l for l in range(L - 1) if all(lo[l][a] < p[a] <= hi[l][a] for a in range(3))), L - 1)
            g = [(p[a] - lo[lvl][a]) / (hi[lvl][a] - lo[lvl][a]) * res for a in range(3)]
            idx = [min(max(int(math.floor(v)), 0), res - 1) for v in g]
            if broken == "no_clamp":  # the flat index then points into a neighbouring row, level or past the array
                idx = [int(math.floor(v)) for v in g]
            cols["ray"].append(r), cols["k"].append(k), cols["t_start"].append(ts), cols["t_end"].append(te)
            cols["level"].append(lvl), cols["cell"].append((idx[0] * res + idx[1]) * res + idx[2])
            cols["on_cell_face"].append(any(v == math.floor(v) for v in g))
            cols["on_box_face"].append([inside[l] and any(p[a] == lo[l][a] or p[a] == hi[l][a] for a in range(3))
                                        for l in range(L)])
            if margin is not None:
                amb = any(abs(v - round(v)) < margin for v in g)
                for l in range(L):
                    cl = [(hi[l][a] - lo[l][a]) / res for a in range(3)]
                    amb |= any(abs(p[a] - lo[l][a]) / cl[a] < margin or abs(p[a] - hi[l][a]) / cl[a] < margin
                               for a in range(3))
                cols["ambiguous"].append(amb)
    n = len(cols["ray"])
    out = dict(ray=np.asarray(cols["ray"], np.int64), k=np.asarray(cols["k"], np.int64),
               t_start=np.asarray(cols["t_start"], f64), t_end=np.asarray(cols["t_end"], f64),
               level=np.asarray(cols["level"], np.int64), cell=np.asarray(cols["cell"], np.int64),
               on_cell_face=np.asarray(cols["on_cell_face"], bool),
               on_box_face=np.asarray(cols["on_box_face"], bool).reshape(n, L), k1=k1s,
               t_near=np.asarray(t_nears, f64), t_far=np.asarray(t_fars, f64), n_rays=R)
    if margin is not None:
        out["ambiguous"] = np.asarray(cols["ambiguous"], bool)
    return out


PER_CANDIDATE = ("ray", "k", "t_start", "t_end", "level", "cell", "on_cell_face", "on_box_face", "ambiguous")


MUTATIONS = ("open_level_box_hi", "open_level_box_lo", "no_clamp", "open_hi_slab")  # and the missing k < max_candidates: expected(chunked=True)


def keep(ref, binaries):
    """bool [n]: the candidates whose cell is set.  binaries [L, res, res, res] (or [res, res, res] at one level)"""
    b = np.asarray(binaries).astype(bool)
    b = b.reshape(-1, b.shape[-1] ** 3)
    return b[ref["level"], ref["cell"]]


def keep_unclamped(ref, binaries):
    """(keep bool [n], readable bool [n]) of a reference made with broken="no_clamp": the byte the flat index
    level * res^3 + cell points at, wherever that is in the array; not readable when it points outside it"""
    b = np.asarray(binaries).astype(bool).reshape(-1)
    flat = ref["level"] * (np.asarray(binaries).shape[-1] ** 3) + ref["cell"]
    ok = (flat >= 0) & (flat < len(b))
    return b[np.clip(flat, 0, len(b) - 1)] & ok, ok


def per_ray(ref, mask=None):
    """int64 [R]: candidates per ray (those of ``mask`` only)"""
    ray = ref["ray"] if mask is None else ref["ray"][mask]
    return np.bincount(ray, minlength=ref["n_rays"]).astype(np.int64)


def prefix(ref, n_rays):
    """the reference of the first ``n_rays`` rays alone: rays march independently"""
    m = ref["ray"] < n_rays
    out = {k: v[m] for k, v in ref.items() if k in PER_CANDIDATE}
    out.update(k1=ref["k1"][:n_rays], t_near=ref["t_near"][:n_rays], t_far=ref["t_far"][:n_rays], n_rays=n_rays)
    return out


def expected(ref, binaries, cap=None, chunked=False):
    """what the march emits: (ray_indices int64 [M], t_starts fp32 [M], t_ends fp32 [M], segments int64 [R + 1]) -- the kept
    candidates with k < cap, in order.  On the dyadic scenes the fp32 casts are exact.
    chunked: the rule broken -- the cap is only looked at once per 64 candidates, k < 64 * ceil(cap / 64)."""
    m = keep(ref, binaries)
    if cap is not None:
        m = m & (ref["k"] < (-(-cap // 64) * 64 if chunked else cap))
    seg = np.concatenate([[0], np.cumsum(per_ray(ref, m))]).astype(np.int64)
    return ref["ray"][m], ref["t_start"][m].astype(f32), ref["t_end"][m].astype(f32), seg


def ray_options(rays, with_options):
    """the per-ray t_min / t_max / t_rand (None where the scene has none), or None for all three"""
    return (rays["t_min"], rays["t_max"], rays.get("t_rand")) if with_options else (None, None, None)


@functools.lru_cache(maxsize=None)
def dyadic_reference(levels, step, with_options, broken=None):
    """march64 of the 61 rays, uncapped; computed once, shared, left unchanged"""
    rays = dyadic_rays()
    t_min, t_max, t_rand = ray_options(rays, with_options)
    return march64(level_boxes(levels), RES, rays["o"], rays["d"], step, NEAR, FAR, t_min, t_max, t_rand, broken=broken)


@functools.lru_cache(maxsize=None)
def cone_reference(levels=LEVELS, margin=1e-4):
    rays = cone_rays()
    return march64(level_boxes(levels), RES, rays["o"], rays["d"], CONE_STEP, 0.0, 1e10, rays["t_min"], rays["t_max"], None,
                   cone_angle=CONE, margin=margin)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)
