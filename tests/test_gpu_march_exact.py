"""The occupancy march (march_ray, csrc/occgrid.hip) against a float64 reference, bit for bit, on a dyadic lattice where every
fp32 intermediate is exact -- also for midpoints exactly on a cell face or a level's box face: all three entry points, t_min /
t_max / t_rand, ray counts that end in a ragged workgroup, max_candidates, what each pass writes, the cone's take-over at and
across a 64-candidate chunk, and the argument checks.  Scenes and reference: tests/march_exact_refs.py; their properties are
asserted without a GPU in tests/test_march_exact_refs_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import march_exact_refs as MX
from gpu_util import cuda, host
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ENTRIES = ("single", "levels-1", "levels-3", "actors-3")
POISON_I32 = 0x7F7F7F7F
POISON_I64 = 0x7F7F7F7F7F7F7F7F
GUARD = 64


class NoActors:
    """what ops.occgrid_march reads of an ActorSpec, for one actor nobody is a candidate of: the march reads n_actors, bounds
    and max_candidates of the descriptor and nothing else"""

    def __init__(self):
        from neurad_studio_amd import _lib

        self.bounds = torch.ones((1, 3), device="cuda")
        self.a = _lib.Actors()
        self.a.n_actors, self.a.bounds, self.a.max_candidates = 1, self.bounds.data_ptr(), 1

    def c_actors(self):
        return self.a, self.bounds

    @staticmethod
    def lists(R):
        return (torch.zeros((R,), dtype=torch.int32, device="cuda"), torch.zeros((R, 1), dtype=torch.int32, device="cuda"),
                torch.zeros((R, 1, 12), device="cuda"), None)


def levels_of(entry):
    return 3 if entry.endswith("3") else 1


def grid_for(ops, entry, kind):
    L = levels_of(entry)
    boxes, b = torch.from_numpy(MX.level_boxes(L)), cuda(MX.binaries_for(kind, L))
    return ops.OccGridSpec(boxes[0], b[0]) if entry == "single" else ops.OccGridSpec(boxes, b)


def march(ops, entry, kind, rays, R, step, opt, near=MX.NEAR, far=MX.FAR, **kw):
    t_min, t_max, t_rand = (None if v is None else cuda(v[:R]) for v in MX.ray_options(rays, opt))
    if entry.startswith("actors"):
        kw["actor_boxes"] = (NoActors(), NoActors.lists(R))
    out = ops.occgrid_march(grid_for(ops, entry, kind), cuda(rays["o"][:R]), cuda(rays["d"][:R]), step, near_plane=near,
                            far_plane=far, t_min=t_min, t_max=t_max, t_rand=t_rand, **kw)
    return tuple(host(v) for v in out)


def assert_same_samples(got, want, what=""):
    ri, ts, te, seg = got
    np.testing.assert_array_equal(seg, want[3], err_msg=f"{what}: segments")
    np.testing.assert_array_equal(ri, want[0], err_msg=f"{what}: ray_indices")
    np.testing.assert_array_equal(MX.bits(ts), MX.bits(want[1]), err_msg=f"{what}: t_starts")
    np.testing.assert_array_equal(MX.bits(te), MX.bits(want[2]), err_msg=f"{what}: t_ends")


# ---- 1. bit-for-bit equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [True, False], ids=["options", "plain"])
@pytest.mark.parametrize("step", MX.STEPS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_march_equals_the_float64_reference_bit_for_bit(ops, entry, step, opt):
    """Every ray count (each ends in a ragged workgroup) and every binaries: the emitted (ray, t_start, t_end) are the
    reference's kept candidates, same order, t as int32 bits, and so are the segments.  No tolerance, no excluded band."""
    rays, full = MX.dyadic_rays(), MX.dyadic_reference(levels_of(entry), step, opt)
    for R in MX.RAY_COUNTS:
        ref = MX.prefix(full, R)
        for kind in ("random", "ones", "zeros"):
            want = MX.expected(ref, MX.binaries_for(kind, levels_of(entry)))
            got = march(ops, entry, kind, rays, R, step, opt)
            assert_same_samples(got, want, f"R = {R}, {kind}")
            if kind == "zeros":
                assert len(got[0]) == 0
            if kind == "ones":
                assert len(got[0]) == len(ref["ray"])


# ---- 2. max_candidates -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("single", "levels-3", "actors-3"))
def test_max_candidates_counts_candidate_intervals(ops, entry):
    """The emitted samples are exactly the kept candidates with k < max_candidates of the uncapped reference; on the all-one
    grid a ray has min(n_candidates, cap) samples.

    On the kernel before the cap was tested per candidate (a cap was only looked at once per 64 candidates) this failed at
    every cap that is no multiple of 64: on the all-one grid the per-ray counts were min(n, 64 * ceil(cap / 64))."""
    rays, ref = MX.dyadic_rays(), MX.dyadic_reference(levels_of(entry), 0.25, True)
    n = MX.per_ray(ref)
    failed = []
    for kind in ("ones", "random"):
        for cap in MX.CAPS:
            want = MX.expected(ref, MX.binaries_for(kind, levels_of(entry)), cap)
            got = march(ops, entry, kind, rays, MX.N_RAYS, 0.25, True, max_candidates=cap)
            counts = np.diff(got[3])
            print(f"{entry} {kind} cap {cap}: {len(got[0])} samples, expected {len(want[0])}; largest per-ray count "
                  f"{counts.max()}")
            if kind == "ones":
                np.testing.assert_array_equal(np.diff(want[3]), np.minimum(n, cap))
            if not np.array_equal(counts, np.diff(want[3])):
                failed.append((kind, cap, int(counts.max()), len(got[0]), len(want[0])))
                continue
            assert_same_samples(got, want, f"{kind}, cap {cap}")
    assert not failed, f"(binaries, cap, largest per-ray count, samples, expected samples): {failed}"


@pytest.mark.parametrize("entry", ("levels-3", "actors-3"))
def test_max_candidates_on_the_cone_scene(ops, entry):
    """counts and order exact -- the cap falls before, at and after k1 and the chunk seams -- t within the cone bound"""
    rays, ref = MX.cone_rays(), MX.cone_reference()
    R, tol = len(rays["k1"]), MX.cone_tolerance()
    for cap in MX.CAPS:
        want = MX.expected(ref, MX.binaries_for("ones", 3), cap)
        ri, ts, te, seg = march(ops, entry, "ones", rays, R, MX.CONE_STEP, True, near=0.0, far=1e10, cone_angle=MX.CONE,
                                max_candidates=cap)
        np.testing.assert_array_equal(seg, want[3], err_msg=f"cap {cap}")
        np.testing.assert_array_equal(ri, want[0])
        capped = ref["k"] < cap
        assert np.abs(ts - ref["t_start"][capped]).max() <= tol and np.abs(te - ref["t_end"][capped]).max() <= tol


# ---- 3. what each pass writes --------------------------------------------------------------------------------------------------
def two_passes(ops, entry, kind, rays, R, step, opt):
    """the count and the write pass through ops.launch, into poisoned buffers with GUARD elements on each side
    -> (counts [R + 2 GUARD] int32, seg [R + 1], ray_indices [M + 2 GUARD] int64, t_starts, t_ends as int32 bits)"""
    t_min, t_max, t_rand = (None if v is None else cuda(v[:R]) for v in MX.ray_options(rays, opt))
    o, d = cuda(rays["o"][:R]), cuda(rays["d"][:R])
    spec = grid_for(ops, entry, kind)
    if entry == "single":
        (g, keep), name, head = spec.c_grid(), "nrhip_occgrid_march", ()
    else:
        (g, keep), name, head = spec.c_levels(), "nrhip_occgrid_march_levels", ()
    if entry.startswith("actors"):
        none = NoActors()
        name, head = "nrhip_occgrid_march_levels_actors", (none.a, *NoActors.lists(R)[:3])
    args = (g, *head, o, d, t_min, t_max, t_rand, R, step, MX.NEAR, MX.FAR, 0.0, 1 << 16)
    counts = torch.full((R + 2 * GUARD,), POISON_I32, dtype=torch.int32, device="cuda")
    ops.launch(name, *args, counts[GUARD:GUARD + R], None, None, None, None)
    seg = torch.zeros((R + 1,), dtype=torch.int64, device="cuda")
    torch.cumsum(counts[GUARD:GUARD + R], 0, out=seg[1:])
    M = int(seg[-1])
    ri = torch.full((M + 2 * GUARD,), POISON_I64, dtype=torch.int64, device="cuda")
    ts = torch.full((M + 2 * GUARD,), POISON_I32, dtype=torch.int32, device="cuda")
    te = torch.full((M + 2 * GUARD,), POISON_I32, dtype=torch.int32, device="cuda")
    ops.launch(name, *args, None, seg, ri[GUARD:], ts[GUARD:].view(torch.float32), te[GUARD:].view(torch.float32))
    torch.cuda.synchronize()
    return host(counts), host(seg), host(ri), host(ts), host(te)


@pytest.mark.parametrize("R", MX.RAY_COUNTS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_each_pass_writes_its_entries_and_nothing_else(ops, entry, R):
    """Count pass: every one of the R counts is written, zero for a ray that misses the box, is clipped away or keeps nothing;
    write pass: exactly seg[-1] entries of each output; the guards on both sides of every buffer stay as they were.  Twice
    into fresh buffers: identical."""
    rays, ref = MX.dyadic_rays(), MX.prefix(MX.dyadic_reference(levels_of(entry), 0.25, True), R)
    want = MX.expected(ref, MX.binaries_for("random", levels_of(entry)))
    runs = [two_passes(ops, entry, "random", rays, R, 0.25, True) for _ in range(2)]
    counts, seg, ri, ts, te = runs[0]
    M = int(want[3][-1])
    assert np.all(counts[:GUARD] == POISON_I32) and np.all(counts[GUARD + R:] == POISON_I32)
    np.testing.assert_array_equal(counts[GUARD:GUARD + R], np.diff(want[3]))
    assert (np.diff(want[3]) == 0).any()
    np.testing.assert_array_equal(seg, want[3])
    assert len(ri) == M + 2 * GUARD
    for buf, poison in ((ri, POISON_I64), (ts, POISON_I32), (te, POISON_I32)):
        assert np.all(buf[:GUARD] == poison) and np.all(buf[GUARD + M:] == poison)
        assert not np.any(buf[GUARD:GUARD + M] == poison)
    np.testing.assert_array_equal(ri[GUARD:GUARD + M], want[0])
    np.testing.assert_array_equal(ts[GUARD:GUARD + M], MX.bits(want[1]))
    np.testing.assert_array_equal(te[GUARD:GUARD + M], MX.bits(want[2]))
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)


# ---- 4. the cone's take-over ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ones", "random"])
@pytest.mark.parametrize("entry", ("levels-3", "actors-3"))
def test_cone_takes_over_inside_at_and_across_a_chunk(ops, entry, kind):
    """k1 = 56 (inside chunk 0), 64 (the chunk boundary), 63 and 0.  Each emitted sample is matched to the reference candidate
    with the nearest t_start: indices strictly increasing, |t - t_ref| <= 4 * 2^-23 * t_far (there for powf), equal bits for
    k < k1 (that part is uniform), keep decisions exact outside the ambiguous band, and intervals tile back to back --
    t_end of candidate k and t_start of candidate k + 1 are the same bits -- across the k1 seam and the chunk seams."""
    rays, ref = MX.cone_rays(), MX.cone_reference()
    R, tol = len(rays["k1"]), MX.cone_tolerance()
    ri, ts, te, seg = march(ops, entry, kind, rays, R, MX.CONE_STEP, True, near=0.0, far=1e10, cone_angle=MX.CONE)
    assert np.all(np.diff(ri) >= 0) and seg[-1] == len(ri) and np.array_equal(np.diff(seg), np.bincount(ri, minlength=R))
    emitted = np.zeros(len(ref["ray"]), bool)
    first = np.searchsorted(ref["ray"], np.arange(R + 1))
    seams = 0
    for r in range(R):
        mine, cand = ri == r, slice(first[r], first[r + 1])
        if not mine.any():
            continue
        assert first[r + 1] > first[r], f"ray {r}: samples from a ray the reference never marches"
        k = np.abs(ts[mine][:, None] - ref["t_start"][cand][None]).argmin(1)
        assert np.all(np.diff(k) > 0)
        assert np.abs(ts[mine] - ref["t_start"][cand][k]).max() <= tol and np.abs(te[mine] - ref["t_end"][cand][k]).max() <= tol
        uniform = k < ref["k1"][r]
        np.testing.assert_array_equal(MX.bits(ts[mine][uniform]), MX.bits(ref["t_start"][cand][k][uniform].astype(np.float32)))
        np.testing.assert_array_equal(MX.bits(te[mine][uniform]), MX.bits(ref["t_end"][cand][k][uniform].astype(np.float32)))
        both = np.diff(k) == 1  # candidates k and k + 1 both emitted
        np.testing.assert_array_equal(MX.bits(te[mine][:-1][both]), MX.bits(ts[mine][1:][both]))
        seams += sum(int(((k[:-1] == s - 1) & both).sum()) for s in {ref["k1"][r], 64, 128} if s > 0)
        emitted[first[r] + k] = True
    sure = ~ref["ambiguous"]
    np.testing.assert_array_equal(emitted[sure], MX.keep(ref, MX.binaries_for(kind, 3))[sure])
    if kind == "ones":
        assert emitted.all() and seams == 3 + 2 + 3 + 2 + 2  # k1 = 56, 64 (k1 IS the chunk seam), 63, 0, 0; chunks at 64, 128
    else:
        assert seams >= 2


# ---- 5. argument edges ---------------------------------------------------------------------------------------------------------
def test_argument_edges_return_before_any_launch(ops):
    """r == 0 is OK and reads nothing (every pointer NULL or unmapped); a bad step, cone or cap and a write pass with a NULL
    output are NRHIP_ERR_INVALID_ARG (code 1) with a message, and nothing is launched: the poisoned outputs stay as they were."""
    from neurad_studio_amd import _lib

    rays, R = MX.dyadic_rays(), 5
    o, d = cuda(rays["o"][:R]), cuda(rays["d"][:R])
    g, keep = grid_for(ops, "levels-3", "ones").c_levels()
    g1, keep1 = grid_for(ops, "single", "ones").c_grid()
    stream = torch.cuda.current_stream().cuda_stream
    counts = torch.full((R,), POISON_I32, dtype=torch.int32, device="cuda")
    seg = torch.zeros((R + 1,), dtype=torch.int64, device="cuda")
    ri = torch.full((4096,), POISON_I64, dtype=torch.int64, device="cuda")
    ts = torch.full((4096,), POISON_I32, dtype=torch.int32, device="cuda")
    te = torch.full((4096,), POISON_I32, dtype=torch.int32, device="cuda")
    ref = ctypes.byref

    def call(name, grid, r=R, step=0.25, cone=0.0, cap=1 << 16, count_pass=True, outputs=(ri, ts, te), rays=(o, d)):
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        tail = (ptr(counts), None, None, None, None) if count_pass else (None, ptr(seg), *(ptr(t) for t in outputs))
        _lib.call(name, ref(grid), ptr(rays[0]), ptr(rays[1]), None, None, None, r, step, MX.NEAR, MX.FAR, cone, cap, *tail,
                  stream)

    unmapped = ctypes.c_void_p(0x1000)
    for name, grid in (("nrhip_occgrid_march", g1), ("nrhip_occgrid_march_levels", g)):
        _lib.call(name, ref(grid), unmapped, unmapped, unmapped, unmapped, unmapped, 0, 0.25, MX.NEAR, MX.FAR, 0.0, 1 << 16,
                  unmapped, None, None, None, None, stream)  # r == 0, the count pass
        _lib.call(name, ref(grid), None, None, None, None, None, 0, 0.25, MX.NEAR, MX.FAR, 0.0, 1 << 16, None, unmapped,
                  unmapped, unmapped, unmapped, stream)      # r == 0, the write pass
        for count_pass in (True, False):
            for bad in (dict(step=0.0), dict(step=-0.25), dict(cone=-2.0 ** -6), dict(cap=0), dict(cap=-1)):
                with pytest.raises(_lib.NeuradHipError, match=r"code 1\): occgrid_march: bad argument"):
                    call(name, grid, count_pass=count_pass, **bad)
        for missing in range(3):
            outputs = tuple(None if i == missing else t for i, t in enumerate((ri, ts, te)))
            with pytest.raises(_lib.NeuradHipError, match=r"code 1\): occgrid_march: write pass needs outputs"):
                call(name, grid, count_pass=False, outputs=outputs)
        with pytest.raises(_lib.NeuradHipError, match=r"code 1\): occgrid_march: null rays"):
            call(name, grid, rays=(o, None))
    torch.cuda.synchronize()
    assert torch.all(counts == POISON_I32) and torch.all(ri == POISON_I64)
    assert torch.all(ts == POISON_I32) and torch.all(te == POISON_I32)
    call("nrhip_occgrid_march_levels", g)  # the same arguments, unbroken: the counts are written
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(counts), MX.per_ray(MX.prefix(MX.dyadic_reference(3, 0.25, False), R)))
