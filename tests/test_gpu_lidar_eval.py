"""csrc/lidar_eval.hip on the GPU: nrhip_nearest_sq_dist per element against the float64 restatement
(tests/lidar_eval_refs.py: the bounds U6 / U8 and their derivation) at every size where the kernel takes another path (one
point, around a wavefront, around the LDS tile, several tiles), under every launch plan, row stride and mask; bitwise
reproducibility across runs, plans and permutations; the chamfer sum; NaN containment; capture in a HIP graph."""
import numpy as np
import pytest
import torch

import lidar_eval_refs as R
import synth
from conftest import load_golden
from gpu_util import cuda, host, ops  # noqa: F401

pytestmark = pytest.mark.gpu

TILE = 1024
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
PLANS = [(q, s) for s in (1, 2, 3) for q in (1, 2, 4)]  # each Q, without and with the target split (even and uneven runs)
NMAX = SIZES[-1]
_refs = {}


def pool():
    """NMAX targets inside +-80 x +-80 x +-4 m and NMAX queries a few decimetres from (other) targets"""
    t = np.stack([synth.uniform((NMAX,), -80, 80, 701), synth.uniform((NMAX,), -80, 80, 702),
                  synth.uniform((NMAX,), -4, 4, 703)], -1)
    q = (t[(np.arange(NMAX) * 7 + 3) % NMAX] + 0.3 * synth.normal((NMAX, 3), 704)).astype(np.float32)
    return q, t.astype(np.float32)


def mask(kind, n, seed):
    if kind == "absent":
        return None
    if kind == "all_true":
        return np.ones(n, bool)
    if kind == "all_false":
        return np.zeros(n, bool)
    return synth.uniform((n,), 0, 1, seed) < 0.6


def reference(n, m, kind):
    """computed once per (N, M, masks) and shared: strides and plans do not change the values"""
    key = (n, m, kind)
    if key not in _refs:
        q, t = pool()
        _refs[key] = R.nearest_sq_dist(q[:n], t[:m], mask(kind, n, 11), mask(kind, m, 12))
        _refs[key].setflags(write=False)
    return _refs[key]


def strided(points, stride):
    """[n, stride] storage whose first three columns are the points, the others NaN (never read as coordinates)"""
    buf = np.full((len(points), stride), np.nan, np.float32)
    buf[:, :3] = points
    return cuda(buf)


def nearest_into(ops, q, sq, qv, t, st, tv, plan):
    """the entry point itself, on an output prefilled with NaN"""
    n, m = q.shape[0], t.shape[0]
    out = torch.full((n,), float("nan"), device="cuda")
    ops.launch("nrhip_nearest_sq_dist", q, sq, qv, n, t, st, tv, m, ops._nearest_plan_arg(plan), out)
    return out


def check_per_element(got, want, what):
    got = host(got).astype(np.float64)
    assert not np.isnan(got).any(), what
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(got), ~fin), what
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= R.U6 * want[fin]), (what, float((err / np.maximum(want[fin], 1e-300)).max() / R.U))


@pytest.mark.parametrize("stride", [3, 4, 5])
@pytest.mark.parametrize("kind", ["absent", "all_true", "mixed", "all_false"])
def test_nearest_per_element_at_every_size_plan_stride_and_mask(ops, kind, stride):
    q, t = pool()
    qd, td = strided(q, stride), strided(t, stride)
    for n in SIZES:
        qv = mask(kind, n, 11)
        qv_d = None if qv is None else cuda(qv.astype(np.uint8))
        for m in SIZES:
            tv = mask(kind, m, 12)
            tv_d = None if tv is None else cuda(tv.astype(np.uint8))
            want = reference(n, m, kind)
            first = None
            for plan in PLANS + [None]:
                got = nearest_into(ops, qd[:n], stride, qv_d, td[:m], stride, tv_d, plan)
                if first is None:
                    first = got
                    check_per_element(got, want, (n, m, kind, stride, plan))
                else:  # every plan: the same bits
                    assert torch.equal(got, first), (n, m, kind, stride, plan)
            if qv is not None:
                assert bool((first[cuda(~qv)] == 0).all())  # an invalid query: 0, written


def test_wrapper_takes_strided_views_without_a_copy(ops):
    q, t = pool()
    scan = strided(t[:1500], 5)           # an [N,5] scan: xyz, intensity, time
    homog = strided(q[:1300], 4)          # homogeneous [N,4] points
    got = ops.nearest_sq_dist(homog, scan[:, :3])
    assert torch.equal(got, ops.nearest_sq_dist(cuda(q[:1300]), cuda(t[:1500])))
    check_per_element(got, reference_plain(q[:1300], t[:1500]), "views")
    v = cuda(np.arange(1500) % 2 == 0)    # bool masks go in as they are
    assert torch.equal(ops.nearest_sq_dist(homog, scan, target_valid=v), ops.nearest_sq_dist(homog, scan[::2]))


def reference_plain(q, t):
    return R.nearest_sq_dist(q, t)


def test_reproducible_across_runs_plans_and_permutations(ops):
    q, t = pool()
    n, m = 1500, 2051
    qd, td = cuda(q[:n]), cuda(t[:m])
    qv, tv = cuda(mask("mixed", n, 21)), cuda(mask("mixed", m, 22))
    base = ops.nearest_sq_dist(qd, td, qv, tv)
    for _ in range(3):
        assert torch.equal(ops.nearest_sq_dist(qd, td, qv, tv), base)
    for plan in PLANS:
        assert torch.equal(ops.nearest_sq_dist(qd, td, qv, tv, plan=plan), base), plan
    pt = torch.from_numpy(np.argsort(synth.uniform((m,), 0, 1, 23))).cuda()
    assert torch.equal(ops.nearest_sq_dist(qd, td[pt], qv, tv[pt]), base)  # a minimum does not depend on the order
    pq = torch.from_numpy(np.argsort(synth.uniform((n,), 0, 1, 24))).cuda()
    assert torch.equal(ops.nearest_sq_dist(qd[pq], td, qv[pq], tv), base[pq])  # the values go with their queries
    value = [ops.chamfer_distance(qd, td, qv, tv, True, plan=p) for p in [None] + PLANS]
    assert all(torch.equal(v, value[0]) for v in value)  # the same terms in the same fixed order: the same sum


@pytest.mark.parametrize("normalize", [False, True])
def test_chamfer_sum_on_the_fixture_scan(ops, normalize):
    g = load_golden("lidar_eval")
    for case in ("ray_drop", "distance"):
        depth, logits, mult = R.case_inputs(g, case)
        pred_ret = (logits.reshape(-1) < 0) if mult > 0 else depth.reshape(-1) < np.float32(R.NON_RETURN_DISTANCE)
        want = R.chamfer(g["pred_points"], g["points"], pred_ret, g["did_return"], normalize)
        src, tgt = cuda(g["pred_points"]), cuda(g["points"])
        got, ds, dt = ops.chamfer_distance(src, tgt, cuda(pred_ret), cuda(g["did_return"]), normalize, return_per_point=True)
        assert got.shape == () and got.dtype == torch.float32 and got.is_cuda
        assert abs(float(got) - want) <= R.U8 * want, (case, float(got), want, abs(float(got) - want) / want / R.U)
        check_per_element(ds, R.nearest_sq_dist(g["pred_points"], g["points"], pred_ret, g["did_return"]), case)
        check_per_element(dt, R.nearest_sq_dist(g["points"], g["pred_points"], g["did_return"], pred_ret), case)
        assert torch.equal(ops.chamfer_distance(src, tgt, cuda(pred_ret), cuda(g["did_return"]), normalize), got)
        if normalize and case == "ray_drop":  # the masked op == the op on the gathered sets, and the drop-in metric
            from neurad_studio_amd.model_components.lidar_metrics import chamfer_distance

            gathered = chamfer_distance(src[cuda(pred_ret)], tgt[cuda(g["did_return"]), :3], 1_000, True)
            assert abs(float(gathered) - want) <= R.U8 * want


@pytest.mark.parametrize("case", R.CASES)
def test_lidar_eval_metrics_match_the_restatement_with_one_transfer(ops, case):
    """model_components/lidar_metrics.py:lidar_eval_metrics (what the plugin's get_image_metrics_and_images runs with
    fused_lidar_eval) on the fixture's scan in its three cases, against the recorded float64 restatement: ray_drop_accuracy
    exact, the others at 1e-4 relative; one call of the transfer point, and nothing before it synchronises (as far as
    torch's sync debug mode sees)"""
    from neurad_studio_amd.model_components import lidar_metrics as LM

    g = load_golden("lidar_eval")
    depth, logits, mult = R.case_inputs(g, case)
    homog = np.concatenate([g["pred_points"], np.ones((len(depth), 1), np.float32)], -1)  # [n,4], as a 4 x 4 pose gives
    outputs = {"depth": cuda(depth), "intensity": cuda(g["intensity"]), "ray_drop_logits": cuda(logits), "points": cuda(homog)}
    scan, distance, did_return = cuda(g["points"]), cuda(g["distance"]), cuda(g["did_return"])
    transfers = []

    def to_host(values):
        torch.cuda.set_sync_debug_mode("default")
        transfers.append(tuple(values.shape))
        return LM.scalars_to_host(values)

    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = LM.lidar_eval_metrics(outputs, scan, distance, did_return, mult, R.NON_RETURN_DISTANCE, to_host=to_host)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert transfers == [(5,)] and tuple(got) == R.METRIC_KEYS == LM.LIDAR_EVAL_KEYS
    assert all(type(v) is float for v in got.values())
    for k in R.METRIC_KEYS:
        want = float(g[f"f64_{case}_{k}"])
        if k == "ray_drop_accuracy":
            assert np.float32(got[k]) == np.float32(want), (case, k, got[k], want)
        else:
            assert abs(got[k] - want) <= 1e-4 * abs(want), (case, k, got[k], want)
    if case != "fallback":  # the chamfer term itself: the kernel's sum, at the sum's own bound
        assert abs(got["chamfer_distance"] - float(g[f"f64_{case}_chamfer"])) <= R.U8 * float(g[f"f64_{case}_chamfer"])


def test_empty_sets_follow_ieee_arithmetic(ops):
    q, t = pool()
    a, b, none = cuda(q[:70]), cuda(t[:90]), torch.zeros(0, 3, device="cuda")
    off_a, off_b = torch.zeros(70, dtype=torch.bool, device="cuda"), torch.zeros(90, dtype=torch.bool, device="cuda")
    inf = float("inf")
    assert ops.nearest_sq_dist(none, b).shape == (0,)
    assert bool((ops.nearest_sq_dist(a, none) == inf).all())
    for norm in (False, True):
        assert float(ops.chamfer_distance(a, none, normalize_with_target=norm)) == inf   # inf / 0 = inf
        assert float(ops.chamfer_distance(none, b, normalize_with_target=norm)) == inf
        assert float(ops.chamfer_distance(a, b, off_a, None, norm)) == inf
        assert float(ops.chamfer_distance(a, b, None, off_b, norm)) == inf
    assert float(ops.chamfer_distance(none, none)) == 0.0
    assert np.isnan(float(ops.chamfer_distance(none, none, normalize_with_target=True)))  # 0 / 0
    assert float(ops.chamfer_distance(a, b, off_a, off_b)) == 0.0
    assert np.isnan(float(ops.chamfer_distance(a, b, off_a, off_b, True)))
    v, ds, dt = ops.chamfer_distance(a, b, off_a, None, return_per_point=True)
    assert bool((ds == 0).all()) and bool((dt == inf).all())


@pytest.mark.parametrize("plan", [None, (4, 1), (1, 3)])
def test_nan_points_stay_in_their_own_row(ops, plan):
    q, t = pool()
    n, m = 1300, 2051
    qd, td = cuda(q[:n]), cuda(t[:m])
    base = ops.nearest_sq_dist(qd, td, plan=plan)
    for col in range(3):
        bad = td.clone()
        j = 1027 + col
        bad[j, col] = float("nan")
        got = ops.nearest_sq_dist(qd, bad, plan=plan)
        keep = torch.ones(m, dtype=torch.bool, device="cuda")
        keep[j] = False
        assert torch.equal(got, ops.nearest_sq_dist(qd, td, target_valid=keep, plan=plan))  # as if the target were absent
        moved = got != base
        assert int(moved.sum()) <= 8 and bool((got[moved] > base[moved]).all())  # only the queries it was nearest to
        badq = qd.clone()
        badq[700, col] = float("nan")
        got = ops.nearest_sq_dist(badq, td, plan=plan)
        assert float(got[700]) == float("inf")
        got[700] = base[700]
        assert torch.equal(got, base)  # every other row: the same bits


def test_graph_replay_gives_the_same_bits_without_host_reads_or_allocations(ops):
    q, t = pool()
    qd, td = cuda(q[:1500]), cuda(t[:2051])
    qv, tv = cuda(mask("mixed", 1500, 21)), cuda(mask("mixed", 2051, 22))
    eager = ops.chamfer_distance(qd, td, qv, tv, True, return_per_point=True) + (ops.nearest_sq_dist(qd, td, qv, tv),)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (a device->host read or a synchronisation inside the capture is an error)
        captured = ops.chamfer_distance(qd, td, qv, tv, True, return_per_point=True) + (ops.nearest_sq_dist(qd, td, qv, tv),)
    for _ in range(2):
        for x in captured:
            x.fill_(float("nan"))
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            graph.replay()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        for a, b in zip(captured, eager):
            assert torch.equal(a, b)
