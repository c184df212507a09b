"""The optimizer kernels of csrc/adam.hip against tests/adam_refs.py, bit for bit: ops.adam_step, ops.adam_step_many and
ops.adam_step_many_dev on whole slabs (sentinels, gradients and every buffer a call must not write included) at every
branch of the launch plan -- second grid-stride passes alone and in company, the 24-per-launch batching with empties, per-
tensor step counts, mixed gradient dtypes and images, dead groups -- and ops.nonfinite_check with one poisoned element at a
time in every load of its unrolled loop, its remainder loop and its tail.  tests/test_adam_refs_host.py shows on the CPU
that these case lists tell a correct kernel from each plausible wrong one."""
import numpy as np
import pytest
import torch

import adam_refs as A
from gpu_util import ops  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- running a case ------------------------------------------------------------------------------------------------------
def _upload(slabs):
    return {k: torch.from_numpy(a).cuda() for k, a in slabs.a.items()}


def _items(c, slabs, d, steps, spoil=None):
    """the tensors of case `c` as slices of the device slabs `d`; spoil = (index, elements): that tensor's parameter is the
    view that many elements further on (off the 16-byte grid)"""
    items = []
    for k, n in enumerate(c.ns):
        s = slice(slabs.off[k], slabs.off[k] + n)
        sp = slice(s.start + spoil[1], s.stop + spoil[1]) if spoil and spoil[0] == k else s
        items.append((d["p"][sp], d["g16" if c.ghalf[k] else "g32"][s], d["m"][s], d["v"][s], steps[k],
                      d["image"][s] if c.image[k] else None))
    return items


def _step_scalars(c, start=None):
    """device step scalars holding step - 1, every other element of one tensor (the others are sentinels)"""
    t = torch.full((2 * len(c.ns) + 1,), -3.0)
    t[1::2] = torch.tensor([float(s - 1) for s in c.steps]) if start is None else torch.tensor(start)
    return t.cuda()


def _run(ops, c, route, slabs, **dev):
    """-> ({kind: array after the call}, step scalars after the call or None)"""
    d = _upload(slabs)
    h = c.hyper
    if route == "step":
        (p, g, m, v, step, image), = _items(c, slabs, d, c.steps)
        assert image is None and g.dtype == torch.float32
        ops.adam_step(p, g, m, v, step, h.lr, h.b1, h.b2, h.eps, h.wd, h.grad_scale)
        steps = None
    elif route == "many":
        ops.adam_step_many(_items(c, slabs, d, c.steps), h.lr, h.b1, h.b2, h.eps, h.wd, h.grad_scale)
        steps = None
    else:
        steps = _step_scalars(c)
        items = _items(c, slabs, d, [steps[2 * k + 1] for k in range(len(c.ns))])
        kw = dict(lr=h.lr, host_grad_scale=h.grad_scale, grad_scale=None, found_inf=torch.zeros((), device="cuda"), workspace=None)
        kw.update(dev)
        ops.adam_step_many_dev(items, kw["lr"], h.b1, h.b2, h.eps, h.wd, kw["grad_scale"], kw["found_inf"], kw["workspace"],
                               kw["host_grad_scale"])
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in d.items()}, (None if steps is None else steps.cpu().numpy())


def _assert_slabs(got, want, c, slabs, what):
    for kind in A.Slabs.KINDS:
        bad = A.mismatches(got[kind], want[kind])
        if bad.size:
            i = int(bad[0])
            k = max([j for j, o in enumerate(slabs.off) if o <= i], default=-1)
            where = f"tensor {k} (n = {c.ns[k]}) element {i - slabs.off[k]}" if k >= 0 else f"leading sentinel {i}"
            raise AssertionError(f"{c.name} / {what}: {kind} differs at {bad.size} places, first {where}: got {got[kind][i]!r} "
                                 f"({got[kind][i:i + 1].view(np.uint16 if got[kind].itemsize == 2 else np.uint32)[0]:#x}), "
                                 f"want {want[kind][i]!r}, was {slabs.a[kind][i]!r}")


def _assert_steps(steps, c, advanced=True):
    want = np.full(2 * len(c.ns) + 1, -3.0, np.float32)
    # (an empty tensor holds no slot of a launch: its count stays)
    want[1::2] = [float(s if advanced and n else s - 1) for s, n in zip(c.steps, c.ns)]
    assert np.array_equal(steps.view(np.uint32), want.view(np.uint32)), (c.name, steps, want)


def _check(ops, c, routes, **dev):
    slabs = A.Slabs(c)
    want = A.expected(c, slabs)
    for route in routes:
        got, steps = _run(ops, c, route, slabs, **dev)
        _assert_slabs(got, want, c, slabs, route)
        if route == "dev":
            _assert_steps(steps, c)
    return slabs, want


def _id(c):
    return c.name


# ---- sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.small_cases("step"), ids=_id)
def test_one_tensor_every_route_small_fp32(ops, c):
    _check(ops, c, ("step", "many", "dev"))


@pytest.mark.parametrize("c", [c for c in A.small_cases("many") if c.ghalf[0] or c.image[0]], ids=_id)
def test_one_tensor_fp16_gradient_and_image_small(ops, c):
    _check(ops, c, ("many", "dev"))


@pytest.mark.parametrize("c", A.big_cases("many"), ids=_id)
def test_second_grid_stride_pass_alone_and_in_company(ops, c):
    """the smallest lengths that take the first lane (and lane 299) through a second pass: beyond 4096 workgroups alone,
    beyond 1024 next to a second live tensor"""
    plan = A.launch_plan(c.ns)[0][-1]
    n = c.ns[-1]
    assert plan.blocks == (A.CAP_ALONE if len(c.ns) == 1 else A.CAP_SHARED)
    assert (plan.passes_first, plan.passes_last, plan.tail) == ((1, 1, 0) if n % 4 == 0 and n % 1024 == 0 else (2, 1, n % 4))
    routes = ("step", "many", "dev") if len(c.ns) == 1 and not c.ghalf[0] else ("many", "dev")
    _check(ops, c, routes)


# ---- batching ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.batch_cases(), ids=_id)
def test_batches_of_24_with_own_step_counts_mixed_dtypes_and_empties(ops, c):
    _check(ops, c, ("many", "dev"))


# ---- dead groups ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ghalf", [False, True], ids=["fp32", "fp16"])
def test_dead_group_is_skipped_only_when_every_one_of_the_twelve_is_zero(ops, ghalf):
    cases = A.dead_cases(ghalf)
    o = 4 * A.DEAD_GROUP
    for name in ["zero", "decay"] + [f"one-{f}{lane}" for f in "gmv" for lane in range(4)]:
        c = cases[name]
        slabs, want = _check(ops, c, ("many", "dev"))
        s = slice(slabs.off[0] + o, slabs.off[0] + o + 4)
        if name == "zero":  # p, m, v and the image bit-identical
            assert all(not A.mismatches(want[k][s], slabs.a[k][s]).size for k in A.Slabs.KINDS)
        elif name == "decay":  # dead rows still decay under AdamW: p * decay rounded once
            assert not A.mismatches(want["p"][s], slabs.a["p"][s] * A.case_args(c, 0).decay).size
        else:
            assert any(A.mismatches(want[k][s], slabs.a[k][s]).size for k in ("p", "m", "v"))


@pytest.mark.parametrize("ghalf", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("eps", ["eps0", "eps1e-50"])
def test_dead_elements_give_nan_in_body_and_tail_when_eps_rounds_to_zero(ops, eps, ghalf):
    """0 / 0, as the arithmetic and torch have it, wherever the element sits.  (Before the shortcut asked for eps > 0 the
    body skipped the group and only the tail wrote NaN.)"""
    c = A.dead_cases(ghalf)[eps]
    assert A.case_args(c, 0).eps == 0
    slabs, want = _check(ops, c, ("many", "dev"))
    o = slabs.off[0]
    assert np.isnan(want["p"][o + 4 * A.DEAD_GROUP:o + 4 * A.DEAD_GROUP + 4]).all() and np.isnan(want["p"][o + A.DEAD_N - 3:o + A.DEAD_N]).all()


def test_dead_elements_give_nan_through_adam_step_when_eps_rounds_to_zero(ops):
    c = A.dead_cases(False)["eps1e-50"]
    c = c._replace(image=(False,), patches=tuple(p for p in c.patches if p.field != "image"))
    _check(ops, c, ("step",))


# ---- device form ---------------------------------------------------------------------------------------------------------
def test_found_inf_leaves_every_slab_and_every_step_scalar_alone(ops):
    c = A.batch_cases()[2]  # 25 live tensors, steps 1 .. 25: the first scalar is still 0
    slabs = A.Slabs(c)
    got, steps = _run(ops, c, "dev", slabs, found_inf=torch.ones((), device="cuda"))
    _assert_slabs(got, slabs.a, c, slabs, "found_inf = 1")
    _assert_steps(steps, c, advanced=False)
    assert steps[1] == 0


def test_device_lr_with_weight_decay(ops):
    c = A.dev_lr_decay_case()
    lr = torch.tensor(c.hyper.lr, device="cuda")
    assert float(lr) == c.hyper.lr and A.case_args(c, 0).decay != 1
    _check(ops, c, ("dev",), lr=lr)
    _check(ops, c, ("many",))


def test_host_grad_scale_with_a_device_scale(ops):
    c = A.dev_scales_case()
    assert c.hyper.grad_scale == 0.5 / 1024
    _check(ops, c, ("dev",), host_grad_scale=0.5, grad_scale=torch.tensor(1024.0, device="cuda"))


def test_49_tensors_in_one_call_with_their_workspace(ops):
    c = A.batch_cases()[4]
    assert sum(n > 0 for n in c.ns) == 49 and len(A.launch_plan(c.ns)[1]) == 3
    ws = ops.adam_workspace(49, "cuda")
    _check(ops, c, ("dev",), workspace=ws)
    slabs = A.Slabs(c)
    with pytest.raises(ValueError):
        _run(ops, c, "dev", slabs, workspace=ws[:-1])


def test_device_form_equals_host_form_bit_for_bit(ops):
    c = A.batch_cases()[3]
    slabs = A.Slabs(c)
    host, _ = _run(ops, c, "many", slabs)
    dev, _ = _run(ops, c, "dev", slabs)
    for kind in A.Slabs.KINDS:
        bits = np.uint16 if host[kind].itemsize == 2 else np.uint32
        assert np.array_equal(host[kind].view(bits), dev[kind].view(bits)), kind


# ---- errors leave nothing touched ----------------------------------------------------------------------------------------
def _error_call(ops, route, spoil=None, step0=False):
    from neurad_studio_amd._lib import NeuradHipError

    c = A.error_case()
    assert len(c.ns) == 30 and all(c.ns) and A.launch_plan(c.ns)[0][27].launch == 1  # the 28th: in the second launch
    slabs = A.Slabs(c)
    d = _upload(slabs)
    h = c.hyper
    if route == "many":
        steps = list(c.steps)
        if step0:
            steps[27] = 0
        with pytest.raises(NeuradHipError):
            ops.adam_step_many(_items(c, slabs, d, steps, spoil), h.lr, h.b1, h.b2, h.eps, h.wd, h.grad_scale)
    else:
        scalars = _step_scalars(c)
        before = scalars.clone()
        with pytest.raises(NeuradHipError):
            ops.adam_step_many_dev(_items(c, slabs, d, [scalars[2 * k + 1] for k in range(30)], spoil), h.lr, h.b1, h.b2, h.eps,
                                   h.wd, None, None, None, h.grad_scale)
        torch.cuda.synchronize()
        assert torch.equal(scalars.view(torch.int32), before.view(torch.int32))
    torch.cuda.synchronize()
    _assert_slabs({k: t.cpu().numpy() for k, t in d.items()}, slabs.a, c, slabs, f"{route} error")


@pytest.mark.parametrize("route", ["many", "dev"])
def test_a_misaligned_28th_tensor_raises_and_nothing_is_touched(ops, route):
    _error_call(ops, route, spoil=(27, 1))


def test_a_28th_tensor_at_step_0_raises_and_nothing_is_touched(ops):
    _error_call(ops, "many", step0=True)


def test_nonfinite_check_refuses_a_misaligned_28th_tensor_before_it_flags(ops):
    from neurad_studio_amd import _lib

    ts = [torch.ones(64 + 8 * k, device="cuda") for k in range(30)]
    ts[0][5] = float("inf")  # the first launch would raise the flag
    keep = [t.clone() for t in ts]
    flag = torch.zeros((), device="cuda")
    with pytest.raises(ValueError):
        ops.nonfinite_check(ts[:27] + [ts[27][1:]] + ts[28:], flag)
    # and the entry point itself (the wrapper refuses such a view before it gets there)
    arr = (_lib.CheckTensor * 30)()
    for k, t in enumerate(ts):
        arr[k].data, arr[k].n, arr[k].dtype = t.data_ptr() + (4 if k == 27 else 0), t.numel() - (1 if k == 27 else 0), 0
    with pytest.raises(_lib.NeuradHipError):
        ops.launch("nrhip_nonfinite_check_many", arr, 30, flag)
    torch.cuda.synchronize()
    assert float(flag) == 0.0
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ts, keep))
    ops.nonfinite_check(ts, flag)
    assert float(flag) == 1.0


# ---- the non-finite check ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.CHECK_NS), ids=list(A.CHECK_NS))
def test_nonfinite_check_sees_one_bad_element_in_every_load_of_every_loop(ops, name):
    n, half, where, plan = A.check_positions(name)
    # the branch this case is for: one unrolled iteration and one remainder iteration for every lane, a second remainder
    # iteration for lanes 0 .. 699, a full tail
    assert (plan.unrolled_first, plan.unrolled_last, plan.rem_first, plan.rem_last, plan.rem2_lanes) == (1, 1, 2, 1, 700)
    assert plan.tail == (7 if half else 3)
    dtype = torch.float16 if half else torch.float32
    ints = torch.int16 if half else torch.int32
    big, tiny = torch.finfo(dtype).max, torch.finfo(dtype).smallest_normal / 4
    idx = torch.tensor(where, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(n, device="cuda", generator=gen).to(dtype)
    x[idx] = torch.tensor([big, -big, tiny, -0.0, -tiny], dtype=dtype, device="cuda").repeat(len(where) // 5 + 1)[:len(where)]
    pristine, xr = x.clone(), x.clone()  # xr: torch's copy (its check also unscales in place)
    other = [] if name.endswith("alone") else [torch.ones(A.COMPANION, device="cuda", dtype=dtype)]
    other_r = [t.clone() for t in other]
    one = torch.ones((), device="cuda")
    flags = torch.zeros(2, device="cuda")

    def both():
        flags.zero_()
        ops.nonfinite_check([x] + other, flags[0])
        torch._amp_foreach_non_finite_check_and_unscale_([xr] + other_r, flags[1], one)
        return flags.tolist()

    assert both() == [0.0, 0.0]  # +-max-finite, denormals and -0 at the very positions that get poisoned
    assert torch.equal(x.view(ints), pristine.view(ints))
    for bad in (float("inf"), float("-inf"), float("nan")):
        for i in where:
            x[i] = bad
            xr[i] = bad
            got = both()
            assert got == [1.0, 1.0], (name, i, bad, got)
            poisoned = x[i].clone()
            x[i] = pristine[i]
            xr[i] = pristine[i]
            assert (torch.isnan(poisoned) if bad != bad else poisoned == bad) and torch.equal(x.view(ints), pristine.view(ints)), (i, bad)
    assert both() == [0.0, 0.0]
    for t in other:
        assert torch.equal(t, torch.ones_like(t))


# ---- above the kernels ---------------------------------------------------------------------------------------------------
def test_hashgrid_adam_32_tables_with_step_counts_of_their_own():
    """capturable HashGridAdam over 32 parameters (two launches of the device form): five never receive a gradient, three
    receive one on alternate steps, so step counts differ within a launch"""
    from neurad_studio_amd.optim import HashGridAdam

    torch.manual_seed(7)
    sizes = [(257 + 61 * k, 4) if k % 3 else (1024 + 3 * k, 1) for k in range(32)]
    p0 = [torch.randn(s, device="cuda") * 0.1 for s in sizes]
    a = [torch.nn.Parameter(p.clone()) for p in p0]
    b = [torch.nn.Parameter(p.clone()) for p in p0]
    ours = HashGridAdam(a, lr=1e-2, eps=1e-15, capturable=True)
    ref = torch.optim.Adam(b, lr=1e-2, eps=1e-15)
    never, alternate = (2, 9, 17, 24, 31), (0, 13, 25)
    for step in range(6):
        for k in range(32):
            g = None
            if k not in never and not (k in alternate and step % 2):
                g = torch.randn(sizes[k], device="cuda") * (10.0 ** (step % 3 - 1))
                g[torch.rand(sizes[k][0], device="cuda") < 0.4] = 0.0
            a[k].grad, b[k].grad = (None, None) if g is None else (g.clone(), g.clone())
        ours.step()
        ref.step()
        for k in range(32):
            assert torch.allclose(a[k], b[k], rtol=2e-6, atol=3e-8), (step, k)
    for k in range(32):
        if k in never:
            assert not ours.state[a[k]] and not ref.state[b[k]] and torch.equal(a[k], p0[k])
            continue
        st = ours.state[a[k]]
        assert st["step"].is_cuda and float(st["step"]) == float(ref.state[b[k]]["step"]) == (3 if k in alternate else 6), k
        assert torch.allclose(st["exp_avg"], ref.state[b[k]]["exp_avg"], rtol=1e-6, atol=1e-12)
