"""The MLP kernels (csrc/mlp.hip, csrc/mlp_chain.hip) element by element, at the smallest shape that reaches each launch
branch of nrhip_mlp_fwd, nrhip_mlp_bwd and nrhip_field_feature_bwd.  Every operand is a small integer and every sum of
absolute products stays below 2^24 (tests/mlp_refs.py derives why and `assert_exact_operands` checks it for every case),
so the kernels must return the int64 reference BIT FOR BIT: outputs, data gradients, the dZ they park, ReLU masks at
pre-activations of exactly 0, weight and bias gradients.  Outputs start at a sentinel with a guard row behind them; weight
and bias gradients start at the integer 3 on every path, and must end at 3 + reference (the header: ACCUMULATED into).

Branch reached <- shape, and the query or restatement (tests/mlp_refs.py) that shows it:
 nrhip_mlp_fwd
  chained kernel, persistent loop        the six shapes of mlp_refs.CHAINED, n = 1, 15, 16, 17, 1000, 70001 <- chain_workgroups:
                                         1094 workgroups' worth of tiles > cu_count * 4
  chained kernel, hidden == NULL         the six shapes, n = 17
  chained shape on the generic kernel    x one float off the 16-byte grid; y one float off (48 -> 32 -> 32 -> 32, out % 4 == 0);
                                         hidden one float off; NRHIP_MLP_GENERIC=1 on all six shapes
  generic kernel                         3 -> 7 -> 5; 13 -> 24 -> 24 -> 24 -> 3 and 8 layers of width 20 with biases on
                                         alternate layers; 5 -> 100 -> 9; 200 -> 7; 70 -> 130 -> 65 (5 and 9 sixteen-blocks: the
                                         unpaired last block of layer_tile); n = 1, 17, 100 (two workgroups)
  4 / 2 / 1 waves, LDS above 64 KiB      any small shape / 48 -> 128 -> 128 -> 16 (and 70 -> 130 -> 65) / 64 -> 144 -> 144 -> 16
                                         <- pick_waves, lds_bytes
  too large                              256 -> 256 -> 256 -> 256 <- pick_waves == 0: NRHIP_ERR_UNSUPPORTED, nothing written
  grid cap                               3 -> 5 -> 2, n = 131,089 <- blocks_for_tiles: 8194 tiles, 2048 workgroups of 4 waves
 nrhip_mlp_bwd
  fused weight gradient, full mask       32 -> 32 -> 33, 32 -> 64 -> 33, 48 -> 32 -> 32 -> 32, 64 -> 32 -> 32 -> 32
                                         <- nrhip_mlp_bwd_workspace - dZ block = NSLOT * 64 * 1024 (mask_from_workspace)
  fused weight gradient, partial mask    48 -> 64 -> 64 -> 32, 64 -> 64 -> 64 -> 32 <- the same query; layer 0 from
                                         mlp_wgrad_kernel reading the parked dZ
  wgrad_merge_kernel loops               n = 64 k - 7, k = 1, 3, 4, 5, 13, 16, 17, 29 workgroups <- chain_workgroups; a full and
                                         a partial mask
  workspace of dZ + 1 partial            n = 1000: one workgroup walks all 63 tiles <- chain_workgroups(n, 1)
  workspace of dZ + 5 partials           n = 1000: blocks > fit <- chain_workgroups(n, 5) == 5 < 16
  workspace of dZ only                   launch_bwd (the data-only chain) + mlp_wgrad_kernel for every layer; dZ compared
  NRHIP_MLP_SPLIT_WGRAD, NRHIP_MLP_GENERIC  all six shapes, n = 17 and 1000; dZ compared
  grad_weight[l] == NULL                 each l of 48 -> 32 -> 32 -> 32 (all_w false: data-only chain + mlp_wgrad_kernel for
                                         the others) and of 13 -> 24 -> 24 -> 24 -> 3; the skipped layer's bias gradient stays 3
  grad_bias == NULL, grad_bias[l] == NULL  fused (merge kernel), data-only chain + mlp_wgrad_kernel, generic
  grad_x == NULL                         chained with the fused weight gradient; chained without; 13 -> 24 -> 24 -> 24 -> 3;
                                         9 -> 6 (one layer: no data kernel at all)
  one layer with grad_x                  9 -> 6, 200 -> 7
  misaligned hidden / workspace / grad_x 48 -> 32 -> 32 -> 32: the generic kernels
  mlp_bwd_data_kernel                    the generic shapes and the 4 / 2 / 1-wave plans above <- pick_waves(transposed);
                                         hidden widths 7, 20 and 130: the pad4 zeroing
  mlp_wgrad_kernel                       70 -> 130 -> 65: 2 x 3 and 3 x 2 ragged 64 x 64 sub-matrices, two layers by sub0
                                         <- wgrad_grid; n = 1, 2, 3, 5, 1023: n % 4, waves with no quad, quads past the end
                                         inside the 4-deep unroll; 5 -> 7 -> 3, n = 262,149 <- wgrad_grid: 257 slices asked, 256
 nrhip_field_feature_bwd
  full / partial mask                    48 -> 32 -> 32 -> 32 / 48 -> 64 -> 64 -> 32, n = 1, 15, 17, 1000, 70001 <- the query
  workspace of dZ + 1 partial            n = 1000
  misaligned grad_feature                NRHIP_ERR_UNSUPPORTED, nothing written"""
import pytest
import torch

import mlp_refs as MR
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SENT = MR.SENTINEL
ERR_UNSUPPORTED = r"\(code 2\)"


# ---- buffers -------------------------------------------------------------------------------------------------------------
def _placed(t, off=0):
    """a device copy of `t` whose address is `off` floats past a 16-byte boundary"""
    flat = torch.zeros((t.numel() + 4,), device="cuda")
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


class Out:
    """an output of `rows` x `cols` floats, `off` floats past a 16-byte boundary, in a buffer full of the sentinel that goes
    on for one guard row"""

    def __init__(self, rows, cols, off=0):
        self.flat = torch.full((off + (rows + 1) * cols + 4,), SENT, device="cuda")
        self.lo, self.hi = off, off + rows * cols
        self.t = self.flat[self.lo:self.hi].view(rows, cols)
        assert self.t.data_ptr() % 16 == 4 * off

    def check(self, want, what):
        MR.assert_equal(self.t, want, what)  # the reference holds integers: an element left at the sentinel differs
        outside = torch.cat([self.flat[:self.lo], self.flat[self.hi:]])
        assert bool((outside == SENT).all()), f"{what}: written outside its {self.t.shape[0]} rows"

    def check_untouched(self, what):
        assert bool((self.flat == SENT).all()), f"{what}: written to"


def _mlp(ops, c):
    ws = [w.cuda() for w in c["weights"]]
    bs = [None if b is None else b.cuda() for b in c["biases"]]
    m, keep = ops._c_mlp(ws, bs)
    return m, (ws, bs, keep)


def _what(c, note):
    return f"{' -> '.join(map(str, c['dims']))} n={c['n']} {note}"


def _case(dims, n, **kw):
    c = MR.case(dims, n, **kw)
    MR.assert_exact_operands(c)
    return c


def _f32(a):
    return torch.from_numpy(a.astype("float32"))


# ---- runners -------------------------------------------------------------------------------------------------------------
def run_fwd(ops, c, note, hidden=True, x_off=0, y_off=0, h_off=0):
    n, dims, nl = c["n"], c["dims"], c["nl"]
    m, keep = _mlp(ops, c)
    x = _placed(c["x"], x_off)
    y = Out(n, dims[-1], y_off)
    hid = Out(n, (nl - 1) * c["h"], h_off) if hidden and nl > 1 else None
    ops.launch("nrhip_mlp_fwd", m, x, n, y.t, None if hid is None else hid.t)
    torch.cuda.synchronize()
    y.check(c["y"], _what(c, note + " y"))
    if hid is not None:
        hid.check(c["hidden"], _what(c, note + " hidden"))


def workspace_query(ops, c, m):
    _, need = ops._workspace("nrhip_mlp_bwd_workspace", m, c["n"], device="cuda", dtype=torch.float32)
    return need


def dz_block(c):
    """(floats of the dZ block, where the partials start behind it)"""
    f = c["n"] * (c["nl"] - 1) * c["h"]
    return f, (f + 3) & ~3


def _grads(c, null_w, null_b, bias_array, ops):
    gws = [torch.full(tuple(w.shape), float(MR.PREFILL), device="cuda") for w in c["weights"]]
    gbs = [torch.full((w.shape[0],), float(MR.PREFILL), device="cuda") for w in c["weights"]]
    from neurad_studio_amd import _lib

    pw = ops._host_ptrs([None if l in null_w else g for l, g in enumerate(gws)], _lib.MAX_LAYERS)
    pb = ops._host_ptrs([None if l in null_b else g for l, g in enumerate(gbs)], _lib.MAX_LAYERS) if bias_array else None
    return gws, gbs, pw, pb


def _check_grads(c, gws, gbs, null_w, null_b, bias_array, note):
    for l in range(c["nl"]):
        if l in null_w:  # the layer is skipped as a whole
            MR.assert_equal(gbs[l], 0 * c["db"][l] + MR.PREFILL, _what(c, f"{note} grad_bias[{l}] of a layer without grad_weight"))
            continue
        MR.assert_equal(gws[l], c["dW"][l] + MR.PREFILL, _what(c, f"{note} grad_weight[{l}]"))
        want = c["db"][l] + MR.PREFILL if bias_array and l not in null_b else 0 * c["db"][l] + MR.PREFILL
        MR.assert_equal(gbs[l], want, _what(c, f"{note} grad_bias[{l}]"))


def run_bwd(ops, c, note, grad_x=True, partials=None, null_w=(), null_b=(), bias_array=True, h_off=0, ws_off=0, gx_off=0,
            check_dz=False, expect_mask=None):
    """partials: None = the workspace nrhip_mlp_bwd_workspace asks for; k = the dZ block and room for k partials (0: the
    dZ block alone, to the float)"""
    n, dims, nl = c["n"], c["dims"], c["nl"]
    m, keep = _mlp(ops, c)
    need = workspace_query(ops, c, m)
    dzf, part_off = dz_block(c)
    if expect_mask is not None:
        assert MR.mask_from_workspace(dims, n, need) == expect_mask == MR.wg_mask(dims)
    elif dims not in MR.CHAINED:
        assert need == part_off  # no fused weight gradient for this shape
    floats = need if partials is None else (part_off + partials * MR.part_floats(dims) if partials else dzf)
    ws = Out(1, max(floats, 1), ws_off)
    x, gy = c["x"].cuda(), c["grad_y"].cuda()
    hid = _placed(_f32(c["hidden"]), h_off) if nl > 1 else None
    gx = Out(n, dims[0], gx_off) if grad_x else None
    gws, gbs, pw, pb = _grads(c, null_w, null_b, bias_array, ops)
    ops.launch("nrhip_mlp_bwd", m, x, hid, gy, n, None if gx is None else gx.t, pw, pb, ws.t, floats)
    torch.cuda.synchronize()
    if gx is not None:
        gx.check(c["grad_x"], _what(c, note + " grad_x"))
    _check_grads(c, gws, gbs, null_w, null_b, bias_array, note)
    outside = torch.cat([ws.flat[:ws.lo], ws.flat[ws.hi:]])
    assert bool((outside == SENT).all()), _what(c, note + ": written outside the workspace")
    if check_dz and nl > 1:
        import numpy as np

        MR.assert_equal(ws.t.reshape(-1)[:dzf].view(n, -1), np.concatenate(c["dz"][:-1], 1), _what(c, note + " dZ"))


def run_feature_bwd(ops, c, note, partials=None, expect_mask=None):
    n, dims = c["n"], c["dims"]
    m, keep = _mlp(ops, c)
    need = workspace_query(ops, c, m)
    dzf, part_off = dz_block(c)
    assert MR.mask_from_workspace(dims, n, need) == expect_mask == MR.wg_mask(dims)
    floats = need if partials is None else part_off + partials * MR.part_floats(dims)
    ws = Out(1, floats)
    x, gf, col0 = c["x"].cuda(), _placed(c["grad_y"]), c["grad_geo0"].cuda()
    hid = _placed(_f32(c["hidden"]))
    gg = Out(n, 33)
    gws, gbs, pw, pb = _grads(c, (), (), True, ops)
    ops.launch("nrhip_field_feature_bwd", m, x, hid, gf, col0, n, gg.t, pw, pb, ws.t, floats)
    torch.cuda.synchronize()
    gg.check(c["grad_geo"], _what(c, note + " grad_geo"))
    MR.assert_equal(gg.t[:, 0], c["grad_geo0"].long().numpy(), _what(c, note + " grad_geo column 0"))
    _check_grads(c, gws, gbs, (), (), True, note)
    assert bool((ws.flat[ws.hi:] == SENT).all()), _what(c, note + ": written outside the workspace")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- nrhip_mlp_fwd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", MR.CHAINED)
def test_forward_chained(ops, dims):
    assert MR.chain_workgroups(70001, 4 * _cus()) == 4 * _cus() < MR.chain_workgroups(70001, 10 ** 9)  # the persistent loop
    for n in MR.CHAIN_NS:
        run_fwd(ops, _case(dims, n), "chained forward")
    run_fwd(ops, _case(dims, 17), "chained forward without hidden", hidden=False)


@pytest.mark.parametrize("how", ["x", "y", "hidden"])
def test_forward_of_a_chained_shape_with_a_misaligned_pointer(ops, how):
    dims = (48, 32, 32, 32)
    assert dims in MR.CHAINED and dims[-1] % 4 == 0  # a misaligned y matters only where the kernel stores y in 16-byte pieces
    for n in (17, 1000):
        run_fwd(ops, _case(dims, n), f"forward, {how} one float off", **{how[0] + "_off": 1})


@pytest.mark.parametrize("switch", ["NRHIP_MLP_GENERIC", "NRHIP_MLP_SPLIT_WGRAD"])
@pytest.mark.parametrize("dims", MR.CHAINED)
def test_chained_shapes_under_the_switches(ops, switches, switch, dims):
    switches.set(switch, "1")
    for n in MR.SWITCH_NS:
        c = _case(dims, n)
        run_fwd(ops, c, f"forward, {switch}")
        run_bwd(ops, c, f"backward, {switch}", check_dz=True, expect_mask=MR.wg_mask(dims))
    run_bwd(ops, _case(dims, 17), f"backward, {switch}, no grad_x", grad_x=False, check_dz=True)


@pytest.mark.parametrize("dims,kw", MR.GENERIC + ((MR.SINGLE, {}),), ids=["-".join(map(str, d)) for d, _ in MR.GENERIC] + ["9-6"])
def test_generic_kernels(ops, dims, kw):
    waves = 2 if dims == MR.WGRAD_RAGGED else 4
    assert dims not in MR.CHAINED and MR.pick_waves(dims) == MR.pick_waves(dims, True) == waves
    assert MR.blocks_for_tiles(100, waves) == 8 // waves  # 7 tiles: more than one workgroup
    for n in MR.GENERIC_NS:
        c = _case(dims, n, **kw)
        run_fwd(ops, c, "generic forward")
        run_bwd(ops, c, "generic backward", check_dz=True)
    c = _case(dims, 17, **kw)
    run_fwd(ops, c, "generic forward without hidden", hidden=False)
    run_bwd(ops, c, "generic backward, no grad_x", grad_x=False, check_dz=True)
    run_bwd(ops, c, "generic backward, no grad_bias", bias_array=False)
    run_bwd(ops, c, "generic backward, grad_bias[0] NULL", null_b=(0,))


@pytest.mark.parametrize("dims,waves", [(MR.TWO_WAVES, 2), (MR.ONE_WAVE, 1)])
def test_generic_kernels_with_fewer_waves_and_large_lds(ops, dims, waves):
    for tr in (False, True):
        assert MR.pick_waves(dims, tr) == waves
        assert 64 * 1024 < MR.lds_bytes(dims, waves, tr) <= 160 * 1024 < MR.lds_bytes(dims, 2 * waves, tr)
    if dims == MR.TWO_WAVES:
        assert MR.lds_bytes(dims, 0) == 98304 and MR.lds_bytes(dims, 4) == 164864
    else:
        assert MR.lds_bytes(dims, 0) == 129024 and MR.lds_bytes(dims, 1) == 129024 + 20736
    for n in MR.PLAN_NS:
        assert MR.blocks_for_tiles(n, waves) == {(17, 2): 1, (100, 2): 4, (17, 1): 2, (100, 1): 7}[n, waves]
        c = _case(dims, n)
        run_fwd(ops, c, f"forward, {waves} waves")
        run_bwd(ops, c, f"backward, {waves} waves", check_dz=True)


def test_too_large_an_mlp_is_refused_and_nothing_is_written(ops):
    from neurad_studio_amd._lib import NeuradHipError

    dims = MR.TOO_LARGE
    assert MR.pick_waves(dims) == 0 == MR.pick_waves(dims, True)
    ws = [torch.zeros((256, 256), device="cuda") for _ in range(3)]
    m, keep = ops._c_mlp(ws, [None] * 3)
    x, y, hid = torch.zeros((5, 256), device="cuda"), Out(5, 256), Out(5, 512)
    with pytest.raises(NeuradHipError, match=ERR_UNSUPPORTED):
        ops.launch("nrhip_mlp_fwd", m, x, 5, y.t, hid.t)
    torch.cuda.synchronize()
    y.check_untouched("y of a refused forward"), hid.check_untouched("hidden of a refused forward")


def test_forward_grid_cap(ops):
    dims, n = MR.FWD_CAPPED
    assert -(-n // 16) == 8194 and MR.blocks_for_tiles(n, MR.pick_waves(dims)) == 2048 < -(-8194 // 4)
    run_fwd(ops, _case(dims, n), "forward past the grid cap")


# ---- nrhip_mlp_bwd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", MR.CHAINED)
def test_backward_chained_with_the_fused_weight_gradient(ops, dims):
    mask = MR.wg_mask(dims)
    full = (1 << (len(dims) - 1)) - 1
    assert mask == (full & ~1 if dims in ((48, 64, 64, 32), (64, 64, 64, 32)) else full)
    for n in MR.CHAIN_NS:
        run_bwd(ops, _case(dims, n), "fused backward", expect_mask=mask)
    c = _case(dims, 1000)
    run_bwd(ops, c, "fused backward, no grad_x", grad_x=False, expect_mask=mask)
    run_bwd(ops, c, "fused backward, no grad_bias", bias_array=False)
    for l in range(len(dims) - 1):
        run_bwd(ops, c, f"fused backward, grad_bias[{l}] NULL", null_b=(l,))


@pytest.mark.parametrize("k", MR.MERGE_COUNTS)
def test_merge_of_k_partials(ops, k):
    if k > MR.chain_workgroups(10 ** 9, _cus()):
        pytest.skip(f"{k} workgroups exceed this device's cap of one per compute unit ({_cus()})")
    n = 64 * k - 7
    assert MR.chain_workgroups(n, min(_cus(), 1024)) == k  # 1024: the partials the full workspace has room for
    for dims in MR.MERGE_SHAPES:
        run_bwd(ops, _case(dims, n), f"fused backward, {k} partials", expect_mask=MR.wg_mask(dims))


@pytest.mark.parametrize("dims", MR.MERGE_SHAPES)
def test_backward_with_smaller_workspaces(ops, dims):
    c = _case(dims, 1000)
    assert MR.chain_workgroups(1000, 1) == 1 and MR.chain_workgroups(1000, 5) == 5 < MR.chain_workgroups(1000, 10 ** 9) == 16
    run_bwd(ops, c, "fused backward, room for one partial", partials=1)
    run_bwd(ops, c, "fused backward, room for five partials", partials=5)
    run_bwd(ops, c, "backward, workspace of dZ alone", partials=0, check_dz=True)
    run_bwd(ops, c, "backward, workspace of dZ alone, no grad_x", partials=0, grad_x=False, check_dz=True)
    run_bwd(ops, c, "backward, workspace of dZ alone, no grad_bias", partials=0, bias_array=False)
    run_bwd(ops, c, "backward, workspace of dZ alone, grad_bias[1] NULL", partials=0, null_b=(1,))


@pytest.mark.parametrize("dims,kw", [((48, 32, 32, 32), {}), MR.GENERIC[1]], ids=["chained", "generic"])
def test_backward_without_one_weight_gradient(ops, dims, kw):
    c = _case(dims, 1000 if dims in MR.CHAINED else 100, **kw)
    for l in range(len(dims) - 1):
        run_bwd(ops, c, f"backward, grad_weight[{l}] NULL", null_w=(l,), check_dz=True)


@pytest.mark.parametrize("which", ["h", "ws", "gx"])
def test_backward_of_a_chained_shape_with_a_misaligned_pointer(ops, which):
    for n in (17, 1000):
        run_bwd(ops, _case((48, 32, 32, 32), n), f"backward, {which} one float off", check_dz=True, **{which + "_off": 1})


def test_single_layer(ops):
    for dims in (MR.SINGLE, (200, 7)):
        for n in MR.GENERIC_NS:
            c = _case(dims, n)
            run_bwd(ops, c, "one layer with grad_x")
            run_bwd(ops, c, "one layer without grad_x", grad_x=False)


@pytest.mark.parametrize("n", MR.WGRAD_NS)
def test_weight_gradient_kernel_on_ragged_sub_matrices(ops, n):
    dims = MR.WGRAD_RAGGED
    bx, nsub, sub0 = MR.wgrad_grid(dims, n)
    assert (bx, nsub, sub0) == (1, 3 * 2 + 2 * 3, [0, 6])
    run_bwd(ops, _case(dims, n), "ragged weight gradient", check_dz=True)


def test_weight_gradient_kernel_slice_cap(ops):
    dims, n = MR.WGRAD_CAPPED
    assert ((n + 3) // 4 + 255) // 256 == 257 and MR.wgrad_grid(dims, n)[0] == 256
    run_bwd(ops, _case(dims, n), "weight gradient past the slice cap", grad_x=False)


# ---- nrhip_field_feature_bwd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,mask", [(32, 7), (64, 6)])
def test_feature_head_backward(ops, h, mask):
    for n in MR.FEATURE_NS:
        c = MR.feature_case(h, n)
        MR.assert_exact_operands(c)
        run_feature_bwd(ops, c, "feature head", expect_mask=mask)
    c = MR.feature_case(h, 1000)
    run_feature_bwd(ops, c, "feature head, room for one partial", partials=1, expect_mask=mask)


@pytest.mark.parametrize("h", [32, 64])
def test_feature_head_backward_refuses_a_misaligned_grad_feature(ops, h):
    from neurad_studio_amd._lib import NeuradHipError

    c = MR.feature_case(h, 17)
    m, keep = _mlp(ops, c)
    need = workspace_query(ops, c, m)
    ws, gg = Out(1, need), Out(17, 33)
    gws, gbs, pw, pb = _grads(c, (), (), True, ops)
    with pytest.raises(NeuradHipError, match=ERR_UNSUPPORTED):
        ops.launch("nrhip_field_feature_bwd", m, c["x"].cuda(), _placed(_f32(c["hidden"])), _placed(c["grad_y"], 1),
                   c["grad_geo0"].cuda(), 17, gg.t, pw, pb, ws.t, need)
    torch.cuda.synchronize()
    gg.check_untouched("grad_geo of a refused call"), ws.check_untouched("workspace of a refused call")
    for g in gws + gbs:
        assert bool((g == MR.PREFILL).all())
