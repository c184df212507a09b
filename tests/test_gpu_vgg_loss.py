"""The VGG perceptual loss as one autograd node (model_components/perceptual.py on csrc/vgg_loss.hip), pinned stage by stage
on its OWN saved tensors.

Why there is no end-to-end precision bound: two fp16-activation restatements of this network that differ only in fp32 and
float64 accumulation end up 3.5-8 % apart in the gradient (ReLU masks and L1 signs flip) while agreeing to 2e-5 .. 2e-4 in
the loss, so a comparison with a float64 network tests nothing.  Instead:
  forward   every layer's float64 conv + bias + ReLU of the node's saved INPUT must match the node's saved OUTPUT within the
            derived per-element bound (9 Cin + 1) u sum |a||w| + 2^-11 |ref|; pools are exact; the loss is the weighted sum
            of the L1 terms of the node's own five features within 8 u.
  backward  tests/vgg_refs.py runs the float64 chain on the saved activations (masks, argmax and signs from them: a linear
            map), once exactly (A) and once with every inter-layer gradient rounded to fp16 at the power-of-two scale the
            kernels' rule gives it (B).  d_AB = |B - A| / |A| is what the fp16 gradient storage alone costs; the node must
            come within 2 d_AB of A (the factor 2 is the margin for the fp32 accumulation order).
Together the stages pin the wiring: a wrong tap, weight or layer order fails its stage.

Seeded He-scaled weights rounded to fp16, biases of about 0.05, uniform images rounded to fp16 (no real weights: torchvision
is not a dependency).  Sizes 2x16x16, 2x32x32, and 1x17x19 for the odd-size path.

Observed on an MI355X, for the record only (no bound is set from these):
  2x16x16: d_AB 5.16e-4, node 5.21e-4 (1.01 d_AB); 2x32x32: d_AB 6.48e-4, node 6.41e-4 (0.989 d_AB); 1x17x19: d_AB 5.91e-4,
  node 5.73e-4 (0.969 d_AB); largest forward err / bound 0.98-0.99 (the bound's half-ulp term 2^-11 |ref| is reached by any
  correctly rounded fp16 value at the bottom of its binade: a ratio just under 1 is what a correct kernel gives); loss err
  0.19-0.53 u."""
import pytest
import torch

import vgg_refs as R

pytestmark = pytest.mark.gpu

SIZES = [(2, 16, 16), (2, 32, 32), (1, 17, 19)]


@pytest.fixture(scope="module")
def module():
    from neurad_studio_amd.model_components.perceptual import VGGPerceptualLoss

    m = VGGPerceptualLoss()
    m.load_state_dict(R.make_weights(0))
    return m.cuda()


@pytest.fixture(scope="module")
def runs(module):
    """size -> (x, y, loss, saved (CPU), grad_x): one run of the node per size, shared and left unchanged"""
    from neurad_studio_amd.model_components.perceptual import vgg_perceptual_loss

    out = {}
    for size in SIZES:
        x, y = R.make_images(*size, seed=sum(size))
        xc = x.cuda().requires_grad_(True)
        loss, saved = vgg_perceptual_loss(xc, y.cuda(), module.packs(), module.weights, return_saved=True)
        loss.backward()
        out[size] = (x, y, loss.detach().cpu(), {k: v.cpu() for k, v in saved.items()}, xc.grad.cpu())
    return out


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_forward_stage_by_stage_on_the_nodes_own_tensors(module, runs, size):
    x, y, loss, saved, _ = runs[size]
    b = size[0]
    weights = {k: v.cpu() for k, v in module.state_dict().items()}
    assert saved["image"].shape == (2 * b, size[1], size[2], 16)
    assert torch.equal(saved["image"][..., :3], torch.cat([x, y]).half()) and not saved["image"][..., 3:].any()
    worst = 0.0
    for st in R.steps():
        if st[0] == "conv":
            _, src, dst, cin, cout = st
            ref, bound = R.conv_layer_ref(saved[src], weights[R.key_of(dst, "weight")], weights[R.key_of(dst, "bias")])
            got = saved[dst].double()
            assert got.shape == ref.shape and torch.isfinite(got).all()
            ratio = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{dst}: err / bound = {ratio}"
            assert 0 < float((got > 0).double().mean()) < 1, dst  # a living layer with ReLU zeros
        elif st[0] == "pool":
            assert torch.equal(saved[st[2]].double(), R.pool_fwd(saved[st[1]])), st[2]
    want = R.loss_ref(saved, b, module.weights)
    err = abs(float(loss) - want)
    print(f"[vgg-loss] {size}: largest forward err / bound = {worst:.3g}; loss {float(loss):.6g}, err = {err / (R.U32 * want):.3g} u")
    assert err <= 8 * R.U32 * want and want > 0


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_backward_within_twice_what_fp16_gradient_storage_costs(module, runs, size):
    _, _, _, saved, grad = runs[size]
    weights = {k: v.cpu() for k, v in module.state_dict().items()}
    a = R.backward_ref(saved, weights, size[0], tap_weights=module.weights)
    b = R.backward_ref(saved, weights, size[0], tap_weights=module.weights, rounded=True)
    d_ab, d_got = R.rel_l2(b, a), R.rel_l2(grad.double(), a)
    print(f"[vgg-loss] {size}: d_AB = {d_ab:.3g}, |got - A| / |A| = {d_got:.3g} ({d_got / d_ab:.3g} d_AB)")
    assert grad.shape == (size[0], size[1], size[2], 3) and torch.isfinite(grad).all() and float(a.abs().max()) > 0
    assert d_got <= 2 * d_ab


def test_no_gradient_for_the_target_and_nothing_saved_without_one(module):
    from neurad_studio_amd.model_components.perceptual import vgg_perceptual_loss

    x, y = (t.cuda() for t in R.make_images(2, 16, 16))
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    loss = module(xg, yg)
    gx, gy = torch.autograd.grad(loss, (xg, yg), allow_unused=True)
    assert gy is None and gx is not None and float(gx.abs().max()) > 0
    loss2, saved = vgg_perceptual_loss(x, y, module.packs(), module.weights, return_saved=True)
    assert saved == {} and not loss2.requires_grad and torch.equal(loss2, loss.detach())
    loss3, saved3 = vgg_perceptual_loss(x, yg, module.packs(), module.weights, return_saved=True)  # only the target asks
    assert saved3 == {} and torch.equal(loss3.detach(), loss.detach())
    with torch.autocast("cuda", dtype=torch.float16):  # the trainer's context: inputs are cast back to fp32
        assert torch.equal(module(x.half(), y.half()), loss.detach())
    for bad in ((2, 15, 16, 3), (2, 16, 16, 4)):
        with pytest.raises(ValueError):
            module(torch.zeros(bad, device="cuda"), torch.zeros(bad, device="cuda"))


def test_run_to_run_and_graph_replay_give_the_same_bits(module):
    x, y = (t.cuda() for t in R.make_images(2, 32, 32, seed=9))

    def step(xin):
        loss = module(xin, y)
        (g,) = torch.autograd.grad(loss, xin)
        return loss.detach(), g

    xs = x.clone().requires_grad_(True)
    l0, g0 = step(xs)
    l1, g1 = step(xs)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(xs)  # warm-up on the side stream: packs, allocator
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lg, gg = step(xs)
    with torch.no_grad():
        xs.copy_(R.make_images(2, 32, 32, seed=10)[0].cuda())  # other pixels: the replay must recompute
    graph.replay()
    torch.cuda.synchronize()
    le, ge = step(xs)
    assert torch.equal(lg, le) and torch.equal(gg, ge) and not torch.equal(ge, g0)


def test_a_weight_edited_in_place_is_picked_up(module):
    x, y = (t.cuda() for t in R.make_images(1, 16, 16, seed=4))
    before = module(x, y)
    w = dict(module.named_parameters())["vgg.slice1.0.0.weight"]
    key, keep = module.cache_key(), w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(0.5)
        assert module.cache_key() != key
        after = module(x, y)
        assert not torch.equal(after, before)
        fresh = type(module)().cuda()
        fresh.load_state_dict(module.state_dict())
        assert torch.equal(fresh(x, y), after)
    finally:
        with torch.no_grad():
            w.copy_(keep)
    assert torch.equal(module(x, y), before)
