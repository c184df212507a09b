"""Table copies that outlive one step: the stacked actor tables of the proposal field (field_components/neurad_encoding.py:
``_stacked_actor_tables`` + ag.StackTablesFn / MultiHashGridStackedFn) and the eval re-layout of a field table
(``ops.eval_table``, NRHIP_EVAL_RELAYOUT=1).

* A grad-enabled forward whose graph is dropped without a backward (an aborted iteration, a metrics pass under grad) must
  not hand the actor grids it touched a gradient in the next step: the reference's per-id loop never evaluates a grid no
  ray of the step hits, so torch.optim.Adam leaves its moments and step count alone -- HashGridAdam must too.
* ``ShardedTableAdam.step`` writes the tables through ``.data`` and raw kernels (no version bump): an eval render after it,
  in the same mode, must see the updated table, not the cached re-layout of the old one."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import cuda

pytestmark = pytest.mark.gpu

ACTOR_Y = (-24.0, -8.0, 8.0, 24.0)  # four parked 4 m cubes at x = 20 m, far enough apart that a ray window sees one
S = 48


def _parked_cars():
    ts = torch.tensor([0.0, 1.0])
    out = []
    for y in ACTOR_Y:
        p = torch.eye(4).repeat(2, 1, 1)
        p[:, :3, 3] = torch.tensor([20.0, y, 0.5])
        out.append({"timestamps": ts.clone(), "poses": p, "dims": torch.tensor([4.0, 4.0, 4.0]),
                    "symmetric": torch.tensor(True), "deformable": torch.tensor(False)})
    return out


def _proposal():
    """a training-mode proposal field (share_actor_table_grads on) over the four cars, O(1) tables, no ray flip"""
    from neurad_studio_amd.fields.neurad_field import NeuRADProposalField, NeuRADProposalFieldConfig
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    c = NeuRADProposalFieldConfig()
    c.grid.static.log2_hashmap_size = 11
    c.grid.actor.log2_hashmap_size = 8
    c.grid.actor.flip_prob = 0.0  # (a random flip per ray would make two runs differ)
    p = NeuRADProposalField(c, actors=DynamicActors(DynamicActorsConfig(), trajectories=_parked_cars()),
                            static_scale=100.0).cuda().train()
    assert p.hashgrid.share_actor_table_grads and len(p.hashgrid.actor_grids) == len(ACTOR_Y)
    w, _ = synth.linear(1, 6, 77, bias=False)
    with torch.no_grad():
        p.hashgrid.static_grid.hash_table.copy_(cuda(synth.hash_table(6 * 2**11, 1, seed=91, scale=2.0)))
        for i, gr in enumerate(p.hashgrid.actor_grids):
            gr.hash_table.copy_(cuda(synth.hash_table(4 * 2**8, 1, seed=500 + i, scale=1.5)))
        p.density_decoder.weight.copy_(cuda(w + np.float32(0.3)))
    return p


def _copy(p):
    q = _proposal()
    q.load_state_dict(p.state_dict())
    return q


def _samples(actors, seed, n_rays=1024):
    """rays from near the origin at the centres of ``actors`` (split evenly), S samples within 1.2 m of the aim point:
    every sample lies inside its actor's box.  n_rays * S >= 2^15 samples (and pairs): the table gradients go through
    the radix partition (csrc/encode_bwd_binned.hip), whose fixed-point sums are bit-reproducible."""
    from neurad_studio_amd.cameras.rays import RayBundle

    which = np.asarray(actors)[np.arange(n_rays) % len(actors)]
    centre = np.stack([np.full(n_rays, 20.0), np.asarray(ACTOR_Y)[which], np.full(n_rays, 0.5)], -1)
    o = synth.normal((n_rays, 3), seed) * np.float32(0.2) + np.array([0.0, 0.0, 0.5], np.float32)
    tgt = centre + synth.uniform((n_rays, 3), -0.3, 0.3, seed + 1)
    d = tgt - o
    dist = np.linalg.norm(d, axis=-1)
    d = (d / dist[:, None]).astype(np.float32)
    edges = (dist[:, None] + np.linspace(-1.2, 1.2, S + 1)[None]).astype(np.float32)
    rb = RayBundle(origins=cuda(o.astype(np.float32)), directions=cuda(d), pixel_area=torch.full((n_rays, 1), 2.43e-6, device="cuda"),
                   times=cuda(synth.uniform((n_rays, 1), 0.1, 0.9, seed + 2)))
    return rb.get_ray_samples(cuda(edges[:, :-1])[..., None], cuda(edges[:, 1:])[..., None])


def _loss(p, rs, seed):
    dens = p.get_density(rs)[0]
    return (dens * cuda(synth.uniform(tuple(dens.shape), 0.5, 1.5, seed))).sum()


def _grads(p):
    return {n: (None if q.grad is None else q.grad.clone()) for n, q in p.named_parameters()}


def _assert_grads_equal(got, want):
    """table gradients bit for bit; the decoder's through its per-block float atomics (csrc/actors.hip
    actor_density_splice_bwd) to the last bits"""
    assert got.keys() == want.keys()
    for n, w in want.items():
        g = got[n]
        assert (g is None) == (w is None), (n, g is None, w is None)
        if w is None:
            continue
        if n.endswith("hash_table"):
            assert torch.equal(g, w), n
        else:
            assert float((g - w).abs().max()) <= 1e-5 * float(w.abs().max()), n


def _actor_tables(p):
    return [gr.hash_table for gr in p.hashgrid.actor_grids]


def test_a_dropped_forward_leaves_the_actor_grids_it_touched_without_gradient():
    from neurad_studio_amd.optim import HashGridAdam

    p = _proposal()
    opt = HashGridAdam(list(p.hashgrid.parameters()), lr=1e-2)
    # a first step that touches every actor: every grid has moments and a step count to lose
    _loss(p, _samples([0, 1, 2, 3], seed=10), seed=11).backward()
    assert all(t.grad is not None for t in _actor_tables(p))
    opt.step()
    opt.zero_grad(set_to_none=True)
    p.density_decoder.weight.grad = None

    rs01, rs2 = _samples([0, 1], seed=20), _samples([2], seed=30)
    dropped = p.get_density(rs01)[0]  # pass 1: grad-enabled forward over actors {0, 1}, never backpropagated
    assert dropped.requires_grad
    del dropped
    _loss(p, rs2, seed=31).backward()  # pass 2: actor {2} only
    tables = _actor_tables(p)
    for a in (0, 1, 3):
        assert tables[a].grad is None, a
    assert tables[2].grad is not None and float(tables[2].grad.abs().sum()) > 0

    # pass 2 alone on a fresh copy with the same parameters: the same gradients
    q = _copy(p)
    _loss(q, rs2, seed=31).backward()
    _assert_grads_equal(_grads(p), _grads(q))

    # HashGridAdam leaves the untouched grids, their moments and their step counts exactly where they were
    before = {a: (tables[a].detach().clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[tables[a]].items()})
              for a in (0, 1, 3)}
    moved = tables[2].detach().clone()
    opt.step()
    for a, (t, st) in before.items():
        assert torch.equal(tables[a].detach(), t), a
        now = opt.state[tables[a]]
        assert now.keys() == st.keys()
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(now[k], st[k]), (a, k)
        assert float(now["step"]) == float(st["step"]) == 1.0, a
    assert not torch.equal(tables[2].detach(), moved) and float(opt.state[tables[2]]["step"]) == 2.0


def test_two_sampler_rounds_in_one_step_add_up_per_grid():
    """the ordinary case the shared stack exists for: the proposal field evaluated twice in one step (two sampler rounds)
    -- each grid receives the sum of both rounds' gradients, a grid neither round touches receives None"""
    p = _proposal()
    ra, rb = _samples([0], seed=40), _samples([1, 2], seed=50)
    (_loss(p, ra, seed=41) + _loss(p, rb, seed=51)).backward()
    got = _grads(p)
    tables = _actor_tables(p)
    assert tables[3].grad is None
    assert all(tables[a].grad is not None for a in (0, 1, 2))
    qa, qb = _copy(p), _copy(p)
    _loss(qa, ra, seed=41).backward()
    _loss(qb, rb, seed=51).backward()
    ga, gb = _grads(qa), _grads(qb)
    assert ga["hashgrid.actor_grids.1.hash_table"] is None and gb["hashgrid.actor_grids.0.hash_table"] is None
    want = {}
    for n in got:
        parts = [g for g in (ga[n], gb[n]) if g is not None]
        want[n] = None if not parts else (parts[0] if len(parts) == 1 else parts[0] + parts[1])
    _assert_grads_equal(got, want)


def _field(table=None):
    """a field whose static table qualifies for the eval re-layout (8 x 4 levels at 2^18 rows: level 0 gets a shadow copy)"""
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig

    cfg = NeuRADFieldConfig()
    cfg.grid.static.log2_hashmap_size = 18
    f = NeuRADField(cfg, actors=None, static_scale=100.0).cuda().eval()
    with torch.no_grad():
        t = f.hashgrid.static_grid.hash_table
        t.copy_(cuda(synth.hash_table(t.shape[0], 4, seed=51, scale=0.5)) if table is None else table)
        for k, l in enumerate(f.mlp_geo.layers):
            w, b = synth.linear(l.out_features, l.in_features, 200 + 10 * k)
            l.weight.copy_(cuda(w)), l.bias.copy_(cuda(b))
        for k, l in enumerate(f.mlp_feature.layers):
            w, b = synth.linear(l.out_features, l.in_features, 300 + 10 * k)
            l.weight.copy_(cuda(w)), l.bias.copy_(cuda(b))
    return f


def test_sharded_table_adam_step_invalidates_the_eval_relayout(monkeypatch):
    from neurad_studio_amd import ops
    from neurad_studio_amd.parallel.sharded_adam import ShardedTableAdam

    monkeypatch.setattr(ops, "_EVAL_RELAYOUT", True)
    ops.clear_eval_tables()
    f = _field()
    t = f.hashgrid.static_grid.hash_table
    assert ops.eval_layout_plan(f.hashgrid.static_grid.spec, t.dtype)[2] >= 1 and f.fused_supported()
    R = 2048
    o, d, area, _ = synth.rays(R, 5)
    edges = np.linspace(0.5, 60.0, 33, dtype=np.float32)[None].repeat(R, 0)
    args = (cuda(o), cuda(d), cuda(area), cuda(edges[:, :-1]), cuda(edges[:, 1:]))

    def render(field):
        with torch.no_grad():
            return field.render(*args)

    before = render(f)
    assert len(ops._EVAL_TABLES) == 1  # the re-laid-out table is cached
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    t.grad = torch.randn(t.shape, device="cuda", generator=g)
    ShardedTableAdam([t], lr=1e-2).step()  # world size 1, same mode: nothing else drops the cache
    after = render(f)
    want = render(_field(t.detach()))  # a fresh field holding the updated table
    for a, b in zip(after, want):
        assert torch.equal(a, b)
    assert not torch.equal(after[0], before[0])
    ops.clear_eval_tables()
