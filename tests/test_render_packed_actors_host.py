"""Host side of the occupancy route with dynamic actors: the PackedActors instantiation set of csrc/render_variants.h, the
field's gate, the ABI version, the sampler's argument errors, and the numpy restatement of the box-aware march rule against
itself (tests/packed_actor_refs.py).  No GPU.

The field checks run in a child process, as tests/test_render_packed_host.py does."""
import os
import subprocess

import numpy as np

import occgrid_oracle as OO
import packed_actor_refs as PA
from host_gate import VARIANTS, gate_constants, run_child, variant_rows

RULE = r'''
#include <cstdio>
#include "render_variants.h"
using namespace nrhip;
int main() {
#define X(L_, F_, H_, O_, S_, P_)                                                     \
  if (render_variant_ok(L_, F_, Out::O_, Src::S_, Prod::P_, Lay::PackedActors))       \
    std::printf("%d %d %d %s %s %s\n", L_, F_, H_, #O_, #S_, #P_);
  NRHIP_RENDER_VARIANTS(X)
  return 0;
}
'''


def test_packed_actor_instantiations_are_the_composited_actor_rows(tmp_path):
    """The rule itself is asked -- the header compiled as host code: Lay::PackedActors admits exactly the five
    `Composite, Actors, F32` rows (render.hip: packed_lay, launch_row)."""
    import __graft_entry__ as ge

    src, exe = tmp_path / "rule.cpp", tmp_path / "rule"
    src.write_text(RULE)
    subprocess.run([ge.HIPCC, "-x", "c++", "-std=c++17", "-I", os.path.dirname(VARIANTS), str(src), "-o", str(exe)], check=True,
                   capture_output=True, timeout=300)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    admitted = {(int(L), int(F), int(H), o, s, p) for L, F, H, o, s, p in (l.split() for l in lines if l.strip())}
    want = {r for r in variant_rows() if r[3] == "Composite" and r[4] == "Actors" and r[5] == "F32"}
    assert admitted == want and len(want) == 5
    assert {(L, F, H) for L, F, H, o, s, p in want} == set(PA.SHAPES) == gate_constants()["_FUSED_ACTOR_FIELDS"]


CHILD = r'''
from neurad_studio_amd import _lib
from neurad_studio_amd.cameras.rays import RayBundle
from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler


def raised(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return [type(e).__name__, str(e)]
    return None


out = {"gate": {}, "errors": {}}
for L, F, H in ((8, 4, 32), (8, 4, 64), (16, 2, 64), (4, 2, 32), (4, 2, 64)):
    f = NeuRADField(field_config(L, F, H), actors=make_actors(), static_scale=100.0)
    out["gate"][f"actors {L} {F} {H}"] = [f.fused_packed_actors_supported(), f.fused_packed_supported()]
    out["gate"][f"static {L} {F} {H}"] = [NeuRADField(field_config(L, F, H), actors=None, static_scale=100.0).fused_packed_actors_supported(), None]
for L, F, H in ((4, 8, 32), (1, 4, 32), (8, 2, 64), (16, 2, 32), (3, 8, 32)):
    f = NeuRADField(field_config(L, F, H), actors=make_actors(), static_scale=100.0)
    out["gate"][f"other {L} {F} {H}"] = [f.fused_packed_actors_supported(), f.fused_packed_supported()]
out["version"] = _lib.load().nrhip_version()
out["prototypes"] = [n in _lib.PROTOTYPES for n in ("nrhip_occgrid_march_levels_actors", "nrhip_render_fwd_packed_actors")]


class Grid:  # a grid object from before the keyword
    def sampling(self, rays_o, rays_d, sigma_fn=None, alpha_fn=None, near_plane=0.0, far_plane=1e10, t_min=None, t_max=None,
                 render_step_size=1e-3, early_stop_eps=1e-4, alpha_thre=0.0, stratified=False, cone_angle=0.0):
        raise AssertionError("a march that knows nothing of the boxes must not run")


z = torch.zeros
sampler = VolumetricSampler(Grid()).eval()
with_actors = NeuRADField(field_config(8, 4, 32), actors=make_actors(), static_scale=100.0).eval()
static = NeuRADField(field_config(8, 4, 32), actors=None, static_scale=100.0).eval()
timed = RayBundle(origins=z(2, 3), directions=z(2, 3), pixel_area=z(2, 1), times=z(2, 1))
untimed = RayBundle(origins=z(2, 3), directions=z(2, 3), pixel_area=z(2, 1))
for name, call in (("render", sampler.render), ("render_train", sampler.render_train)):
    out["errors"][f"{name} no times"] = raised(lambda: call(with_actors, untimed, 0.1, actor_boxes=True))
    out["errors"][f"{name} no actors"] = raised(lambda: call(static, timed, 0.1, actor_boxes=True))
out["errors"]["forward no times"] = raised(lambda: sampler(untimed, 0.1, actor_boxes=True, field=with_actors))
print(json.dumps(out))
'''


def test_gate_version_and_argument_errors():
    res = run_child(CHILD)
    for k, (actors_gate, static_gate) in res["gate"].items():
        assert actors_gate == k.startswith("actors"), k
        assert not static_gate, k  # fused_packed_supported stays False for actor fields
    assert res["version"] >= 518 and res["prototypes"] == [True, True]
    for k, e in res["errors"].items():
        assert e and e[0] == "ValueError" and "actor_boxes=True" in e[1], (k, e)
        assert ("times" in e[1]) == k.endswith("no times") and ("no dynamic actors" in e[1]) == k.endswith("no actors"), (k, e)


def test_a_grid_without_the_keyword_is_refused():
    """a grid object whose `sampling` does not take `actor_boxes`: a clear error, not a silent static march (the candidate
    lists need a GPU, so the check is asked directly)"""
    from neurad_studio_amd.cameras.rays import RayBundle
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    import pytest
    import torch

    class Grid:
        def sampling(self, rays_o, rays_d, **kw):
            raise AssertionError("must not run")

        def sampling_old(self, rays_o, rays_d, sigma_fn=None, alpha_fn=None, render_step_size=1e-3):
            raise AssertionError("must not run")

    g = Grid()
    g.sampling = g.sampling_old
    z = torch.zeros
    rb = RayBundle(origins=z(2, 3), directions=z(2, 3), pixel_area=z(2, 1), times=z(2, 1))
    with pytest.raises(TypeError, match="actor_boxes"):
        VolumetricSampler(g)._march(rb, 0.1, 0.0, None, 0.0, 0.0, actor_boxes=(None, None))


# ---- the march rule against itself ------------------------------------------------------------------------------------
def _case(name, levels, n_rays=24):
    s = PA.scene(name)
    o, d, times = s["o"][:n_rays], s["d"][:n_rays], s["times"][:n_rays]
    ap = PA.oracle_actor_params(name)
    boxes = PA.level_boxes(s["box0"], levels)
    binaries = PA.random_binaries(levels, 16, 5)
    box_fn = lambda ri, ts, te: PA.in_box(ap, o, d, times, ri, ts, te)  # noqa: E731
    return o, d, boxes, binaries, box_fn, dict(near_plane=0.1, far_plane=120.0), 2 * s["step"]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_march_rule_restatement_against_itself():
    for name in ("golden", "street"):
        for levels in (1, 3):
            o, d, boxes, binaries, box_fn, kw, step = _case(name, levels)
            every = PA.march_boxes(boxes, np.ones_like(binaries), o, d, step, None, **kw)
            plain = PA.march_boxes(boxes, binaries, o, d, step, None, **kw)
            got = PA.march_boxes(boxes, binaries, o, d, step, box_fn, **kw)
            inside = box_fn(*every)
            cell = np.isin(PA.sample_keys(every[0], every[1]), PA.sample_keys(plain[0], plain[1]))
            classes = PA.march_classes(cell, inside)
            print(name, levels, "cell only / box only / both / neither:", classes)
            assert all(c > 0 for c in classes), (name, levels, classes)
            assert _same(got, [a[cell | inside] for a in every])
            # no candidates: the plain march (one level: occgrid_oracle's own)
            if levels == 1:
                assert _same(plain, OO.occgrid_march(boxes[0], binaries[0], o, d, step, **kw))
            assert _same(PA.march_boxes(boxes, binaries, o, d, step, lambda ri, ts, te: np.zeros(ri.shape, bool), **kw), plain)
            # all-zero binaries: only the in-box intervals survive; all-one binaries: the plain march on them
            empty = PA.march_boxes(boxes, np.zeros_like(binaries), o, d, step, box_fn, **kw)
            assert _same(empty, [a[inside] for a in every]) and empty[0].shape[0] > 0
            assert _same(PA.march_boxes(boxes, np.ones_like(binaries), o, d, step, box_fn, **kw), every)
