"""Host side of the fused training node for packed samples of a scene with dynamic actors: the PackedRowsOvr instantiation
set of csrc/render_variants.h, the field's gate, the ABI version and prototypes, the argument errors of
``render_train_packed(..., times=...)``, the sampler's default routing and the device check of the new ``ops`` wrappers.
No GPU.

The field checks run in a child process, as tests/test_render_packed_actors_host.py does."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

import packed_actor_refs as PA
from host_gate import VARIANTS, gate_constants, header_functions, run_child, variant_rows

NEW = ["nrhip_field_fwd_train_packed_ovr", "nrhip_actor_find_packed", "nrhip_actor_pair_positions_fwd_packed",
       "nrhip_actor_pair_positions_bwd_packed"]

RULE = r'''
#include <cstdio>
#include "render_variants.h"
using namespace nrhip;
int main() {
  const Lay lays[] = {Lay::Dense, Lay::Packed, Lay::PackedRows, Lay::PackedActors, Lay::PackedRowsOvr};
  const char* names[] = {"Dense", "Packed", "PackedRows", "PackedActors", "PackedRowsOvr"};
  for (int k = 0; k < 5; ++k) {
#define X(L_, F_, H_, O_, S_, P_)                                              \
  if (render_variant_ok(L_, F_, Out::O_, Src::S_, Prod::P_, lays[k]))          \
    std::printf("%s %d %d %d %s %s %s\n", names[k], L_, F_, H_, #O_, #S_, #P_);
    NRHIP_RENDER_VARIANTS(X)
#undef X
  }
  return 0;
}
'''


def test_packed_override_instantiations_are_the_override_rows(tmp_path):
    """The rule itself is asked -- the header compiled as host code: Lay::PackedRowsOvr admits exactly the five
    `PerSample, Overrides, F32` rows (render.hip: packed_lay, launch_row); Packed, PackedRows and PackedActors admit what
    they admitted before, and every row is still a dense kernel."""
    import __graft_entry__ as ge

    src, exe = tmp_path / "rule.cpp", tmp_path / "rule"
    src.write_text(RULE)
    subprocess.run([ge.HIPCC, "-x", "c++", "-std=c++17", "-I", os.path.dirname(VARIANTS), str(src), "-o", str(exe)], check=True,
                   capture_output=True, timeout=300)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    admitted = {}
    for lay, L, F, H, o, s, p in (l.split() for l in lines if l.strip()):
        admitted.setdefault(lay, set()).add((int(L), int(F), int(H), o, s, p))
    rows = set(variant_rows())
    pick = lambda o, s, prods: {r for r in rows if r[3] == o and r[4] == s and r[5] in prods}  # noqa: E731
    want = pick("PerSample", "Overrides", ("F32",))
    assert admitted["PackedRowsOvr"] == want and len(want) == 5
    assert {(L, F, H) for L, F, H, o, s, p in want} == set(PA.SHAPES) == gate_constants()["_FUSED_ACTOR_FIELDS"]
    assert admitted["Dense"] == rows
    assert admitted["Packed"] == pick("Composite", "Static", ("F32", "F16Pairs"))
    assert admitted["PackedRows"] == pick("PerSample", "Static", ("F32",))
    assert admitted["PackedActors"] == pick("Composite", "Actors", ("F32",)) and len(admitted["PackedActors"]) == 5


def test_header_declares_and_prototypes_list_the_entry_points():
    from neurad_studio_amd import _lib

    declared = header_functions()
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES, name
    lib = _lib.load()
    assert lib.nrhip_version() >= 519
    for name in NEW:
        assert hasattr(lib, name), name


I32, I64, F32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
ONE = ctypes.c_void_p(0x1000)  # any non-null address: validation fails before anything is dereferenced
INVALID_ARG, UNSUPPORTED = 1, 2  # NRHIP_ERR_INVALID_ARG, NRHIP_ERR_UNSUPPORTED


def _field(L=8, F=4, H=32):
    """an nrhip_field the validation accepts; every pointer is the same non-null address"""
    from neurad_studio_amd import _lib

    f = _lib.Field()
    g = f.grid
    g.num_levels, g.n_features, g.log2_table_size, g.param_dtype = L, F, 11, 0
    for l in range(L):
        g.scalings[l] = 16.0 * 2 ** l
    f.table, f.static_scale, f.use_sdf, f.beta = 0x1000, 100.0, 1, 3.0
    f.geo.in_dim, f.geo.hidden_dim, f.geo.out_dim, f.geo.num_layers = L * F, H, 33, 2
    f.feat.in_dim, f.feat.hidden_dim, f.feat.out_dim, f.feat.num_layers = 48, H, 32, 3
    for k in range(3):
        f.geo.weight[k] = f.geo.bias[k] = f.feat.weight[k] = f.feat.bias[k] = 0x1000
    return f


def _actors():
    from neurad_studio_amd import _lib

    a = _lib.Actors()
    a.n_times, a.n_actors, a.actor_scale, a.max_candidates = 2, 3, 10.0, 3
    a.timestamps = a.positions = a.rotations_6d = a.present = a.bounds = a.tables = 0x1000
    return a


def _rays(r, m, ptr=0x1000, seg=0x1000):
    from neurad_studio_amd import _lib

    p = _lib.PackedRays()
    p.n_rays, p.n_samples = r, m
    p.origins = p.directions = p.pixel_area = p.t_starts = p.t_ends = ptr
    p.segments = seg
    return p


def test_host_side_validation_and_no_ops():
    """the argument checks of the four entry points run on the host before any launch: n_rays == 0 and n_samples == 0 are
    no-ops that read no pointer, n_samples >= 2^31 is NRHIP_ERR_UNSUPPORTED, NULL arrays and unaligned rows are refused"""
    from neurad_studio_amd import _lib

    lib = _lib.load()
    f, a, o, n = _field(), _actors(), ONE, None
    err = lib.nrhip_last_error
    ovr = lambda rays, row=o, rows=o, dirs=o, out=(o,) * 7: lib.nrhip_field_fwd_train_packed_ovr(  # noqa: E731
        f, rays, row, rows, dirs, *out, None)
    empty = _rays(0, 0, ptr=None, seg=None)
    assert ovr(empty, n, n, n, (n,) * 7) == 0 and ovr(_rays(5, 0, ptr=None, seg=None), n, n, n, (n,) * 7) == 0
    assert ovr(_rays(4, 1 << 31)) == UNSUPPORTED and b"2^31" in err()
    assert ovr(_rays(4, -8)) == INVALID_ARG and b"negative" in err()
    assert ovr(_rays(4, 8, seg=None)) == INVALID_ARG and b"NULL pointer" in err()
    for k in range(3):
        args = [o, o, o]
        args[k] = None
        assert ovr(_rays(4, 8), *args) == INVALID_ARG and b"NULL pointer" in err(), k
    assert ovr(_rays(4, 8), rows=ctypes.c_void_p(0x1004)) == INVALID_ARG and b"aligned" in err()
    for k in range(7):
        out = [o] * 7
        out[k] = None
        assert ovr(_rays(4, 8), out=out) == INVALID_ARG and b"NULL output" in err(), k
    assert lib.nrhip_field_fwd_train_packed_ovr(_field(4, 8, 32), _rays(4, 8), o, o, o, *(o,) * 7, None) == UNSUPPORTED

    find = lambda rays, ri=o, cand=(o, o, o), outs=(o, o, o): lib.nrhip_actor_find_packed(  # noqa: E731
        a, rays, ri, *cand, *outs, None, None)
    assert find(empty, n, (n, n, n), (n, n, n)) == 0 and find(_rays(5, 0, ptr=None, seg=None), n, (n, n, n), (n, n, n)) == 0
    assert find(_rays(4, 1 << 31)) == UNSUPPORTED and b"2^31" in err()
    assert find(_rays(4, 8), ri=None) == INVALID_ARG and find(_rays(4, 8), outs=(n, o, o)) == INVALID_ARG
    assert find(_rays(4, 8, ptr=None)) == INVALID_ARG and lib.nrhip_actor_find_packed(None, _rays(4, 8), *(o,) * 7, None, None) == INVALID_ARG

    fwd = lambda rays, p, ptrs=(o,) * 6: lib.nrhip_actor_pair_positions_fwd_packed(  # noqa: E731
        a, rays, ptrs[0], ptrs[1], ptrs[2], ptrs[3], None, I64(p), ptrs[4], ptrs[5], None)
    bwd = lambda rays, p, ptrs=(o,) * 8: lib.nrhip_actor_pair_positions_bwd_packed(  # noqa: E731
        a, rays, ptrs[0], ptrs[1], ptrs[2], ptrs[3], None, I64(p), *ptrs[4:], None)
    for call, k_ptrs in ((fwd, 6), (bwd, 8)):
        assert call(_rays(4, 8), 0, (n,) * k_ptrs) == 0  # no pairs: a no-op that reads no pointer
        assert call(_rays(4, 8), -1) == INVALID_ARG
        assert call(_rays(0, 0, ptr=None, seg=None), 5) == INVALID_ARG and b"without samples" in err()
        assert call(_rays(4, 1 << 31), 5) == UNSUPPORTED
        for k in range(k_ptrs):
            ptrs = [o] * k_ptrs
            ptrs[k] = None
            assert call(_rays(4, 8), 5, ptrs) == INVALID_ARG and b"NULL pointer" in err(), k


CHILD = r'''
from neurad_studio_amd import _lib


def raised(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return [type(e).__name__, str(e)]
    return None


out = {"gate": {}, "errors": {}}
for L, F, H in ((8, 4, 32), (8, 4, 64), (16, 2, 64), (4, 2, 32), (4, 2, 64)):
    f = NeuRADField(field_config(L, F, H), actors=make_actors(), static_scale=100.0)
    out["gate"][f"actors {L} {F} {H}"] = [f.fused_packed_actors_train_supported(), f.fused_packed_train_supported()]
    s = NeuRADField(field_config(L, F, H), actors=None, static_scale=100.0)
    out["gate"][f"static {L} {F} {H}"] = [s.fused_packed_actors_train_supported(), None]
for L, F, H in ((4, 8, 32), (1, 4, 32), (8, 2, 64), (16, 2, 32), (3, 8, 32)):
    f = NeuRADField(field_config(L, F, H), actors=make_actors(), static_scale=100.0)
    out["gate"][f"other {L} {F} {H}"] = [f.fused_packed_actors_train_supported(), f.fused_packed_train_supported()]
f = NeuRADField(field_config(8, 4, 32), actors=make_actors(), static_scale=100.0)
f.mlp_feature.layers[1].bias = None
out["gate"]["nobias 8 4 32"] = [f.fused_packed_actors_train_supported(), f.fused_packed_train_supported()]

z = torch.zeros
fld = NeuRADField(field_config(8, 4, 32), actors=make_actors(), static_scale=100.0).train()
o, d, a, t = z(2, 3), z(2, 3), z(2), z(2)
ts, te = z(4), z(4)
seg, ri = torch.tensor([0, 2, 4]), torch.tensor([0, 0, 1, 1])
call = fld.render_train_packed
out["errors"]["both"] = raised(lambda: call(o, d, a, ts, te, segments=seg, ray_indices=ri, num_rays=2, times=t))
out["errors"]["neither"] = raised(lambda: call(o, d, a, ts, te, times=t))
out["errors"]["no num_rays"] = raised(lambda: call(o, d, a, ts, te, ray_indices=ri, times=t))
og = z(2, 3, requires_grad=True)
out["errors"]["rays need grad"] = raised(lambda: call(og, d, a, ts, te, segments=seg, times=t))
out["errors"]["rays need grad, ray_gradients"] = raised(lambda: call(og, d, a, ts, te, segments=seg, times=t, ray_gradients=True))
out["errors"]["no times"] = raised(lambda: call(o, d, a, ts, te, segments=seg))
out["errors"]["no times, ray_gradients"] = raised(lambda: call(og, d, a, ts, te, segments=seg, ray_gradients=True))
other = NeuRADField(field_config(4, 8, 32), actors=make_actors(), static_scale=100.0).train()
out["errors"]["other shape"] = raised(lambda: other.render_train_packed(o, d, a, ts, te, segments=seg, times=t))
out["version"] = _lib.load().nrhip_version()
print(json.dumps(out))
'''


def test_gate_version_and_argument_errors():
    res = run_child(CHILD)
    for k, (actors_gate, static_gate) in res["gate"].items():
        assert actors_gate == k.startswith("actors"), k
        assert not static_gate, k  # fused_packed_train_supported stays False for actor fields
    assert res["version"] >= 519
    e = res["errors"]
    for k in ("both", "neither"):
        assert e[k] and e[k][0] == "ValueError" and "exactly one of segments / ray_indices" in e[k][1], (k, e[k])
    assert e["no num_rays"] and e["no num_rays"][0] == "ValueError" and "num_rays" in e["no num_rays"][1]
    for k in ("rays need grad", "rays need grad, ray_gradients", "no times", "no times, ray_gradients", "other shape"):
        assert e[k] and e[k][0] == "NotImplementedError" and "operator route" in e[k][1], (k, e[k])
    for k in ("rays need grad", "rays need grad, ray_gradients"):
        assert "rays" in e[k][1] and "actor" in e[k][1], (k, e[k])


def test_sampler_keyword_defaults_to_off():
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler

    p = inspect.signature(VolumetricSampler.render_train).parameters
    assert p["fused_actor_training"].default is False
    assert p["actor_boxes"].default is False and p["fused_ray_gradients"].default is False
    assert "no fused training node with actors" not in VolumetricSampler.render_train.__doc__


def test_new_wrappers_refuse_cpu_tensors():
    from neurad_studio_amd import _lib, ops

    z = torch.zeros
    o, d, a, t = z(2, 3), z(2, 3), z(2), z(2)
    ts, te, ri = z(4), z(4), torch.tensor([0, 0, 1, 1])
    si, ai = torch.tensor([1]), torch.tensor([0], dtype=torch.int32)
    cand = (z(2, dtype=torch.int32), z(2, 1, dtype=torch.int32), z(2, 1, 12), None)
    with pytest.raises(_lib.NeuradHipError, match="GPU tensor"):
        ops.actor_find_packed(None, cand, o, d, a, ts, te, ri)
    with pytest.raises(_lib.NeuradHipError, match="GPU tensor"):
        ops.actor_pair_positions_packed(None, o, d, a, ts, te, ri, t, si, ai)
    with pytest.raises(_lib.NeuradHipError, match="GPU tensor"):
        ops.actor_pair_positions_packed_bwd(None, o, d, a, ts, te, ri, t, si, ai, None, z(1, 3), z(1))
    with pytest.raises(_lib.NeuradHipError, match="GPU tensor"):
        ops.field_fwd_train_packed(None, o, d, a, ts, te, torch.tensor([0, 2, 4]),
                                   override=(z(4, dtype=torch.int32), z(1, 32), z(1, 3)))
