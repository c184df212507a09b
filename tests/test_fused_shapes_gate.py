"""Which fields the fused kernels take (NeuRADField.fused_supported and the model's fused paths): the static grids with
L * F <= 32 that render.hip is instantiated for, and with dynamic actors only the (L, F, H) its actor and override kernels
exist for.  Host logic only: no GPU.

The checks run in a child process: importing the field module binds FieldHeadNames for the whole process (the
reference's own enum when nerfstudio is importable, field_components/field_heads.py), which other tests pin."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys
import torch
from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig
from neurad_studio_amd.models.neurad import NeuRADHotPath, NeuRADHotPathConfig


def field_config(L, F, H):
    cfg = NeuRADFieldConfig(geo_hidden_dim=H, nff_hidden_dim=H)
    st, ac = cfg.grid.static, cfg.grid.actor
    st.num_levels, st.hashgrid_dim, st.log2_hashmap_size = L, F, 10
    ac.num_levels, ac.hashgrid_dim, ac.log2_hashmap_size = min(2, L), F, 8  # the actor grids share F (the default)
    return cfg


def make_actors():
    p = torch.eye(4).repeat(2, 1, 1)
    p[:, :3, 3] = torch.tensor([10.0, 0.0, 0.5])
    traj = {"timestamps": torch.tensor([0.0, 1.0]), "poses": p, "dims": torch.tensor([2.0, 4.5, 1.6]),
            "symmetric": torch.tensor(True), "deformable": torch.tensor(False)}
    return DynamicActors(DynamicActorsConfig(), trajectories=[traj])


out = {}
for kind, L, F, H in json.loads(sys.argv[1]):
    if kind == "model":
        c = NeuRADHotPathConfig(appearance_dim=0)
        c.field = field_config(L, F, H)
        for pf in (c.sampling.proposal_field_1, c.sampling.proposal_field_2):
            pf.grid.static.log2_hashmap_size, pf.grid.actor.log2_hashmap_size = 10, 8
        m = NeuRADHotPath(c, static_scale=100.0, actors=make_actors()).eval()
        with torch.no_grad():
            ev = m.fused_eval_possible()
        m.train()
        out[f"{kind} {L} {F} {H}"] = [ev, m.fused_training_possible()]
    else:
        f = NeuRADField(field_config(L, F, H), actors=make_actors() if kind == "actors" else None, static_scale=100.0)
        out[f"{kind} {L} {F} {H}"] = [f.fused_supported(), f.fused_supported(with_actors=True)]
print(json.dumps(out))
'''


def gate(cases):
    """-> {"kind L F H": [..]} from a fresh interpreter"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(cases)], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


STATIC = [(1, 4, 32), (1, 4, 64), (4, 2, 32), (4, 2, 64), (4, 4, 32), (4, 4, 64), (8, 2, 32), (8, 2, 64), (8, 4, 32),
          (16, 2, 64), (4, 8, 32)]
OTHER = [(3, 8, 32), (2, 2, 32), (4, 2, 48), (8, 8, 32)]
WITH_ACTORS = [(4, 2, 32), (4, 2, 64), (8, 4, 32), (8, 4, 64), (16, 2, 64)]  # dispatch_render_actors / the ovr kernel


def test_static_grids_take_the_fused_kernels_where_they_are_instantiated():
    res = gate([["static", *c] for c in STATIC + OTHER])
    for c in STATIC:
        assert res["static %d %d %d" % c] == [True, True], c
    for c in OTHER:
        assert res["static %d %d %d" % c] == [False, False], c


def test_fields_with_actors_take_the_fused_kernels_only_where_they_exist():
    """4 x 4 (num_levels = 4 at the default hashgrid_dim) and 4 x 8 have 4 levels like NeuRAD tiny's 4 x 2, but no
    actor kernel: they keep the operator-level path"""
    cases = [(4, 4, 32), (4, 4, 64), (4, 8, 32), (4, 8, 64), (1, 4, 32), (8, 2, 32), (16, 2, 32)] + WITH_ACTORS
    res = gate([["actors", *c] for c in cases])
    for c in cases:
        # the static-scene kernels never take a scene with actors; the actor kernels exist for WITH_ACTORS only
        assert res["actors %d %d %d" % c] == [False, c in WITH_ACTORS], c


@pytest.mark.parametrize("L,F", [(4, 4), (4, 8), (4, 2)])
def test_model_fused_paths_with_actors(L, F):
    res = gate([["model", L, F, 32]])
    want = (L, F) == (4, 2)
    assert res[f"model {L} {F} 32"] == [want, want]
