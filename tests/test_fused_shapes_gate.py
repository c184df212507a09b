"""Which fields the fused kernels take (NeuRADField.fused_supported and the model's fused paths): the static grids with
L * F <= 32 that render.hip is instantiated for, and with dynamic actors only the (L, F, H) its actor and override kernels
exist for.  Host logic only: no GPU.

The checks run in a child process: importing the field module binds FieldHeadNames for the whole process (the
reference's own enum when nerfstudio is importable, field_components/field_heads.py), which other tests pin."""
import ast
import json
import os
import re
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
WITH_ACTORS = [(4, 2, 32), (4, 2, 64), (8, 4, 32), (8, 4, 64), (16, 2, 64)]  # the actor and override kernels


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


# ---- the gate's constants against the kernels' variant table -------------------------------------------------------------
VARIANTS = os.path.join(ROOT, "neurad_studio_amd", "csrc", "render_variants.h")
FIELD_PY = os.path.join(ROOT, "neurad_studio_amd", "fields", "neurad_field.py")


def variant_rows(path=VARIANTS):
    """-> [(L, F, H, output, source, products)] of the X-macro, comments dropped"""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    table = src[src.index("#define NRHIP_RENDER_VARIANTS(X)"):]
    return [(int(L), int(F), int(H), o, s, p)
            for L, F, H, o, s, p in re.findall(r"\bX\(\s*(\d+),\s*(\d+),\s*(\d+),\s*(\w+),\s*(\w+),\s*(\w+)\s*\)", table)]


def gate_constants():
    """_FUSED_GRIDS / _FUSED_ACTOR_FIELDS read from the module's source (importing it binds FieldHeadNames: see the top)"""
    out = {}
    for node in ast.parse(open(FIELD_PY).read()).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") in ("_FUSED_GRIDS", "_FUSED_ACTOR_FIELDS"):
            out[node.targets[0].id] = set(ast.literal_eval(node.value))
    return out


def check_gate_against_table(rows, consts):
    assert len(rows) == len(set(rows)) > 0, "duplicate or no rows"
    assert {r[3] for r in rows} <= {"PerSample", "Composite"} and {r[4] for r in rows} <= {"Static", "EvalTable", "Actors", "Overrides"}
    assert {r[5] for r in rows} <= {"F32", "Bf16Split", "F16Pairs"}
    have = set(rows)
    plain = {(L, F) for L, F, H, o, s, p in rows if (s, p) == ("Static", "F32")}
    # a static grid is fused when the plain kernel exists for both outputs at both hidden widths -- and no plain row is a stray
    whole = {(L, F) for L, F in plain
             if all((L, F, H, o, "Static", "F32") in have for H in (32, 64) for o in ("PerSample", "Composite"))}
    assert whole == plain == consts["_FUSED_GRIDS"], (whole ^ consts["_FUSED_GRIDS"], plain ^ whole)
    assert {H for L, F, H, o, s, p in rows if (s, p) == ("Static", "F32")} == {32, 64}
    actors = {(L, F, H) for L, F, H, o, s, p in rows if s == "Actors"}
    overrides = {(L, F, H) for L, F, H, o, s, p in rows if s == "Overrides"}
    assert actors == overrides == consts["_FUSED_ACTOR_FIELDS"], (actors ^ overrides, actors ^ consts["_FUSED_ACTOR_FIELDS"])
    # the dispatcher's last candidate: every row has the plain kernel of its (L, F, H, output) behind it
    for L, F, H, o, s, p in rows:
        assert (L, F, H, o, "Static", "F32") in have, (L, F, H, o, s, p)


def test_gate_constants_follow_the_variant_table():
    rows = variant_rows()
    assert len(rows) == 54  # one launch case per row, fp32 and fp16 tables each: render.hip's 108 render_kernel instantiations
    check_gate_against_table(rows, gate_constants())


def test_gate_check_notices_a_missing_row():
    """the check above has teeth: any single row taken out of the table breaks it, unless that row is an optional variant
    (eval table, pair / split products) the dispatcher merely prefers"""
    rows, consts = variant_rows(), gate_constants()
    for i, r in enumerate(rows):
        optional = r[4] == "EvalTable" or r[5] != "F32"
        try:
            check_gate_against_table(rows[:i] + rows[i + 1:], consts)
            noticed = False
        except AssertionError:
            noticed = True
        assert noticed != optional, r
