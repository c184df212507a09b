"""Host-side test helpers that need no GPU: the C header's declarations, the render kernels' variant table, the fused
gate's constants read from source, and a runner for checks that need a fresh interpreter (importing the field module binds
FieldHeadNames for the whole process -- the reference's own enum when nerfstudio is importable -- which other tests pin)."""
import ast
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "neurad_hip.h")
VARIANTS = os.path.join(ROOT, "neurad_studio_amd", "csrc", "render_variants.h")
FIELD_PY = os.path.join(ROOT, "neurad_studio_amd", "fields", "neurad_field.py")

# what a child source starts with: the imports, a field config of a given shape and one parked actor
CHILD_PRELUDE = r'''
import json, sys
import torch
from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig


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

'''


def run_child(source, *args):
    """run `source` (after CHILD_PRELUDE) in a fresh interpreter -> its last output line, parsed as JSON"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    r = subprocess.run([sys.executable, "-c", CHILD_PRELUDE + source, *args], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|const char\*)\s+(nrhip_\w+)\s*\(", src)))


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
