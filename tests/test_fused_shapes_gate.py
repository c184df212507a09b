"""Which fields the fused kernels take (NeuRADField.fused_supported and the model's fused paths): the static grids with
L * F <= 32 that render.hip is instantiated for, and with dynamic actors only the (L, F, H) its actor and override kernels
exist for.  Host logic only: no GPU.

The checks run in a child process: importing the field module binds FieldHeadNames for the whole process (the
reference's own enum when nerfstudio is importable, field_components/field_heads.py), which other tests pin."""
import json

import pytest

from host_gate import gate_constants, run_child, variant_rows

CHILD = r'''
from neurad_studio_amd.models.neurad import NeuRADHotPath, NeuRADHotPathConfig

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
    return run_child(CHILD, json.dumps(cases))


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
