"""Host side of the fused render kernel on packed samples (NeuRADField.render_packed / fused_packed_supported and the
packed instantiation set of csrc/render_variants.h).  No GPU.

The field checks run in a child process, as tests/test_fused_shapes_gate.py does: importing the field module binds
FieldHeadNames for the whole process."""
import os
import subprocess

from host_gate import VARIANTS, gate_constants, run_child, variant_rows

CHILD = r'''
from neurad_studio_amd.fields.neurad_field import _FUSED_GRIDS


def raised(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return [type(e).__name__, str(e)]
    return None


out = {"gate": {}, "errors": {}}
for L, F in _FUSED_GRIDS:
    for H in (32, 64):
        out["gate"][f"static {L} {F} {H}"] = NeuRADField(field_config(L, F, H), actors=None, static_scale=100.0).fused_packed_supported()
for L, F, H in ((8, 4, 32), (4, 2, 32), (16, 2, 64)):  # shapes the ACTOR kernels exist for: still no packed kernel
    out["gate"][f"actors {L} {F} {H}"] = NeuRADField(field_config(L, F, H), actors=make_actors(), static_scale=100.0).fused_packed_supported()
for L, F, H in ((3, 8, 32), (4, 2, 48)):
    out["gate"][f"other {L} {F} {H}"] = NeuRADField(field_config(L, F, H), actors=None, static_scale=100.0).fused_packed_supported()

f = NeuRADField(field_config(8, 4, 32), actors=None, static_scale=100.0).eval()
z = torch.zeros
o, d, a, ts, te = z(2, 3), z(2, 3), z(2), z(5), z(5)
seg, ri = torch.tensor([0, 2, 5]), torch.tensor([0, 0, 1, 1, 1])
with torch.no_grad():
    out["errors"]["both"] = raised(lambda: f.render_packed(o, d, a, ts, te, segments=seg, ray_indices=ri, num_rays=2))
    out["errors"]["neither"] = raised(lambda: f.render_packed(o, d, a, ts, te))
    out["errors"]["no num_rays"] = raised(lambda: f.render_packed(o, d, a, ts, te, ray_indices=ri))
    # past the argument checks the HIP path refuses CPU tensors: there is no fallback
    out["errors"]["cpu"] = raised(lambda: f.render_packed(o, d, a, ts, te, segments=seg))
    g = NeuRADField(field_config(8, 4, 32), actors=make_actors(), static_scale=100.0).eval()
    out["errors"]["actors"] = raised(lambda: g.render_packed(o, d, a, ts, te, segments=seg))
out["errors"]["grad"] = raised(lambda: f.render_packed(o, d, a, ts, te, segments=seg))
print(json.dumps(out))
'''


def test_packed_gate_and_argument_errors():
    res = run_child(CHILD)
    gate = res["gate"]
    assert len([k for k in gate if k.startswith("static")]) == 14
    for k, v in gate.items():
        assert v == k.startswith("static"), k
    err = res["errors"]
    for k in ("both", "neither", "no num_rays"):
        assert err[k] and err[k][0] == "ValueError", (k, err[k])
    assert err["grad"] and err["grad"][0] == "RuntimeError" and "no_grad" in err["grad"][1]
    assert err["actors"] and err["actors"][0] == "NotImplementedError" and "operator path" in err["actors"][1]
    assert err["cpu"] and err["cpu"][0] == "NeuradHipError"


RULE = r'''
#include <cstdio>
#include "render_variants.h"
using namespace nrhip;
int main() {
#define X(L_, F_, H_, O_, S_, P_)                                                     \
  if (render_variant_ok(L_, F_, Out::O_, Src::S_, Prod::P_, Lay::Packed))             \
    std::printf("%d %d %d %s %s %s\n", L_, F_, H_, #O_, #S_, #P_);
  NRHIP_RENDER_VARIANTS(X)
  return 0;
}
'''


def test_packed_instantiations_are_the_composited_static_rows(tmp_path):
    """The dispatcher instantiates the packed layout for exactly the rows render_variant_ok(..., Lay::Packed) admits
    (render.hip: launch_row).  The rule itself is asked -- the header compiled as host code -- and must pick the
    `Composite, Static` rows with F32 or F16Pairs products: 14 + 6, every fused grid at both widths among them."""
    import __graft_entry__ as ge

    src, exe = tmp_path / "rule.cpp", tmp_path / "rule"
    src.write_text(RULE)
    subprocess.run([ge.HIPCC, "-x", "c++", "-std=c++17", "-I", os.path.dirname(VARIANTS), str(src), "-o", str(exe)], check=True,
                   capture_output=True, timeout=300)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    admitted = {(int(L), int(F), int(H), o, s, p) for L, F, H, o, s, p in (l.split() for l in lines if l.strip())}
    rows = variant_rows()
    want = {r for r in rows if r[3] == "Composite" and r[4] == "Static" and r[5] in ("F32", "F16Pairs")}
    assert admitted == want
    assert len([r for r in want if r[5] == "F32"]) == 14 and len([r for r in want if r[5] == "F16Pairs"]) == 6
    assert {(L, F) for L, F, H, o, s, p in want if p == "F32"} == gate_constants()["_FUSED_GRIDS"]
    assert {H for L, F, H, o, s, p in want} == {32, 64}
