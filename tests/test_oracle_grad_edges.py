"""Pin the position-gradient references at the exact edges of the contraction and the feature rescale against the
REFERENCE's own fp32 autograd (tests/golden/ray_grads_edges.npz, oracle/make_golden_grad_edges.py), element by element:

  E1 |u|_inf tied on 2 or 3 axes outside the unit cube, E2 |u|_inf == 1, E3 2 scal_0 std' == 1 on an E2 sample.

The float64 derivatives of the oracle (static encoding) and of the float64 torch chain (actor pairs; the GPU tests use
both as references) must sit within the reference's own fp32 rounding of them, |ref - got| <= 2 u A + u |ref|, where A is
the float64 sum of |terms| of the element.  The wrong subgradients (whole dL/dm to the first maximal axis; no clamp
gradient at equality) must fall far outside that bound on the edge rows: the fixture really hits the edges."""
import numpy as np

import neurad_oracle as O
import synth
from conftest import load_golden
from grad_edge_refs import actor_case, edge_g_enc, edge_grid, excess

U = 2.0 ** -24
KINDS = {"control": 0, "E1": 1, "E2": 2, "E3": 3}


def test_static_edges_oracle_vs_reference_autograd():
    g = load_golden("ray_grads_edges")
    grid, sc = edge_grid(), float(g["static_scale"])
    args = (g["o"], g["d"], g["area"], g["starts"], g["ends"], edge_g_enc(g))
    go, gd, goa, gda = O.encode_static_ray_grads(grid, sc, *args, with_abs=True)
    # the edges are in the fixture, exactly
    mean, std = O.fast_isotropic_gaussian(g["o"], g["d"], g["area"], g["starts"], g["ends"])
    u = np.abs(mean / np.float32(sc))
    mag = u.max(-1)
    ties = ((u == mag[..., None]).sum(-1) >= 2) & (mag >= 1)
    k = g["kind"]
    assert ties[k == 1].all(1).sum() >= 40 and (((u == mag[..., None]).sum(-1) == 3) & (mag >= 1)).any()
    assert (mag[k >= 2] == 1).any(1).all() and not (mag[k == 0] == 1).any()
    _, cstd = O.contract_gaussian(mean, std, sc)
    a0 = (np.float32(32) * np.float32(2)) * cstd
    assert (a0[k == 3] == 1).any(1).all() and ((a0 == 1) & (mag == 1)).sum() == (k == 3).sum()
    for got, ref, A in ((go, g["enc_go"], goa), (gd, g["enc_gd"], gda)):
        assert excess(got, ref, A).max() <= 2.0, excess(got, ref, A).max()
    # the wrong subgradients are outside that bound on every edge kind they touch
    for ties_, clamp, kinds in (("first", True, (1, 2, 3)), ("split", False, (3,))):
        bo, bd = O.encode_static_ray_grads(grid, sc, *args, ties=ties_, clamp_at_one=clamp)
        for kk in kinds:
            worst = max(excess(bo, g["enc_go"], goa)[k == kk].max(), excess(bd, g["enc_gd"], gda)[k == kk].max())
            assert worst > 100.0, (ties_, clamp, kk, worst)
        assert excess(bo, g["enc_go"], goa)[k == 0].max() <= 2.0


def test_actor_edges_chain_vs_reference_autograd():
    g = load_golden("ray_grads_edges")
    out = actor_case(g)
    assert np.abs(out["x01"] - g["a_x01"]).max() < 2e-7 and np.abs(out["cstd"] / g["a_cstd"] - 1).max() < 1e-6
    assert (out["outside"] & (out["tied"] == 2)).sum() >= 10 and (out["outside"] & (out["tied"] == 3)).sum() >= 5
    assert (out["mag"] == 1).sum() >= 4
    for key, ref in (("dpos", "a_dpos"), ("drot", "a_drot"), ("go", "a_go"), ("gd", "a_gd")):
        e = excess(out[key], g[ref], out["A_" + key] if "A_" + key in out else out["A_g" + key[1]])
        assert e.max() <= 2.0 * 16, (key, e.max())
    bad = actor_case(g, ties="first")
    worst = max(excess(bad["go"], g["a_go"], out["A_go"]).max(), excess(bad["gd"], g["a_gd"], out["A_gd"]).max())
    assert worst > 1000.0, worst


def test_hashgrid_input_grads_vs_reference_autograd():
    """dL/dx of a plain HashEncoding, per element (golden field_actors_grads: the reference's autograd)"""
    g = load_golden("field_actors_grads")
    sc = O.hash_scalings(4, 64, 1024)
    gx, ga = O.hashgrid_input_grads(g["hx"], synth.hash_table(4 * 2**9, 4, seed=400, scale=0.7), sc, 2**9, g["hgy"],
                                    with_abs=True)
    assert excess(gx, g["hdx"], ga).max() <= 4.0
