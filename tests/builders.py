"""The synthetic parameters and rays the fixtures under tests/golden/ were generated from, and the tests' variations of
them: one copy, on the CPU (numpy, torch on the CPU and the oracle).  The fixture generators (oracle/make_golden*.py,
scripts/make_golden_field_shapes.py) keep their own parameter code: they define the fixtures."""
import numpy as np
import torch

import neurad_oracle as O
import synth

# golden tag -> (L, min_res, max_res, log2_hashmap_size, F)
HASH_CFGS = {"c2small": (16, 16, 1024, 12, 2), "neurad": (8, 32, 8192, 12, 4), "prop": (6, 128, 4096, 11, 1),
             "tiny": (1, 32, 32, 10, 4), "actor": (4, 64, 1024, 10, 4)}

RENDER_CFGS = [  # (L, F, lg, min_res, max_res, H, use_sdf, R, S)
    (16, 2, 12, 16, 1024, 64, True, 37, 128),   # BASELINE config 2 shape (small table)
    (8, 4, 11, 32, 8192, 32, True, 50, 32),     # NeuRAD defaults
    (8, 4, 11, 32, 8192, 32, False, 21, 33),    # density head, ragged S (not a multiple of 16)
    (16, 2, 12, 16, 1024, 32, True, 5, 7),      # S < 16
    (8, 4, 11, 32, 8192, 64, False, 9, 1),      # single sample per ray
    (4, 8, 10, 64, 1024, 64, True, 13, 48),
]

# fixture tag -> (L, F, min_res, max_res, log2_hashmap_size, table seed); scripts/make_golden_field_shapes.py's SHAPES
SHAPES = {"tiny": (1, 4, 32, 32, 10, 53), "neurad_tiny": (4, 2, 32, 8192, 11, 57)}


def field_params(use_sdf=True, L=8, F=4, lg=11, H=32, mn=32, mx=8192, scale=0.5, seed=51):
    """The field of oracle/make_golden.py's golden_field (the defaults), or the same layer seeds on another grid: geo layer 0
    takes the L * F encoding columns, H is the width of both MLPs"""
    grid = O.GridParams(synth.hash_table(L * 2**lg, F, seed=seed, scale=scale), L, mn, mx, lg)
    gw, gb, fw, fb = [], [], [], []
    for k, (o, i) in enumerate([(H, L * F), (33, H)]):
        w, b = synth.linear(o, i, 200 + 10 * k)
        gw.append(w), gb.append(b)
    for k, (o, i) in enumerate([(H, 48), (H, H), (32, H)]):
        w, b = synth.linear(o, i, 300 + 10 * k)
        fw.append(w), fb.append(b)
    return O.FieldParams(grid, 100.0, gw, gb, fw, fb, use_sdf=use_sdf)


def tagged_field_params(tag, use_sdf=True, H=32):
    """the field of a SHAPES fixture; H = 64: the same grid with 64-wide MLPs (oracle-only shapes)"""
    L, F, mn, mx, lg, seed = SHAPES[tag]
    return field_params(use_sdf, L, F, lg, H, mn, mx, scale=0.5, seed=seed)


def shape_params(L, F, H, use_sdf, half=False):
    """an (L, F) grid with O(1) features and H-wide MLPs; fp16 storage: the oracle sees the rounded table"""
    lg, mn, mx = (10, 32, 32) if L == 1 else (10, 32, 2048)
    p = field_params(use_sdf, L, F, lg, H, mn, mx, scale=2.0 if use_sdf else 0.5, seed=60 + L + F)
    if half:
        p.grid.table = p.grid.table.astype(np.float16).astype(np.float32)
    if use_sdf:
        p.beta = 3.0  # alphas away from saturation: the compositing is exercised
    return p


def mlp_params(cfg):
    i, n, w, o = (int(v) for v in cfg)
    dims = [i] + [w] * (n - 1) + [o]
    ws, bs = [], []
    for k in range(n):
        wk, bk = synth.linear(dims[k + 1], dims[k], 100 + 10 * k)
        ws.append(wk), bs.append(bk)
    return ws, bs


def prop_params(seed, lg=11):
    w, _ = synth.linear(1, 6, seed + 1, bias=False)
    return O.ProposalParams(O.GridParams(synth.hash_table(6 * 2**lg, 1, seed=seed, scale=2.0), 6, 128, 4096, lg),
                            100.0, w + np.float32(0.3))


def actor_params(g, L=4, F=4):
    """the three actor grids of the actor fixtures: L = F = 4 (oracle/make_golden_actors.py), 2 x 2 for NeuRAD tiny"""
    grids = [O.GridParams(synth.hash_table(L * 2**9, F, seed=400 + i, scale=0.7), L, 64, 1024, 9) for i in range(3)]
    return O.ActorParams(g["timestamps"], g["positions"], g["rotations_6d"], g["present"], g["sizes"], g["padding"],
                         grids, actor_scale=10.0)


def sample_rays(R, S, seed, fars=200.0):
    """-> origins, directions, pixel areas, bin starts, bin ends, bin edges [R, S + 1]"""
    o, d, area, _ = synth.rays(R, seed)
    bins, eu, _ = O.power_sampler(np.zeros(R), np.full(R, fars, np.float32), S)
    return o, d, area, np.ascontiguousarray(eu[:, :-1]), np.ascontiguousarray(eu[:, 1:]), eu


def trajectories():
    """3 actors moving along +x (the scene of oracle/make_golden_actors.py): actor 2 overlaps actor 1's box, actor 0 is
    present early only"""
    ts_all = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0])
    out = []
    for a, (y0, yaw, dims, ts) in enumerate([(8.0, 0.3, (2.0, 4.5, 1.6), ts_all[:3]), (-6.0, -0.2, (2.1, 4.8, 1.7), ts_all),
                                             (-5.0, 0.1, (1.9, 4.2, 1.5), ts_all[1:])]):
        poses = []
        for t in ts:
            c, s = np.cos(yaw + 0.05 * float(t)), np.sin(yaw + 0.05 * float(t))
            p = torch.eye(4)
            p[:3, :3] = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
            p[:3, 3] = torch.tensor([12.0 + 2.0 * float(t) + a, y0, 0.5])
            poses.append(p)
        out.append({"timestamps": ts.clone(), "poses": torch.stack(poses), "dims": torch.tensor(dims),
                    "symmetric": torch.tensor(True), "deformable": torch.tensor(False)})
    return out
