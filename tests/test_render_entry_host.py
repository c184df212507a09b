"""The host side of the fused render entry points (csrc/render.hip) and of the pair-position entry points (csrc/actors.hip):
what each one returns, and says, for arguments it refuses or has nothing to do for.  Library loaded on the CPU, every
pointer the placeholder address; every call here fails validation or returns early -- none reaches a launch or a memset.
No GPU."""
import ctypes

import pytest

I64, F32 = ctypes.c_int64, ctypes.c_float
ADDR = 0x1000  # any non-null, 16-byte aligned address: nothing is dereferenced
ONE = ctypes.c_void_p(ADDR)
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 2  # NRHIP_OK, NRHIP_ERR_INVALID_ARG, NRHIP_ERR_UNSUPPORTED

OUT3 = ["out_features", "out_depth", "out_acc"]
ROWS = ["feature", "sdf", "alpha"]
SAVE = ["save_enc", "save_geo_hidden", "save_feat_in", "save_feat_hidden"]
OVR = ["ovr_row", "ovr_rows", "ovr_dirs"]
CAND = ["cand_count", "cand_actor", "cand_w2b"]
PAIR = ["times", "sample_idx", "actor_idx", "ray_flip", "n_pairs"]
GRADS = ["grad_x01", "grad_cstd", "grad_positions", "grad_rotations_6d"]
# entry point -> (packed rays?, name in its messages, arguments after the descriptors and before the stream)
RENDER = {
    "nrhip_field_fwd": (False, "field_fwd", ROWS),
    "nrhip_field_fwd_train": (False, "field_fwd_train", ROWS + SAVE),
    "nrhip_field_fwd_train_ovr": (False, "field_fwd_train_ovr", OVR + ROWS + SAVE),
    "nrhip_render_fwd": (False, "render_fwd", OUT3 + ["out_weights"]),
    "nrhip_render_fwd_ex": (False, "render_fwd", OUT3 + ["out_weights", "eps"]),
    "nrhip_render_fwd_actors": (False, "render_fwd_actors", CAND + OUT3 + ["out_weights", "eps", "workspace"]),
    "nrhip_render_fwd_packed": (True, "render_fwd_packed", OUT3 + ["out_weights", "eps"]),
    "nrhip_field_fwd_train_packed": (True, "field_fwd_train_packed", ROWS + SAVE),
    "nrhip_field_fwd_train_packed_ovr": (True, "field_fwd_train_packed_ovr", OVR + ROWS + SAVE),
    "nrhip_render_fwd_packed_actors": (True, "render_fwd_packed_actors", CAND + OUT3 + ["out_weights", "eps", "workspace"]),
}
PAIRS = {
    "nrhip_actor_pair_positions_fwd": (False, "actor_pair_positions", PAIR + ["x01", "cstd"]),
    "nrhip_actor_pair_positions_bwd": (False, "actor_pair_positions_bwd", PAIR + GRADS),
    "nrhip_actor_pair_positions_bwd_rays": (False, "actor_pair_positions_bwd_rays", PAIR + GRADS + ["grad_origins", "grad_directions"]),
    "nrhip_actor_pair_positions_fwd_packed": (True, "actor_pair_positions_fwd_packed", ["ray_of"] + PAIR + ["x01", "cstd"]),
    "nrhip_actor_pair_positions_bwd_packed": (True, "actor_pair_positions_bwd_packed", ["ray_of"] + PAIR + GRADS),
}
WITH_ACTORS = [n for n in RENDER if n.endswith("actors")]
TRAIN = [n for n, (_, _, names) in RENDER.items() if "save_enc" in names]
OVERRIDES = [n for n, (_, _, names) in RENDER.items() if "ovr_row" in names]
OPTIONAL = ("out_weights", "ray_flip")  # may be NULL: a call without them would go on to the launch


@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as ge
    from neurad_studio_amd import _lib

    if not os.path.exists(ge.LIB):
        ge.build()
    return _lib.load()


def _grid(g, L, F, dtype):
    g.num_levels, g.n_features, g.log2_table_size, g.param_dtype = L, F, 11, dtype
    for l in range(L):
        g.scalings[l] = 16.0 * 2 ** l


def field(L=8, F=4, H=32, dtype=0):
    """an nrhip_field the validation accepts (given a shape the kernels exist for)"""
    from neurad_studio_amd import _lib

    f = _lib.Field()
    _grid(f.grid, L, F, dtype)
    f.table, f.static_scale, f.use_sdf, f.beta = ADDR, 100.0, 1, 3.0
    f.geo.in_dim, f.geo.hidden_dim, f.geo.out_dim, f.geo.num_layers = L * F, H, 33, 2
    f.feat.in_dim, f.feat.hidden_dim, f.feat.out_dim, f.feat.num_layers = 48, H, 32, 3
    for k in range(3):
        f.geo.weight[k] = f.geo.bias[k] = f.feat.weight[k] = f.feat.bias[k] = ADDR
    return f


def actors(L=8, F=4, dtype=0, **fields):
    from neurad_studio_amd import _lib

    a = _lib.Actors()
    a.n_actors, a.n_times, a.actor_scale, a.max_candidates = 3, 2, 10.0, 4
    for name in ("timestamps", "positions", "rotations_6d", "present", "bounds", "tables"):
        setattr(a, name, ADDR)
    _grid(a.grid, L, F, dtype)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def rays(packed, r=4, s=8, pointers=ADDR):
    from neurad_studio_amd import _lib

    d = _lib.PackedRays() if packed else _lib.Rays()
    d.n_rays, d.n_samples = r, s
    for name in ("origins", "directions", "pixel_area") + (("t_starts", "t_ends", "segments") if packed else ("starts", "ends")):
        setattr(d, name, pointers)
    return d


def call(lib, name, null_all=False, **over):
    """the entry point with valid arguments, `over` replacing some by name (f, a, rays, or one of its argument names);
    null_all: every plain pointer argument NULL"""
    packed, _, names = {**RENDER, **PAIRS}[name]
    args = [] if name in PAIRS else [over.get("f", field())]
    if name in PAIRS or name in WITH_ACTORS:
        args.append(over.get("a", actors()))
    args.append(over.get("rays", rays(packed)))
    for n in names:
        default = F32(0.0) if n == "eps" else I64(4) if n == "n_pairs" else (None if null_all else ONE)
        args.append(over.get(n, default))
    return getattr(lib, name)(*args, None)


def refused(lib, name, code, *fragments, named=True, **over):
    """the call returns `code`; its message holds every fragment and (named) starts with the entry point's name"""
    who = {**RENDER, **PAIRS}[name][1]
    assert call(lib, name, **over) == code, (name, over, lib.nrhip_last_error())
    msg = lib.nrhip_last_error().decode()
    assert all(f in msg for f in fragments) and (not named or msg.startswith(who + ":")), (name, over, msg)


def test_null_descriptors(lib):
    for name in RENDER:
        refused(lib, name, INVALID_ARG, "field descriptor is NULL", named=False, f=None)
    for name in WITH_ACTORS:
        refused(lib, name, INVALID_ARG, "actors descriptor is NULL", a=None)
    for name in PAIRS:
        refused(lib, name, INVALID_ARG, "actors descriptor is NULL", named=False, a=None)
    for name, (packed, _, _) in {**RENDER, **PAIRS}.items():
        refused(lib, name, INVALID_ARG, "rays descriptor is NULL", named=packed, rays=None)


def test_bad_ray_descriptors(lib):
    for name, (packed, _, _) in {**RENDER, **PAIRS}.items():
        refused(lib, name, INVALID_ARG, "negative", named=packed, rays=rays(packed, r=-1))
        refused(lib, name, INVALID_ARG, "NULL pointer", named=packed, rays=rays(packed, pointers=None))
        if packed:
            refused(lib, name, UNSUPPORTED, "2^31", rays=rays(True, s=1 << 31))


def test_unsupported_shapes(lib):
    for name in RENDER:
        refused(lib, name, UNSUPPORTED, "fused field kernel: no instantiation for L=3 F=8 H=32", named=False, f=field(3, 8, 32))
    # a shape of the static scene's kernels that the override kernel is not built for: refused by the dispatcher
    for name in OVERRIDES:
        refused(lib, name, UNSUPPORTED, "no instantiation for L=4 F=8 H=32", f=field(4, 8, 32))


def test_early_stop_eps_range(lib):
    for name, (_, _, names) in RENDER.items():
        if "eps" in names:
            for eps in (-0.1, 1.0):
                refused(lib, name, INVALID_ARG, "early_stop_eps", "not in [0,1)", eps=F32(eps))


def test_null_outputs_and_buffers(lib):
    for name, (_, _, names) in RENDER.items():
        for n in OUT3 + ROWS + SAVE:
            if n in names:
                refused(lib, name, INVALID_ARG, "NULL pointer / empty actor set" if name == "nrhip_render_fwd_actors" else "NULL output",
                        **{n: None})
    for name in TRAIN:
        for n in SAVE:
            refused(lib, name, INVALID_ARG, "save buffers must be 16-byte aligned", **{n: ctypes.c_void_p(0x1004)})


def test_override_arguments(lib):
    for name in OVERRIDES:
        for n in OVR:
            refused(lib, name, INVALID_ARG, "NULL pointer", **{n: None})
        refused(lib, name, INVALID_ARG, "override rows must be 16-byte aligned", ovr_rows=ctypes.c_void_p(0x1008))
        # the buffers are looked at before the override arguments
        refused(lib, name, INVALID_ARG, "NULL output", ovr_row=None, save_enc=None)
    refused(lib, "nrhip_field_fwd_train_ovr", UNSUPPORTED, "N >= 2^31", rays=rays(False, r=1 << 20, s=1 << 11))


def test_actor_arguments(lib):
    for name in WITH_ACTORS:
        for n in CAND + ["workspace"]:
            refused(lib, name, INVALID_ARG, "NULL pointer / empty actor set", **{n: None})
        for bad in (dict(bounds=None), dict(tables=None), dict(n_actors=0), dict(actor_scale=0.0)):
            refused(lib, name, INVALID_ARG, "NULL pointer / empty actor set", a=actors(**bad))
        refused(lib, name, UNSUPPORTED, "must share one storage type", a=actors(dtype=1))
        refused(lib, name, UNSUPPORTED, "actor grid (L=8 F=2)", "(F=4)", "(L=8)", a=actors(F=2))
        refused(lib, name, UNSUPPORTED, "actor grid (L=9 F=4)", a=actors(L=9))
        refused(lib, name, INVALID_ARG, "num_levels", named=False, a=actors(L=0))
    # dense: the pointers come before the sample count
    refused(lib, "nrhip_render_fwd_actors", INVALID_ARG, "needs >= 1 sample per ray", rays=rays(False, s=0))
    refused(lib, "nrhip_render_fwd_actors", INVALID_ARG, "NULL pointer / empty actor set", rays=rays(False, s=0), workspace=None)
    # packed: the output, eps and grid checks come before the candidates, and those before the ray count
    refused(lib, "nrhip_render_fwd_packed_actors", INVALID_ARG, "NULL output", out_acc=None, cand_count=None)
    refused(lib, "nrhip_render_fwd_packed_actors", INVALID_ARG, "early_stop_eps", eps=F32(1.0), cand_count=None)
    refused(lib, "nrhip_render_fwd_packed_actors", UNSUPPORTED, "must share one storage type", a=actors(dtype=1), cand_count=None)
    refused(lib, "nrhip_render_fwd_packed_actors", UNSUPPORTED, "n_rays >= 2^31", rays=rays(True, r=1 << 31))
    refused(lib, "nrhip_render_fwd_packed_actors", INVALID_ARG, "NULL pointer / empty actor set", rays=rays(True, r=1 << 31),
            workspace=None)


def test_sample_counts(lib):
    for name in ("nrhip_render_fwd", "nrhip_render_fwd_ex"):
        refused(lib, name, INVALID_ARG, "needs >= 1 sample per ray", rays=rays(False, s=0))
        refused(lib, name, INVALID_ARG, "NULL output", rays=rays(False, s=0), out_depth=None)
    # nothing per sample to write: no pointer is looked at
    for name in ("nrhip_field_fwd", "nrhip_field_fwd_train", "nrhip_field_fwd_train_ovr"):
        assert call(lib, name, null_all=True, rays=rays(False, s=0, pointers=None)) == OK, name
    for name in ("nrhip_field_fwd_train_packed", "nrhip_field_fwd_train_packed_ovr"):
        assert call(lib, name, null_all=True, rays=rays(True, s=0, pointers=None)) == OK, name


def test_zero_rays_is_a_no_op_with_every_pointer_null(lib):
    for name, (packed, _, _) in RENDER.items():
        assert call(lib, name, null_all=True, rays=rays(packed, r=0, pointers=None)) == OK, name
        assert call(lib, name, null_all=True, rays=rays(packed, r=0, s=0, pointers=None)) == OK, name
    for name in WITH_ACTORS:  # ... and the actor set is not looked at either, beyond its grid
        assert call(lib, name, null_all=True, rays=rays(RENDER[name][0], r=0, pointers=None),
                    a=actors(bounds=None, tables=None, n_actors=0)) == OK, name


def test_pair_position_arguments(lib):
    for name, (packed, _, names) in PAIRS.items():
        refused(lib, name, INVALID_ARG, "bad argument", n_pairs=I64(-1))
        refused(lib, name, INVALID_ARG, "bad argument", a=actors(actor_scale=0.0))
        refused(lib, name, INVALID_ARG, "need >= 1 actor and timestamp", named=False, a=actors(n_times=0))
        refused(lib, name, INVALID_ARG, "actors descriptor has a NULL pointer", named=False, a=actors(present=None))
        for n in names:
            if n not in OPTIONAL and n != "n_pairs":
                refused(lib, name, INVALID_ARG, "NULL pointer", **{n: None})
        # no pairs: nothing to do, whatever the pointers (the count is looked at first: -1 is refused above)
        assert call(lib, name, null_all=True, n_pairs=I64(0)) == OK, name
        assert call(lib, name, null_all=True, n_pairs=I64(0), rays=rays(packed, r=0, s=0, pointers=None)) == OK, name
        if packed:
            refused(lib, name, INVALID_ARG, "pairs of a batch without samples", n_pairs=I64(1), rays=rays(True, s=0))
            refused(lib, name, INVALID_ARG, "pairs of a batch without samples", n_pairs=I64(1), rays=rays(True, r=0))
