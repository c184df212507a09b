

def test_decode_rgb_recognises_only_the_reference_decoder_shape_and_falls_back_to_the_modules_on_cpu():
    """decode_rgb dispatches to the HIP decoder for the module tree of models/neurad.py:201-216 only; anything else -- and
    any CPU tensor -- runs the torch modules (no device, no library call)."""
    import torch

    from neurad_studio_amd.model_components.cnns import _fused_decoder_args, decode_rgb, make_rgb_decoder

    dec = make_rgb_decoder(48, 32, 3)
    args = _fused_decoder_args(dec)
    assert args is not None and len(args[0]) == 38 and len(args[1]) == 8 and len(args[2]) == 8
    assert [tuple(p.shape) for p in args[0][:6]] == [(32, 48, 1, 1), (32,), (32, 32, 7, 7), (32,), (32,), (32,)]
    assert _fused_decoder_args(make_rgb_decoder(48, 16, 3)) is None          # other width
    assert _fused_decoder_args(make_rgb_decoder(48, 32, 2)) is None          # other upsampling factor
    assert _fused_decoder_args(torch.nn.Sequential(torch.nn.Conv2d(48, 3, 1))) is None
    no_bn = make_rgb_decoder(48, 32, 3)
    no_bn[2].main_branch[1] = torch.nn.Identity()
    assert _fused_decoder_args(no_bn) is None
    x = torch.randn(2 * 64, 48)
    dec.eval()
    with torch.no_grad():
        got = decode_rgb(dec, x, (8, 8))
        want = dec(x.view(2, 8, 8, 48).permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert got.shape == (2, 24, 24, 3) and torch.equal(got, want)


def _ops_under(monkeypatch, env):
    """a private copy of neurad_studio_amd/ops.py executed under `env`: two of its switches are read at import"""
    import importlib.util
    import sys

    from neurad_studio_amd import ops

    for k in ("NRHIP_ENCODE_BWD_ATOMIC", "NRHIP_BIN_ROUND_LOG2", "NRHIP_MULTI_BWD_BINNED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name = "neurad_studio_amd._ops_under_test"
    spec = importlib.util.spec_from_file_location(name, ops.__file__)
    mod = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, name, mod)  # (the dataclasses look their module up)
    spec.loader.exec_module(mod)
    return mod


def test_binned_table_gradient_choice_matches_the_four_call_sites_it_replaced(monkeypatch):
    """ops._binned_table_grad -> (binned, half) for hashgrid_bwd / proposal_density_bwd / encode_bwd (`single`) and for
    _multi_bwd_block (`multi`, which alone honours NRHIP_MULTI_BWD_BINNED).  The expected values are what the expressions
    at those sites gave before they were folded into the helper: binned = n >= 2^15 and no NRHIP_ENCODE_BWD_ATOMIC (and the
    multi switch); half = binned, an fp16 gradient, n <= 2^23 and no NRHIP_BIN_ROUND_LOG2 (hashgrid_bwd and
    proposal_density_bwd return fp32 and never asked)."""
    import ctypes as C

    import torch

    f32, f16 = torch.float32, torch.float16
    ns = ((1 << 15) - 1, 1 << 15, 1 << 23, (1 << 23) + 1)
    no, yes, yes_half = (False, False), (True, False), (True, True)
    # environment -> {(n, out_dtype): (single, multi)}
    expected = {
        (): {
            (ns[0], f32): (no, no), (ns[0], f16): (no, no),
            (ns[1], f32): (yes, yes), (ns[1], f16): (yes_half, yes_half),
            (ns[2], f32): (yes, yes), (ns[2], f16): (yes_half, yes_half),
            (ns[3], f32): (yes, yes), (ns[3], f16): (yes, yes),
        },
        (("NRHIP_ENCODE_BWD_ATOMIC", "1"),): {
            (ns[0], f32): (no, no), (ns[0], f16): (no, no),
            (ns[1], f32): (no, no), (ns[1], f16): (no, no),
            (ns[2], f32): (no, no), (ns[2], f16): (no, no),
            (ns[3], f32): (no, no), (ns[3], f16): (no, no),
        },
        (("NRHIP_BIN_ROUND_LOG2", "20"),): {
            (ns[0], f32): (no, no), (ns[0], f16): (no, no),
            (ns[1], f32): (yes, yes), (ns[1], f16): (yes, yes),
            (ns[2], f32): (yes, yes), (ns[2], f16): (yes, yes),
            (ns[3], f32): (yes, yes), (ns[3], f16): (yes, yes),
        },
        (("NRHIP_MULTI_BWD_BINNED", "0"),): {
            (ns[0], f32): (no, no), (ns[0], f16): (no, no),
            (ns[1], f32): (yes, no), (ns[1], f16): (yes_half, no),
            (ns[2], f32): (yes, no), (ns[2], f16): (yes_half, no),
            (ns[3], f32): (yes, no), (ns[3], f16): (yes, no),
        },
    }
    for env, table in expected.items():
        ops = _ops_under(monkeypatch, dict(env))
        queries = []

        def fake_call(name, *args, _queries=queries):  # the library's workspace query: 4096 bytes, "the partition can do it"
            _queries.append(name)
            C.cast(args[-1], C.POINTER(C.c_int64)).contents.value = 4096

        monkeypatch.setattr(ops, "call", fake_call)
        assert set(table) == {(n, dt) for n in ns for dt in (f32, f16)}
        for (n, dt), (single, multi) in table.items():
            what = f"{dict(env)} n={n} {dt}"
            assert ops._binned_table_grad(n, dt) == single, what
            assert ops._binned_table_grad(n, dt, enabled=ops._MULTI_BWD_BINNED) == multi, what
            # hashgrid_bwd and proposal_density_bwd take the binned path exactly when they get a workspace
            del queries[:]
            ws = ops._table_grad_workspace(C.c_int(0), n, "cpu")
            assert (ws is not None) == single[0], what
            assert queries == (["nrhip_encode_bwd_binned_workspace"] if single[0] else []), what
            assert ws is None or (ws.dtype == torch.uint8 and ws.numel() == 4096)
    # a table the library cannot cut into slices (workspace 0): atomics, whatever the batch
    monkeypatch.setattr(ops, "call", lambda name, *args: None)
    assert ops._table_grad_workspace(C.c_int(0), 1 << 20, "cpu") is None


def test_launch_marshalling_passes_addresses_null_scalars_and_structs_and_keeps_the_tensors():
    """ops._c_args is the conversion ``launch`` and the workspace queries apply to their arguments: a tensor (an
    nn.Parameter too) goes as its address, None as NULL, a ctypes structure by reference, everything else as it is; the
    pair it returns holds the tensors, so they outlive the call that receives the addresses."""
    import ctypes as C
    import gc
    import weakref

    import torch

    from neurad_studio_amd import _lib, ops

    t = torch.arange(6, dtype=torch.float32)[::2].contiguous()  # (a copy nobody else holds, like _chk's)
    p = torch.nn.Parameter(torch.ones(4))
    g = _lib.Grid()
    g.num_levels = 7
    arr = (C.c_void_p * 2)(1, 2)
    addr_t, addr_p, alive = t.data_ptr(), p.data_ptr(), (weakref.ref(t), weakref.ref(p))
    held = ops._c_args((t, p, None, 5, 2.5, g, arr))
    del t, p
    gc.collect()
    c_args, kept = held
    assert c_args[0] == addr_t and c_args[1] == addr_p and type(c_args[0]) is int and type(c_args[1]) is int
    assert c_args[2] is None                       # ctypes passes None as a NULL pointer
    assert c_args[3] == 5 and type(c_args[3]) is int and c_args[4] == 2.5 and type(c_args[4]) is float
    assert type(c_args[5]) is type(C.byref(g)) and c_args[5]._obj is g
    assert C.cast(c_args[5], C.POINTER(_lib.Grid)).contents.num_levels == 7
    assert c_args[6] is arr
    assert len(c_args) == 7
    # the tensors live as long as the returned pair does, and no longer
    assert alive[0]() is kept[0] and alive[1]() is kept[1] and kept[0].data_ptr() == addr_t
    del held, c_args, kept
    gc.collect()
    assert alive[0]() is None and alive[1]() is None
