"""Tensor-level wrappers over the C ABI (no autograd here; see autograd.py).

PyTorch is plumbing only: it owns the device buffers and the current HIP stream.  Every function
launches hand-written HIP kernels from libneurad_hip.so on ``torch.cuda.current_stream()`` and fails
loudly when given CPU tensors -- there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import call


def _stream() -> C.c_void_p:  # (_stream / _ptr: for tests and scripts that call the library directly; wrappers use launch)
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _chk(t: Tensor, name: str, dtype=torch.float32) -> Tensor:
    if not isinstance(t, Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise _lib.NeuradHipError(f"{name}: tensor is on {t.device}; the HIP path needs a GPU tensor (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _opt(t: Optional[Tensor], name: str, dtype=torch.float32) -> Optional[Tensor]:
    """an optional per-ray / per-sample argument: None, or the tensor flattened and checked"""
    return None if t is None else _chk(t.reshape(-1), name, dtype)


def _c_args(args: tuple) -> Tuple[list, tuple]:
    """-> (what the C entry point receives, the arguments themselves).  A tensor (parameters included) goes as its address,
    None as NULL, a ctypes structure by reference; ints, floats, ctypes arrays and byref objects go as they are.  Nothing is
    checked here -- ``_chk`` and the wrappers do that.  Whoever holds the pair holds every tensor the addresses point to."""
    return [a.data_ptr() if isinstance(a, Tensor) else C.byref(a) if isinstance(a, C.Structure) else a for a in args], args


def launch(name: str, *args) -> None:
    """Enqueue entry point ``name`` on the current stream (which it appends to ``args``).  ``args`` holds every tensor until
    the entry point has returned, a contiguous copy made in the argument list included.  Host-only entry points (workspace
    and size queries, plans) take no stream: they go through ``call`` with the same conversion."""
    c_args, keep = _c_args(args)
    call(name, *c_args, torch.cuda.current_stream().cuda_stream)


def _workspace(entry: str, *args, device, dtype) -> Tuple[Tensor, int]:
    """Ask ``entry`` (a ``*_workspace`` query: args..., int64* out) for its scratch size and allocate it -> (scratch of
    max(size, 1) elements of ``dtype``: never a NULL address, the size the library asked for)"""
    need = C.c_int64(0)
    c_args, keep = _c_args(args)
    call(entry, *c_args, C.byref(need))
    return torch.empty((max(need.value, 1),), device=device, dtype=dtype), need.value


def _host_ptrs(tensors: Sequence[Optional[Tensor]], n: Optional[int] = None):
    """host array of ``n`` (default: as many as tensors) data pointers for a ``void* const*`` argument; None -> NULL.  The
    caller keeps the tensors."""
    return (C.c_void_p * (len(tensors) if n is None else n))(*[0 if t is None else t.data_ptr() for t in tensors])


def hash_scalings(num_levels: int, min_res: int, max_res: int) -> Tensor:
    """scalings_l = floor(min_res * g**l) evaluated exactly like encodings.py:347-350 (fp32 torch ops on CPU)."""
    levels = torch.arange(num_levels)
    growth = np.exp((np.log(max_res) - np.log(min_res)) / (num_levels - 1)) if num_levels > 1 else 1.0
    return torch.floor(min_res * growth**levels).to(torch.float32)


@dataclass
class GridSpec:
    """Static description of one HashEncoding (encodings.py:326-352)."""

    num_levels: int
    features_per_level: int
    log2_hashmap_size: int
    min_res: int
    max_res: int
    scalings: Optional[Tensor] = None  # CPU fp32 [L]

    def __post_init__(self):
        if self.scalings is None:
            self.scalings = hash_scalings(self.num_levels, self.min_res, self.max_res)

    @property
    def out_dim(self) -> int:
        return self.num_levels * self.features_per_level

    @property
    def table_rows(self) -> int:
        return self.num_levels << self.log2_hashmap_size

    def c_grid(self, table) -> _lib.Grid:
        """table: the hash table (its shape is checked), or its storage dtype alone"""
        dtype = table.dtype if isinstance(table, Tensor) else table
        if dtype not in (torch.float32, torch.float16):
            raise TypeError(f"hash table must be fp32 or fp16, got {dtype}")
        if isinstance(table, Tensor) and tuple(table.shape) != (self.table_rows, self.features_per_level):
            raise ValueError(f"hash table shape {tuple(table.shape)} != {(self.table_rows, self.features_per_level)}")
        g = _lib.Grid()
        g.num_levels, g.n_features = self.num_levels, self.features_per_level
        g.log2_table_size = self.log2_hashmap_size
        g.param_dtype = 1 if dtype == torch.float16 else 0
        sc = self.scalings.tolist()
        for i, v in enumerate(sc):
            g.scalings[i] = v
        return g


def _c_mlp(weights: Sequence[Tensor], biases: Sequence[Optional[Tensor]]) -> Tuple[_lib.Mlp, list]:
    n = len(weights)
    if not 1 <= n <= _lib.MAX_LAYERS:
        raise ValueError(f"MLP needs 1..{_lib.MAX_LAYERS} layers, got {n}")
    keep = []
    m = _lib.Mlp()
    m.num_layers = n
    m.in_dim = weights[0].shape[1]
    m.out_dim = weights[-1].shape[0]
    m.hidden_dim = weights[0].shape[0] if n > 1 else 0
    for k, (w, b) in enumerate(zip(weights, biases)):
        exp_in = m.in_dim if k == 0 else m.hidden_dim
        exp_out = m.out_dim if k == n - 1 else m.hidden_dim
        if tuple(w.shape) != (exp_out, exp_in):
            raise ValueError(f"layer {k}: weight shape {tuple(w.shape)} != {(exp_out, exp_in)} (uniform hidden width)")
        w = _chk(w, f"weight[{k}]")
        keep.append(w)
        m.weight[k] = w.data_ptr()
        if b is not None:
            b = _chk(b, f"bias[{k}]")
            keep.append(b)
            m.bias[k] = b.data_ptr()
        else:
            m.bias[k] = None
    return m, keep


def _ray_constants(origins: Tensor, directions: Tensor, pixel_area: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """what both ray descriptors hold per RAY, checked: origins [R,3], directions [R,3], pixel_area flattened to [R]"""
    return _chk(origins, "origins"), _chk(directions, "directions"), _chk(pixel_area.reshape(-1), "pixel_area")


def _ray_order(r, order: Optional[Tensor]) -> Optional[Tensor]:
    """the optional processing order of a ray descriptor ``r``: int32 [R] from ``ray_order`` (locality hint for the fused
    kernels), checked and stored -> the tensor the descriptor now points to"""
    if order is not None:
        order = _chk(order, "order", torch.int32)
        if order.shape != (r.n_rays,):
            raise ValueError(f"order must be int32 [R={r.n_rays}], got {tuple(order.shape)}")
        r.order = order.data_ptr()
    return order


def _c_rays(origins: Tensor, directions: Tensor, pixel_area: Tensor, starts: Tensor, ends: Tensor,
            order: Optional[Tensor] = None):
    """starts/ends: [R,S] each, or views into one [R,S+1] edge tensor (stride S+1) -- no copies are made.
    order: see ``_ray_order``."""
    o, d, a = _ray_constants(origins, directions, pixel_area)
    R = o.shape[0]
    if starts.dim() != 2 or starts.shape != ends.shape or starts.shape[0] != R:
        raise ValueError(f"starts/ends must be [R,S] with R={R}; got {tuple(starts.shape)}, {tuple(ends.shape)}")
    if not (starts.is_cuda and ends.is_cuda and starts.dtype == torch.float32 and ends.dtype == torch.float32):
        raise _lib.NeuradHipError("starts/ends must be fp32 GPU tensors")
    S = starts.shape[1]
    if starts.stride(1) != 1 or ends.stride(1) != 1 or starts.stride(0) != ends.stride(0):
        starts, ends = starts.contiguous(), ends.contiguous()
    r = _lib.Rays()
    r.n_rays, r.n_samples = R, S
    r.origins, r.directions, r.pixel_area = o.data_ptr(), d.data_ptr(), a.data_ptr()
    r.starts, r.ends = starts.data_ptr(), ends.data_ptr()
    r.sample_stride = starts.stride(0) if R > 1 else max(S, 1)
    return r, (o, d, a, starts, ends, _ray_order(r, order))


_RAY_ORDER_LARGE = 16384  # rays above which ray_order takes the multi-workgroup counting sort


def ray_order(origins: Tensor, directions: Tensor, static_scale: float, t_ref: Optional[float] = None,
              key_bits: int = 0) -> Tensor:
    """Processing order that groups rays looking at the same region (csrc/rayorder.hip) -> int32 [R] permutation to pass
    as ``order=`` to field_fwd / field_fwd_train / render_fwd.  t_ref: distance of the key point along the ray; default
    = static_scale, the contraction boundary, where the key cell is set by where the ray leaves the scene."""
    t_ref = float(static_scale) if t_ref is None else t_ref
    o, d = _chk(origins, "origins"), _chk(directions, "directions")
    out = torch.empty((o.shape[0],), device=o.device, dtype=torch.int32)
    if o.shape[0] > _RAY_ORDER_LARGE:  # many workgroups: the one-workgroup pass costs ~2 us per 1024 rays
        ws, need = _workspace("nrhip_ray_order_workspace", o.shape[0], int(key_bits), device=o.device, dtype=torch.uint8)
        launch("nrhip_ray_order_large", o, d, o.shape[0], float(t_ref), float(static_scale), int(key_bits), ws, need, out)
        return out
    launch("nrhip_ray_order", o, d, o.shape[0], float(t_ref), float(static_scale), int(key_bits), out)
    return out


# ------------------------------------------------------------------------------------------------
# Table gradients: the atomics-free radix partition (csrc/encode_bwd_binned.hip) or memory-side atomics.
# A/B switch for profiling and for the parity test of the atomic path
_FORCE_ATOMIC_SCATTER = os.environ.get("NRHIP_ENCODE_BWD_ATOMIC") is not None
_MULTI_BWD_BINNED = os.environ.get("NRHIP_MULTI_BWD_BINNED", "1") != "0"  # 0: the actor grids' gradients by atomics (A/B)
_BINNED_MIN_SAMPLES = 1 << 15
_BINNED_ROUND_SAMPLES = 1 << 23  # round_samples() of csrc/encode_bwd_binned.hip


def _binned_table_grad(n_samples: int, out_dtype=torch.float32, enabled: bool = True) -> Tuple[bool, bool]:
    """-> (binned, half).  binned: the partition computes this gradient (unless the library then reports no workspace: a
    table too large to cut into LDS slices) -- not for small batches (one actor's hits), where four launches + scratch cost
    more than the few atomics.  half: it also writes the fp16 gradient of an fp16-storage table itself, which takes one round
    of the library's default length; otherwise fp32 comes back and the caller casts."""
    binned = enabled and n_samples >= _BINNED_MIN_SAMPLES and not _FORCE_ATOMIC_SCATTER
    half = (binned and out_dtype == torch.float16 and n_samples <= _BINNED_ROUND_SAMPLES
            and "NRHIP_BIN_ROUND_LOG2" not in os.environ)
    return binned, half


def _table_grad_workspace(c_grid, n_samples: int, device) -> Optional[Tensor]:
    """Scratch for the atomics-free table gradients; None -> use the atomic entry point."""
    if not _binned_table_grad(n_samples)[0]:
        return None
    ws, need = _workspace("nrhip_encode_bwd_binned_workspace", c_grid, int(n_samples), device=device, dtype=torch.uint8)
    return ws if need > 0 else None


def _table_grad(spec: "GridSpec", n_samples: int, device, out_dtype, binned, atomic) -> Tensor:
    """The gradient [L*T, F] of one table from ``n_samples`` samples, by the partition where ``_table_grad_workspace`` has
    scratch for it.  binned(suffix, c_grid, *tail) launches the caller's partition entry point: its name + suffix ("_f16":
    the fp16 gradient of an fp16-storage table, written by the partition itself, one round) with its own arguments between
    the grid and ``tail`` = (grad_table[, overwrite = 1: every element is written, no zero-fill], workspace, bytes).
    atomic() -> the gradient by memory-side atomics (fp32 only; the caller casts): a tiny batch, or a table too large to cut
    into LDS slices."""
    half = _binned_table_grad(n_samples, out_dtype)[1]
    dtype = torch.float16 if half else torch.float32
    g = spec.c_grid(dtype)
    ws = _table_grad_workspace(g, n_samples, device)
    if ws is None:
        return atomic()
    gt = torch.empty((spec.table_rows, spec.features_per_level), device=device, dtype=dtype)
    binned("_f16" if half else "", g, gt, *(() if half else (1,)), ws, ws.numel())
    return gt


def _zero_table_grad(spec: "GridSpec", device) -> Tuple[_lib.Grid, Tensor]:
    """-> (grid descriptor, zeros [L*T, F] fp32) for an atomic (accumulating) entry point"""
    gt = torch.zeros((spec.table_rows, spec.features_per_level), device=device, dtype=torch.float32)
    return spec.c_grid(gt), gt


def hashgrid_fwd(spec: GridSpec, table: Tensor, x: Tensor) -> Tensor:
    x = _chk(x, "x")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"x must be [N,3], got {tuple(x.shape)}")  # encodings.py:428
    table = table if table.is_contiguous() else table.contiguous()
    out = torch.empty((x.shape[0], spec.out_dim), device=x.device, dtype=torch.float32)
    launch("nrhip_hashgrid_fwd", spec.c_grid(table), table, x, x.shape[0], out)
    return out


def hashgrid_bwd(spec: GridSpec, table_like: Tensor, x: Tensor, grad_out: Tensor) -> Tensor:
    x, grad_out = _chk(x, "x"), _chk(grad_out, "grad_out")
    n = x.shape[0]

    def atomic():
        g, gt = _zero_table_grad(spec, x.device)
        launch("nrhip_hashgrid_bwd", g, x, grad_out, n, gt)
        return gt

    return _table_grad(spec, n, x.device, torch.float32,
                       lambda sfx, g, *tail: launch("nrhip_hashgrid_bwd_binned" + sfx, g, x, grad_out, n, *tail), atomic)


_POINTER_TABLES: dict = {}


def _ptr_array(tensors: Sequence[Tensor]) -> Tensor:
    """device array of data pointers (the multi-grid entry points take `void* const*` in device memory); uploaded once
    per distinct set of tensors -- a pageable H2D copy per call synchronises the host with the stream"""
    key = (tensors[0].device, tuple(t.data_ptr() for t in tensors))
    ptrs = _POINTER_TABLES.get(key)
    if ptrs is None:
        if len(_POINTER_TABLES) >= 32:
            _POINTER_TABLES.clear()
        ptrs = _POINTER_TABLES[key] = torch.tensor(key[1], dtype=torch.int64, device=key[0])
    return ptrs


def hashgrid_multi_fwd(spec: GridSpec, tables: Sequence[Tensor], grid_id: Tensor, x: Tensor) -> Tensor:
    """sample i -> tables[grid_id[i]]: all actor grids in one launch"""
    x, grid_id = _chk(x, "x"), _chk(grid_id, "grid_id", torch.int32)
    tables = [_chk(t, "table", tables[0].dtype) for t in tables]  # fp32 or fp16 storage, one dtype per call
    out = torch.empty((x.shape[0], spec.out_dim), device=x.device, dtype=torch.float32)
    launch("nrhip_hashgrid_multi_fwd", spec.c_grid(tables[0]), _ptr_array(tables), len(tables), grid_id, x, x.shape[0], out)
    return out


def grids_present(grid_id: Tensor, n_grids: int) -> List[bool]:
    """which grids a batch of rows refers to, as a host list (ONE device->host read; callers do it in the forward, right
    behind the read that sized the batch, so that the backward needs none)"""
    # (a scatter of ones, not torch.bincount: bincount first reduces max(grid_id) over all rows -- 0.25 ms at 0.5 M rows)
    return torch.zeros(n_grids, device=grid_id.device, dtype=torch.uint8).index_fill_(0, grid_id.long(), 1).tolist()


def hashgrid_multi_bwd(spec: GridSpec, n_grids: int, grid_id: Tensor, x: Tensor, grad_out: Tensor,
                       present: Optional[List[bool]] = None, out_dtype=torch.float32, dense_block: bool = False):
    """-> one gradient per grid, None for grids no sample refers to (like the reference's per-id loop, which never
    touches them: their optimizer state must not decay).  present: ``grids_present(grid_id, n_grids)`` when the caller
    already has it -- the backward then runs without a device->host read and without a host->device copy.
    dense_block=True: -> ONE tensor [n_grids, rows, F] instead (zeros for the grids without samples)."""
    x, grid_id, grad_out = _chk(x, "x"), _chk(grid_id, "grid_id", torch.int32), _chk(grad_out, "grad_out")
    if present is None:
        present = grids_present(grid_id, n_grids)
    present = [bool(p) for p in present]
    if dense_block:
        # slot a = grid a; a grid without samples keeps its (all-zero) slot
        block = _multi_bwd_block(spec, n_grids, grid_id, x, grad_out, tuple(a if p else -1 for a, p in enumerate(present)), n_grids,
                                 out_dtype) if any(present) else None
        if block is None:
            block = torch.zeros((n_grids, spec.table_rows, spec.features_per_level), device=x.device, dtype=out_dtype)
        return block
    if not any(present):
        return [None] * n_grids
    slots, k = [], 0
    for p in present:
        slots.append(k if p else -1)
        k += int(p)
    views = iter(_multi_bwd_block(spec, n_grids, grid_id, x, grad_out, tuple(slots), k, out_dtype).unbind(0))
    return [next(views) if p else None for p in present]


def _multi_bwd_block(spec: GridSpec, n_grids: int, grid_id: Tensor, x: Tensor, grad_out: Tensor, slots: Tuple[int, ...],
                     n_slots: int, out_dtype) -> Tensor:
    """-> [n_slots, rows, F] of ``out_dtype``: slot slots[a] holds grid a's gradient (slots[a] < 0: grid a sends nothing)"""
    n = x.shape[0]
    binned, half = _binned_table_grad(n, out_dtype, enabled=_MULTI_BWD_BINNED)
    if binned:
        # the radix partition over (slot, level, slice) (csrc/encode_bwd_binned.hip, MultiSrc): no memory-side atomics, every
        # element of the block written by the partition (no zero-fill), fp16-storage grids get their fp16 gradient directly
        g = spec.c_grid(torch.float32)  # (levels and sizes only: the gradient's type is the `half` flag of the call)
        ws, need = _workspace("nrhip_hashgrid_multi_bwd_binned_workspace", g, n_slots, n, device=x.device, dtype=torch.uint8)
        if need > 0:
            block = torch.empty((n_slots, spec.table_rows, spec.features_per_level), device=x.device,
                                dtype=torch.float16 if half else torch.float32)
            slot32 = _slot_table(slots, x.device, torch.int32)
            launch("nrhip_hashgrid_multi_bwd_binned", g, n_grids, grid_id, slot32, n_slots, x, grad_out, n, block,
                   1 if half else 0, ws, need)
            return block if block.dtype == out_dtype else block.to(out_dtype)
    # one zero-filled block for all touched grids (a scene has ~100 actor grids: one fill, not one per grid)
    flat = torch.zeros((n_slots, spec.table_rows, spec.features_per_level), device=x.device, dtype=torch.float32)
    g = spec.c_grid(flat[0])
    # device array of the gradient tables' addresses, computed ON the device (base + slot * stride; 0 for untouched grids):
    # a torch.tensor(list, device=...) here is a pageable host->device copy, i.e. a stream synchronisation per backward
    slot = _slot_table(slots, x.device, torch.int64)
    ptrs = torch.where(slot >= 0, slot * (flat[0].numel() * 4) + flat.data_ptr(), torch.zeros_like(slot))
    launch("nrhip_hashgrid_multi_bwd", g, n_grids, grid_id, x, grad_out, x.shape[0], ptrs)
    # fp16-storage grids: autograd wants the parameter's dtype -- ONE cast of the block
    return flat if out_dtype == torch.float32 else flat.to(out_dtype)


_SLOT_TABLES: dict = {}


def _slot_table(slots: Tuple[int, ...], device, dtype) -> Tensor:
    """int64 / int32 [n_grids] on the device: position of each grid in the gradient block, -1 for grids without one; uploaded
    once per distinct pattern"""
    key = (device, slots, dtype)
    t = _SLOT_TABLES.get(key)
    if t is None:
        if len(_SLOT_TABLES) >= 64:
            _SLOT_TABLES.clear()
        t = _SLOT_TABLES[key] = torch.tensor(slots, dtype=dtype, device=device)
    return t


def hashgrid_multi_bwd_input(spec: GridSpec, tables: Sequence[Tensor], grid_id: Tensor, x: Tensor, grad_out: Tensor):
    x, grid_id, grad_out = _chk(x, "x"), _chk(grid_id, "grid_id", torch.int32), _chk(grad_out, "grad_out")
    tables = [_chk(t, "table", tables[0].dtype) for t in tables]
    gx = torch.empty_like(x)
    launch("nrhip_hashgrid_multi_bwd_input", spec.c_grid(tables[0]), _ptr_array(tables), len(tables), grid_id, x, grad_out,
           x.shape[0], gx)
    return gx


def hashgrid_bwd_input(spec: GridSpec, table: Tensor, x: Tensor, grad_out: Tensor) -> Tensor:
    x, grad_out = _chk(x, "x"), _chk(grad_out, "grad_out")
    gx = torch.empty_like(x)
    launch("nrhip_hashgrid_bwd_input", spec.c_grid(table), table, x, grad_out, x.shape[0], gx)
    return gx


def encode_fwd(spec: GridSpec, table: Tensor, static_scale: float, origins, directions, pixel_area, starts, ends):
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    out = torch.empty((r.n_rays * r.n_samples, spec.out_dim), device=origins.device, dtype=torch.float32)
    launch("nrhip_encode_fwd", spec.c_grid(table), table, float(static_scale), r, out)
    return out


def encode_bwd(spec: GridSpec, static_scale: float, origins, directions, pixel_area, starts, ends, grad_out,
               out_dtype=torch.float32):
    """-> grad table [L*T, F].  out_dtype=torch.float16 (an fp16-storage table): the binned path writes the gradient in fp16
    itself where it can (one round, i.e. <= 2^23 samples) -- otherwise fp32 is returned and the caller casts."""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    grad_out = _chk(grad_out, "grad_out")
    scale = float(static_scale)

    def atomic():
        g, gt = _zero_table_grad(spec, origins.device)
        launch("nrhip_encode_bwd", g, scale, r, grad_out, gt)
        return gt

    return _table_grad(spec, r.n_rays * r.n_samples, origins.device, out_dtype,
                       lambda sfx, g, *tail: launch("nrhip_encode_bwd_binned" + sfx, g, scale, r, grad_out, *tail), atomic)


def encode_bwd_rays(spec: GridSpec, table: Tensor, static_scale: float, origins, directions, pixel_area, starts, ends,
                    grad_out) -> Tuple[Tensor, Tensor]:
    """dL/d(origins), dL/d(directions) [R,3] of the static encoding path from dL/d(rescaled features) [N, L*F]: the
    gradient a camera optimizer that moves the rays receives (cameras/camera_optimizers.py:173-182).  One kernel, no
    atomics (csrc/hashgrid_dx.hip)."""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    grad_out = _chk(grad_out, "grad_out")
    if grad_out.numel() != r.n_rays * r.n_samples * spec.out_dim:
        raise ValueError(f"grad_out has {grad_out.numel()} elements, expected {r.n_rays * r.n_samples * spec.out_dim}")
    g = spec.c_grid(table)
    out = torch.empty((2, r.n_rays, 3), device=origins.device, dtype=torch.float32)
    launch("nrhip_encode_bwd_rays", g, _chk(table, "table", table.dtype), float(static_scale), r, grad_out, out[0], out[1])
    return out[0], out[1]


def sh4_fwd(dirs01: Tensor) -> Tensor:
    d = _chk(dirs01, "dirs")
    out = torch.empty((d.shape[0], 16), device=d.device, dtype=torch.float32)
    launch("nrhip_sh4_fwd", d, d.shape[0], out)
    return out


def mlp_fwd(x: Tensor, weights, biases, save_hidden: bool = False):
    x = _chk(x, "x")
    m, keep = _c_mlp(weights, biases)
    if x.dim() != 2 or x.shape[1] != m.in_dim:
        raise ValueError(f"x must be [N,{m.in_dim}], got {tuple(x.shape)}")
    n = x.shape[0]
    y = torch.empty((n, m.out_dim), device=x.device, dtype=torch.float32)
    hidden = None
    if save_hidden and m.num_layers > 1:
        hidden = torch.empty((n, (m.num_layers - 1) * m.hidden_dim), device=x.device, dtype=torch.float32)
    launch("nrhip_mlp_fwd", m, x, n, y, hidden)
    return (y, hidden) if save_hidden else y


def _mlp_grads(m: _lib.Mlp, n: int, weights, biases, device):
    """what both MLP backward entry points write into: -> (weight gradients, bias gradients (None where there is no bias),
    the C arguments behind them: the two host pointer arrays, the workspace and its size)"""
    # one zero-filled buffer for every weight / bias gradient of the MLP (one fill launch instead of 2 per layer)
    sizes = [w.numel() for w in weights] + [0 if b is None else b.numel() for b in biases]
    views = torch.split(torch.zeros((sum(sizes),), device=device, dtype=torch.float32), sizes)
    gws = [v.view_as(w) for v, w in zip(views[:len(weights)], weights)]
    gbs = [None if b is None else v.view_as(b) for v, b in zip(views[len(weights):], biases)]
    ws, need = _workspace("nrhip_mlp_bwd_workspace", m, n, device=device, dtype=torch.float32)
    return gws, gbs, (_host_ptrs(gws, _lib.MAX_LAYERS), _host_ptrs(gbs, _lib.MAX_LAYERS), ws, need)


def mlp_bwd(x: Tensor, hidden: Optional[Tensor], grad_y: Tensor, weights, biases, need_grad_x: bool = True):
    x, grad_y = _chk(x, "x"), _chk(grad_y, "grad_y")
    m, keep = _c_mlp(weights, biases)
    n = x.shape[0]
    gx = torch.empty_like(x) if need_grad_x else None
    gws, gbs, out = _mlp_grads(m, n, weights, biases, x.device)
    launch("nrhip_mlp_bwd", m, x, hidden, grad_y, n, gx, *out)
    return gx, gws, gbs


def field_feature_bwd_supported(weights, biases) -> bool:
    """shapes nrhip_field_feature_bwd covers: NeuRADField's feature head 48 -> {32,64} -> {32,64} -> 32 with biases"""
    return (len(weights) == 3 and weights[0].shape[1] == 48 and weights[2].shape[0] == 32 and weights[0].shape[0] in (32, 64)
            and all(b is not None for b in biases))


def field_feature_bwd(x: Tensor, hidden: Tensor, grad_feature: Tensor, grad_geo0: Tensor, weights, biases):
    """Backward of feature = geo[:, 1:] + mlp_feature([geo[:, 1:] | sh]) (neurad_field.py:146-152) in one pass: returns
    (grad_geo [N,33] = (grad_geo0 | grad_feature + grad_x[:, :32]), weight gradients, bias gradients)."""
    x, grad_feature, grad_geo0 = _chk(x, "x"), _chk(grad_feature, "grad_feature"), _chk(grad_geo0.reshape(-1), "grad_geo0")
    m, keep = _c_mlp(weights, biases)
    n = x.shape[0]
    if grad_geo0.shape[0] != n or grad_feature.shape != (n, 32):
        raise ValueError("field_feature_bwd: grad_feature [N,32] and grad_geo0 [N] expected")
    g_geo = torch.empty((n, 33), device=x.device, dtype=torch.float32)
    gws, gbs, out = _mlp_grads(m, n, weights, biases, x.device)
    launch("nrhip_field_feature_bwd", m, x, hidden, grad_feature, grad_geo0, n, g_geo, *out)
    return g_geo, gws, gbs


# ------------------------------------------------------------------------------------------------
@dataclass
class FieldSpec:
    """What the fused field/render kernels need (NeuRADField, neurad_field.py:78-152)."""

    grid: GridSpec
    table: Tensor
    static_scale: float
    geo_w: List[Tensor]
    geo_b: List[Optional[Tensor]]
    feat_w: List[Tensor]
    feat_b: List[Optional[Tensor]]
    use_sdf: bool = True
    beta: float = 20.0 + 1e-4  # |beta| + beta_min (model_components/utils.py:38-41)

    def c_field(self, eval_layout: bool = False):
        f = _lib.Field()
        f.grid = self.grid.c_grid(self.table)
        f.table = self.table.data_ptr()
        f.static_scale = float(self.static_scale)
        f.geo, k1 = _c_mlp(self.geo_w, self.geo_b)
        f.feat, k2 = _c_mlp(self.feat_w, self.feat_b)
        f.use_sdf = 1 if self.use_sdf else 0
        f.beta = float(self.beta)
        k3 = None
        if eval_layout:  # inference: the coarse levels from their shadow copies (bit-identical outputs)
            k3 = eval_table(self.grid, self.table)
            if k3 is not None:
                f.eval_table, f.eval_layout = k3[0].data_ptr(), k3[1]
        return f, (k1, k2, k3)


# Eval-time layout of the coarse levels (csrc/eval_layout.hip).  OPT-IN (NRHIP_EVAL_RELAYOUT=1): measured on BASELINE
# config[1] it changes neither the fabric reads nor the L1 -> L2 requests of the render kernel (the coarse levels are L2
# resident either way and the 16 lanes that share a level walk consecutive samples of one ray, i.e. the same lines in both
# layouts) and costs 2.6 % of kernel time (168.7 -> 173.1 us: one more LDS read and two more live registers per level);
# outputs are bit-identical.  profiles/r03_eval_relayout.txt.
_EVAL_RELAYOUT = os.environ.get("NRHIP_EVAL_RELAYOUT", "0") == "1"
_EVAL_TABLES: dict = {}  # (data_ptr, version, dtype, shape, grid key) -> (eval table, layout array, n shadow levels)


def eval_layout_plan(spec: GridSpec, table_dtype=torch.float32):
    """host logic: -> (layout ctypes array [L*4] = {mulY, mulZ, mask, row0} per level, rows of the eval table, number of
    levels that get a shadow copy)"""
    lay = (C.c_uint32 * (4 * spec.num_levels))()
    rows = C.c_int64(0)
    call("nrhip_eval_layout_plan", C.byref(spec.c_grid(table_dtype)), lay, C.byref(rows))
    n_shadow = sum(1 for l in range(spec.num_levels) if lay[4 * l] != 2654435761)
    return lay, rows.value, n_shadow


def eval_table(spec: GridSpec, table: Tensor):
    """The table re-laid out for inference, cached per (storage, in-place version): -> (eval table, layout) or None when no
    level qualifies or the layout is switched off.  A derived buffer: the parameter (and the state_dict) stay as they are;
    writes through ``table.data`` do not bump the version -- call ``clear_eval_tables()`` after such edits."""
    if not _EVAL_RELAYOUT or not table.is_cuda:
        return None
    key = (table.data_ptr(), table._version, table.dtype, tuple(table.shape), spec.num_levels, spec.min_res, spec.max_res)
    hit = _EVAL_TABLES.get(key)
    if hit is None:
        lay, rows, n_shadow = eval_layout_plan(spec, table.dtype)
        if n_shadow == 0:
            hit = (None, None)
        else:
            out = torch.empty((rows, spec.features_per_level), device=table.device, dtype=table.dtype)
            launch("nrhip_eval_layout_build", spec.c_grid(table), table, lay, out)
            hit = (out, lay)
        for k in [k for k in _EVAL_TABLES if k[0] == key[0] and k != key]:  # older versions of the same parameter
            del _EVAL_TABLES[k]
        if len(_EVAL_TABLES) >= 4:
            _EVAL_TABLES.clear()
        _EVAL_TABLES[key] = hit
    return None if hit[0] is None else hit


TABLE_EPOCH = [0]  # bumped whenever a kernel has written tables behind autograd's back (the optimizer): copies made from
                   # the tables before that (eval re-layouts, field_components/neurad_encoding.py's stacked actor tables) are stale


def clear_eval_tables() -> None:
    _EVAL_TABLES.clear()
    TABLE_EPOCH[0] += 1


def field_fwd(fs: FieldSpec, origins, directions, pixel_area, starts, ends, order: Optional[Tensor] = None):
    """-> feature [R,S,32], sdf (or raw geo output) [R,S], alpha (or density) [R,S]"""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends, order)
    f, keep2 = fs.c_field()
    R, S = r.n_rays, r.n_samples
    dev = origins.device
    feature = torch.empty((R, S, 32), device=dev, dtype=torch.float32)
    sdf = torch.empty((R, S), device=dev, dtype=torch.float32)
    alpha = torch.empty((R, S), device=dev, dtype=torch.float32)
    launch("nrhip_field_fwd", f, r, feature, sdf, alpha)
    return feature, sdf, alpha


def field_fwd_train(fs: FieldSpec, origins, directions, pixel_area, starts, ends, order: Optional[Tensor] = None,
                    override=None):
    """field_fwd + the activations the backward needs: -> (feature [N,32], geo_out [N], head [N]),
    (enc [N,L*F], geo_hidden [N,H], feat_in [N,48], feat_hidden [N,2H]).
    override = (ovr_row int32 [N] (row index or -1), ovr_rows [P,L*F], ovr_dirs [P,3]): samples inside an actor box take
    their encoding row and SH direction from the caller (nrhip_field_fwd_train_ovr)."""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends, order)
    f, keep2 = fs.c_field()
    n, dev = r.n_rays * r.n_samples, origins.device
    H, LF = fs.geo_w[0].shape[0], fs.grid.out_dim  # hidden width, encoding width L*F
    mk = lambda c: torch.empty((n, c), device=dev, dtype=torch.float32)  # noqa: E731
    feature, enc, hg, xf, hf = mk(32), mk(LF), mk(H), mk(48), mk(2 * H)
    sdf = torch.empty((n,), device=dev, dtype=torch.float32)
    head = torch.empty((n,), device=dev, dtype=torch.float32)
    if override is not None:
        ov, rows, dirs = override
        ov, rows, dirs = _chk(ov.reshape(-1), "ovr_row", torch.int32), _chk(rows, "ovr_rows"), _chk(dirs, "ovr_dirs")
        if ov.shape[0] != n or rows.dim() != 2 or rows.shape[1] != LF or dirs.shape != (rows.shape[0], 3):
            raise ValueError(f"field_fwd_train: override = (int32 [N], [P,{LF}], [P,3])")
        launch("nrhip_field_fwd_train_ovr", f, r, ov, rows, dirs, feature, sdf, head, enc, hg, xf, hf)
    else:
        launch("nrhip_field_fwd_train", f, r, feature, sdf, head, enc, hg, xf, hf)
    return (feature, sdf, head), (enc, hg, xf, hf)


def _render_outputs(R: int, S: int, device, return_weights: bool, out=None):
    """-> features [R,32], depth [R,1], accumulation [R,1] (the caller's ``out`` when given), weights [R,S] or None"""
    mk = lambda c: torch.empty((R, c), device=device, dtype=torch.float32)  # noqa: E731
    feats, depth, acc = (mk(32), mk(1), mk(1)) if out is None else out
    return feats, depth, acc, (mk(S) if return_weights else None)


def render_fwd(fs: FieldSpec, origins, directions, pixel_area, starts, ends, return_weights: bool = False,
               out: Optional[Tuple[Tensor, Tensor, Tensor]] = None, early_stop_eps: float = 0.0,
               order: Optional[Tensor] = None):
    """The fused headline kernel.  -> features [R,32], depth [R,1], accumulation [R,1] (, weights [R,S]).
    early_stop_eps > 0 (eval option, default exact): rays stop once their transmittance is below it.
    order: processing order from ``ray_order`` (locality hint; outputs stay in batch order)."""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends, order)
    f, keep2 = fs.c_field(eval_layout=not fs.table.requires_grad)
    feats, depth, acc, w = _render_outputs(r.n_rays, r.n_samples, origins.device, return_weights, out)
    launch("nrhip_render_fwd_ex", f, r, feats, depth, acc, w, float(early_stop_eps))
    return (feats, depth, acc, w) if return_weights else (feats, depth, acc)


def render_fwd_actors(fs: FieldSpec, spec: "ActorSpec", cand, origins, directions, pixel_area, starts, ends,
                      return_weights: bool = False, early_stop_eps: float = 0.0, order: Optional[Tensor] = None):
    """``render_fwd`` for a scene with dynamic actors, still one kernel: samples inside an actor box read that actor's
    grid (cand = ``actor_prepare``'s per-ray candidate lists).  Raises NrhipError(UNSUPPORTED) when the actor grid does
    not share the static grid's features per level -- callers fall back to the operator-level path."""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends, order)
    f, keep2 = fs.c_field()
    a, keep3 = spec.c_actors()
    cnt, act, w2b, _ = cand
    feats, depth, acc, w = _render_outputs(r.n_rays, r.n_samples, origins.device, return_weights)
    work = torch.empty((r.n_rays + 4,), device=origins.device, dtype=torch.int32)
    launch("nrhip_render_fwd_actors", f, a, r, cnt, act, w2b, feats, depth, acc, w, float(early_stop_eps), work)
    return (feats, depth, acc, w) if return_weights else (feats, depth, acc)


# ------------------------------------------------------------------------------------------------
def render_weight_from_alpha(alphas: Tensor):
    a = _chk(alphas, "alphas")
    R, S = a.shape
    w, t = torch.empty_like(a), torch.empty_like(a)
    launch("nrhip_render_weight_from_alpha", a, R, S, w, t)
    return w, t


def render_weight_from_alpha_bwd(alphas, grad_w, grad_t=None):
    a, gw = _chk(alphas, "alphas"), _chk(grad_w, "grad_w")
    gt = None if grad_t is None else _chk(grad_t, "grad_t")
    ga = torch.empty_like(a)
    launch("nrhip_render_weight_from_alpha_bwd", a, gw, gt, a.shape[0], a.shape[1], ga)
    return ga


def render_weight_from_density(t_starts, t_ends, sigmas):
    s, e, sg = _chk(t_starts, "t_starts"), _chk(t_ends, "t_ends"), _chk(sigmas, "sigmas")
    R, S = sg.shape
    w, t, a = torch.empty_like(sg), torch.empty_like(sg), torch.empty_like(sg)
    launch("nrhip_render_weight_from_density", s, e, sg, R, S, w, t, a)
    return w, t, a


def render_weight_from_density_bwd(t_starts, t_ends, sigmas, grad_w):
    s, e, sg, gw = (_chk(v, n) for v, n in ((t_starts, "t_starts"), (t_ends, "t_ends"), (sigmas, "sigmas"),
                                            (grad_w, "grad_w")))
    gs = torch.empty_like(sg)
    launch("nrhip_render_weight_from_density_bwd", s, e, sg, gw, sg.shape[0], sg.shape[1], gs)
    return gs


def accumulate_along_rays(weights, values=None):
    w = _chk(weights, "weights")
    R, S = w.shape
    if values is None:
        out = torch.empty((R, 1), device=w.device, dtype=torch.float32)
        launch("nrhip_accumulate_along_rays", w, None, R, S, 1, out)
        return out
    v = _chk(values, "values")
    Cc = v.shape[-1]
    out = torch.empty((R, Cc), device=w.device, dtype=torch.float32)
    launch("nrhip_accumulate_along_rays", w, v, R, S, Cc, out)
    return out


def composite_fwd(weights, features, starts, ends):
    w, f, s, e = (_chk(v, n) for v, n in ((weights, "weights"), (features, "features"), (starts, "starts"),
                                          (ends, "ends")))
    R, S, Cc = f.shape
    of = torch.empty((R, Cc), device=w.device, dtype=torch.float32)
    od = torch.empty((R, 1), device=w.device, dtype=torch.float32)
    oa = torch.empty((R, 1), device=w.device, dtype=torch.float32)
    launch("nrhip_composite_fwd", w, f, s, e, R, S, Cc, of, od, oa)
    return of, od, oa


def lidar_carving(starts: Tensor, ends: Tensor, is_lidar: Tensor, did_return: Optional[Tensor], distance: Tensor,
                  carving_epsilon: float, non_return_lidar_distance: float, weights: Optional[Tensor] = None,
                  want_mask: bool = True, want_grad: bool = True):
    """starts/ends [R,S] (any row stride), per-ray is_lidar / did_return (bool) / distance -> (is_close [R,S] bool or
    None, loss_per_ray [R] or None, grad_weights [R,S] or None); the loss terms need ``weights`` [R,S]."""
    R, S = starts.shape
    assert starts.stride(1) == 1 and ends.stride(1) == 1 and starts.stride(0) == ends.stride(0)
    for v, n in ((starts, "starts"), (ends, "ends")):
        if not v.is_cuda or v.dtype != torch.float32:
            raise _lib.NeuradHipError(f"{n}: expected a float32 GPU tensor")
    u8 = lambda m: None if m is None else m.reshape(-1).contiguous().view(torch.uint8)  # noqa: E731  (bool is 1 byte)
    lid, ret = u8(is_lidar), u8(did_return)
    dist = _chk(distance.reshape(-1), "distance")
    w = None if weights is None else _chk(weights, "weights")
    dev = starts.device
    close = torch.empty((R, S), dtype=torch.bool, device=dev) if want_mask else None
    loss = torch.empty((R,), dtype=torch.float32, device=dev) if w is not None else None
    gw = torch.empty((R, S), dtype=torch.float32, device=dev) if (w is not None and want_grad) else None
    launch("nrhip_lidar_carving", starts, ends, starts.stride(0), w, lid, ret, dist, float(carving_epsilon),
           float(non_return_lidar_distance), R, S, close, loss, gw)
    return close, loss, gw


def embedding_lerp(weight: Tensor, idx_lo: Tensor, idx_hi: Optional[Tensor] = None, frac: Optional[Tensor] = None) -> Tensor:
    """out[r] = weight[idx_lo[r]] * (1 - frac[r]) + weight[idx_hi[r]] * frac[r]   (idx_hi None: weight[idx_lo])"""
    w, lo = _chk(weight, "weight"), _chk(idx_lo.reshape(-1), "idx_lo", torch.int64)
    hi = _opt(idx_hi, "idx_hi", torch.int64)
    fr = _opt(frac, "frac")
    out = torch.empty((lo.shape[0], w.shape[1]), dtype=torch.float32, device=w.device)
    launch("nrhip_embedding_lerp_fwd", w, lo, hi, fr, lo.shape[0], w.shape[0], w.shape[1], out)
    return out


def embedding_lerp_bwd(g_out: Tensor, idx_lo, idx_hi, frac, n_embed: int) -> Tensor:
    g, lo = _chk(g_out, "g_out"), _chk(idx_lo.reshape(-1), "idx_lo", torch.int64)
    hi = _opt(idx_hi, "idx_hi", torch.int64)
    fr = _opt(frac, "frac")
    gw = torch.zeros((n_embed, g.shape[1]), dtype=torch.float32, device=g.device)
    launch("nrhip_embedding_lerp_bwd", g, lo, hi, fr, lo.shape[0], n_embed, g.shape[1], gw)
    return gw


def accumulate_along_rays_bwd(weights, values, g_out, need_grad_weights=True, need_grad_values=True):
    """-> (grad weights [R,S] or None, grad values [R,S,C] or None) of out[r,c] = sum_s w[r,s] v[r,s,c]"""
    w, v, g = _chk(weights, "weights"), _chk(values, "values"), _chk(g_out, "g_out")
    R, S, Cc = v.shape
    gw = torch.empty_like(w) if need_grad_weights else None
    gv = torch.empty_like(v) if need_grad_values else None
    launch("nrhip_accumulate_along_rays_bwd", w, v, g, R, S, Cc, gw, gv)
    return gw, gv


def composite_bwd(weights, features, starts, ends, g_feat, g_depth=None, g_acc=None, need_grad_features=True):
    w, f, s, e, gf = (_chk(v, n) for v, n in ((weights, "weights"), (features, "features"), (starts, "starts"),
                                              (ends, "ends"), (g_feat, "g_feat")))
    gd = _opt(g_depth, "g_depth")
    ga = _opt(g_acc, "g_acc")
    R, S, Cc = f.shape
    gw = torch.empty_like(w)
    gfe = torch.empty_like(f) if need_grad_features else None
    launch("nrhip_composite_bwd", w, f, s, e, gf, gd, ga, R, S, Cc, gw, gfe)
    return gw, gfe


# ------------------------------------------------------------------------------------------------
@dataclass
class ProposalSpec:
    grid: GridSpec
    table: Tensor
    static_scale: float
    decoder_weight: Tensor  # [1, L] (nn.Linear(L,1,bias=False).weight)

    def c_prop(self):
        p = _lib.Proposal()
        p.grid = self.grid.c_grid(self.table)
        p.table = self.table.data_ptr()
        p.static_scale = float(self.static_scale)
        dw = _chk(self.decoder_weight.reshape(-1), "decoder_weight")
        p.decoder_weight = dw.data_ptr()
        return p, dw


def proposal_density_fwd(ps: ProposalSpec, origins, directions, pixel_area, starts, ends, save_features: bool = False):
    """density [R,S]; with save_features also the rescaled per-level features, level-major [L, R*S], for the backward"""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    p, keep2 = ps.c_prop()
    dens = torch.empty((r.n_rays, r.n_samples), device=origins.device, dtype=torch.float32)
    lf = (torch.empty((ps.grid.num_levels, r.n_rays * r.n_samples), device=origins.device, dtype=torch.float32)
          if save_features else None)
    launch("nrhip_proposal_density_fwd", p, r, dens, lf)
    return (dens, lf) if save_features else dens


def proposal_density_bwd(ps: ProposalSpec, origins, directions, pixel_area, starts, ends, density, grad_density,
                         level_features: Optional[Tensor] = None):
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    p, keep2 = ps.c_prop()
    gdec = torch.zeros((1, ps.grid.num_levels), device=origins.device, dtype=torch.float32)
    ws = _table_grad_workspace(p.grid, r.n_rays * r.n_samples, origins.device)
    if ws is not None:
        gt = torch.empty((ps.grid.table_rows, 1), device=origins.device, dtype=torch.float32)
        launch("nrhip_proposal_density_bwd_binned", p, r, _chk(density, "density"), level_features,
               _chk(grad_density, "grad_density"), gt, gdec, 1, ws, ws.numel())
    else:
        if ps.table.dtype != torch.float32:  # the atomic kernel recomputes the features from an fp32 table: small batches only
            ps32 = ProposalSpec(ps.grid, ps.table.float(), ps.static_scale, ps.decoder_weight)  # (alive until the launch)
            p, keep2 = ps32.c_prop()
        gt = torch.zeros((ps.grid.table_rows, 1), device=origins.device, dtype=torch.float32)
        launch("nrhip_proposal_density_bwd", p, r, _chk(density, "density"), _chk(grad_density, "grad_density"), gt, gdec)
    return gt, gdec


def weights_from_density(deltas, densities) -> Tensor:
    d, s = _chk(deltas, "deltas"), _chk(densities, "densities")
    w = torch.empty_like(s)
    launch("nrhip_weights_from_density", d, s, s.shape[0], s.shape[1], w)
    return w


def weights_from_density_bwd(deltas, densities, grad_w) -> Tensor:
    d, s, g = _chk(deltas, "deltas"), _chk(densities, "densities"), _chk(grad_w, "grad_w")
    gs = torch.empty_like(s)
    launch("nrhip_weights_from_density_bwd", d, s, g, s.shape[0], s.shape[1], gs)
    return gs


def power_sampler(nears: Optional[Tensor], fars: Tensor, num_samples: int, lam: float = -1.0, scaling: float = 0.1,
                  t_rand: Optional[Tensor] = None, last_edge: float = 0.0):
    """-> spacing bins, euclidean bins [R,S+1]; last_edge > 0 sets the last euclidean edge (the model's sky stretch)"""
    f = _chk(fars.reshape(-1), "fars")
    n = _opt(nears, "nears")
    R = f.shape[0]
    tr = None if t_rand is None else _chk(t_rand, "t_rand")
    sp = torch.empty((R, num_samples + 1), device=f.device, dtype=torch.float32)
    eu = torch.empty_like(sp)
    launch("nrhip_power_sampler", n, f, R, num_samples, float(lam), float(scaling), tr, float(last_edge), sp, eu)
    return sp, eu


def power_sampler_ordered(nears: Optional[Tensor], fars: Tensor, num_samples: int, origins: Tensor, directions: Tensor,
                          static_scale: float, lam: float = -1.0, scaling: float = 0.1, t_rand: Optional[Tensor] = None,
                          last_edge: float = 0.0, t_ref: Optional[float] = None, key_bits: int = 0):
    """``power_sampler`` and ``ray_order`` as one launch -> (spacing bins, euclidean bins [R,S+1], order int32 [R])"""
    f = _chk(fars.reshape(-1), "fars")
    n = _opt(nears, "nears")
    o, d = _chk(origins, "origins"), _chk(directions, "directions")
    R = f.shape[0]
    if o.shape != (R, 3) or d.shape != (R, 3):
        raise ValueError(f"origins / directions must be [R={R},3]")
    tr = None if t_rand is None else _chk(t_rand, "t_rand")
    sp = torch.empty((R, num_samples + 1), device=f.device, dtype=torch.float32)
    eu = torch.empty_like(sp)
    order = torch.empty((R,), device=f.device, dtype=torch.int32)
    launch("nrhip_power_sampler_ordered", n, f, R, num_samples, float(lam), float(scaling), tr, float(last_edge), sp, eu, o,
           d, float(static_scale if t_ref is None else t_ref), float(static_scale), int(key_bits), order)
    return sp, eu, order


def pdf_sample(weights, spacing_bins, nears, fars, num_samples, lam=-1.0, scaling=0.1, histogram_padding=0.01,
               rand: Optional[Tensor] = None):
    w, b = _chk(weights, "weights"), _chk(spacing_bins, "spacing_bins")
    f = _chk(fars.reshape(-1), "fars")
    n = _opt(nears, "nears")
    R, Sp = w.shape
    stride = 0
    if rand is not None:
        rand = _chk(rand, "rand")
        stride = 0 if rand.numel() == R else num_samples + 1
    sp = torch.empty((R, num_samples + 1), device=w.device, dtype=torch.float32)
    eu = torch.empty_like(sp)
    launch("nrhip_pdf_sample", w, b, n, f, R, Sp, num_samples, float(lam), float(scaling), float(histogram_padding), rand,
           stride, sp, eu)
    return sp, eu


def proposal_sampler_fwd(props: Sequence[ProposalSpec], origins, directions, pixel_area, nears, fars,
                         num_samples=(128, 64, 32), lam=-1.0, scaling=0.1, histogram_padding=0.01,
                         sky_distance=20000.0, actor_specs: Optional[Sequence["ActorSpec"]] = None, cand=None):
    """Fused S5 (+ the far clamp of M1).  -> (weights per round, spacing bins per round+1, euclid bins per round+1).
    actor_specs[i] (+ cand, the per-ray candidate lists of ``actor_prepare``): the actor grids of props[i] -- proposal
    samples inside an actor box take their density from them (nrhip_proposal_sampler_fwd_actors)."""
    n_rounds = len(props)
    if len(num_samples) != n_rounds + 1:
        raise ValueError("num_samples needs one entry per proposal round plus the final count")
    o, d = _chk(origins, "origins"), _chk(directions, "directions")
    a = _chk(pixel_area.reshape(-1), "pixel_area")
    f = _opt(fars, "fars")
    n = _opt(nears, "nears")
    R = o.shape[0]
    cfg = _lib.SamplerCfg()
    cfg.n_rounds = n_rounds
    for i, v in enumerate(num_samples):
        cfg.n_samples[i] = v
    cfg.lam, cfg.scaling, cfg.histogram_padding, cfg.sky_distance = lam, scaling, histogram_padding, sky_distance
    cprops = (_lib.Proposal * n_rounds)()
    keep = []
    for i, p in enumerate(props):
        cp, k = p.c_prop()
        cprops[i] = cp
        keep.append(k)
    ws = [torch.empty((R, num_samples[i]), device=o.device, dtype=torch.float32) for i in range(n_rounds)]
    sps = [torch.empty((R, num_samples[i] + 1), device=o.device, dtype=torch.float32) for i in range(n_rounds + 1)]
    eus = [torch.empty((R, num_samples[i] + 1), device=o.device, dtype=torch.float32) for i in range(n_rounds + 1)]
    entry, actor_part = "nrhip_proposal_sampler_fwd", ()
    if actor_specs is not None:
        cacts = (_lib.Actors * n_rounds)()
        for i, s in enumerate(actor_specs):
            ca, k = s.c_actors()
            cacts[i] = ca
            keep.append(k)
        entry, actor_part = "nrhip_proposal_sampler_fwd_actors", (cacts, *cand[:3])  # (cand_count, cand_actor, cand_w2b)
    launch(entry, cfg, cprops, *actor_part, o, d, a, n, f, R, _host_ptrs(ws), _host_ptrs(sps), _host_ptrs(eus))
    return ws, sps, eus


@dataclass
class ActorSpec:
    """Device-side view of DynamicActors + the per-actor grids."""

    timestamps: Tensor      # [Tn] fp32
    positions: Tensor       # [Tn,A,3]
    rotations_6d: Tensor    # [Tn,A,6]
    present: Tensor         # [Tn,A] bool
    bounds: Tensor          # [A,3]
    grid: GridSpec
    tables: List[Tensor]    # A tables [L*T, F] fp32, already ordered by actor_to_id
    actor_scale: float = 10.0

    def c_actors(self):
        # plain pointers + sizes: valid while this spec's tensors are the same storage and `present` is unedited -- re-built
        # when one of them is re-assigned or `present` is written in place
        key = (self.timestamps.data_ptr(), self.positions.data_ptr(), self.rotations_6d.data_ptr(), self.present.data_ptr(),
               self.present._version, self.bounds.data_ptr(), tuple(t.data_ptr() for t in self.tables), self.actor_scale)
        cached = getattr(self, "_c_actors", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        present = self.present.contiguous()
        present = present.view(torch.uint8) if present.dtype == torch.bool else present.to(torch.uint8)  # bool is 1 byte
        keep = [_chk(self.timestamps, "timestamps"), _chk(self.positions, "positions"),
                _chk(self.rotations_6d, "rotations_6d"), present, _chk(self.bounds, "bounds")]
        tabs = [_chk(t, "actor table", self.tables[0].dtype) for t in self.tables]  # one storage type (fp32 | fp16)
        # device array of table pointers: uploaded once per set of tables, not once per call (a pageable H2D copy
        # synchronises the host with the stream)
        ptrs = _ptr_array(tabs)
        a = _lib.Actors()
        a.n_times, a.n_actors = self.positions.shape[0], self.positions.shape[1]
        a.timestamps, a.positions, a.rotations_6d = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
        a.present, a.bounds = keep[3].data_ptr(), keep[4].data_ptr()
        a.grid = self.grid.c_grid(tabs[0])
        a.tables = ptrs.data_ptr()
        a.actor_scale = float(self.actor_scale)
        a.max_candidates = a.n_actors  # per-ray lists as long as the actor count: no ray can overflow, no host check
        self._c_actors = (key, (a, (keep, tabs, ptrs)))
        return self._c_actors[1]


def actor_prepare(spec: ActorSpec, origins, directions, pixel_area, starts, ends, times, edit: Optional[dict] = None):
    """-> (cand_count [R] i32, cand_actor [R,K] i32, cand_w2b [R,K,12], None) with K = the number of actors, so every
    actor a ray passes fits (the reference has no limit either); R*K*52 bytes, e.g. 300 MB for 57 344 rays x 100 actors.
    edit: DynamicActors.actor_editing (lateral / longitudinal / height / rotation / index, dynamic_actors.py:53-59) for an
    eval-time move of the boxes (nrhip_actor_prepare_edited), None: the trajectories as they are."""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    a, keep2 = spec.c_actors()
    R, K, dev = r.n_rays, a.max_candidates, origins.device
    t = _chk(times.reshape(-1), "times")
    cnt = torch.empty((R,), dtype=torch.int32, device=dev)
    act = torch.empty((R, K), dtype=torch.int32, device=dev)  # only the first cnt[r] entries of a row are ever read
    w2b = torch.empty((R, K, 12), dtype=torch.float32, device=dev)
    if edit is None:
        launch("nrhip_actor_prepare", a, r, t, cnt, act, w2b, None)
    else:
        e = _lib.ActorEdit(float(edit.get("lateral", 0.0)), float(edit.get("longitudinal", 0.0)),
                           float(edit.get("height", 0.0)), float(edit.get("rotation", 0.0)), int(edit.get("index", -1)))
        launch("nrhip_actor_prepare_edited", a, r, t, e, cnt, act, w2b, None)
    return cnt, act, w2b, None


def actor_prepare_line(spec: ActorSpec, origins, directions, t0, t1, times, edit: Optional[dict] = None):
    """``actor_prepare`` for rays that have no [R,S] sample edges (the packed samples of an occupancy march): one candidate
    list per RAY from the ray's line through origins + directions * t0 and origins + directions * t1 (floats or [R] tensors;
    finite, t0 != t1).  The cull measures the distance to the infinite line, so any two distinct points give the candidates
    of every sample on the ray.  Nothing is sized by the number of samples."""
    o = _chk(origins, "origins")
    R, dev = o.shape[0], o.device
    col = lambda t: (t.reshape(R).float() if isinstance(t, Tensor) else torch.full((R,), float(t), device=dev))  # noqa: E731
    ends = torch.stack([col(t0), col(t1)], dim=1)  # two zero-length samples: their means are the two points
    area = torch.zeros((R,), device=dev, dtype=torch.float32)  # (enters a sample's std only, which the cull does not read)
    return actor_prepare(spec, o, directions, area, ends, ends, times, edit=edit)


def actor_encode(spec: ActorSpec, cand, origins, directions, pixel_area, starts, ends, features: Tensor,
                 ray_flip: Optional[Tensor] = None):
    """Overwrites the rows of ``features`` [N,out_dim] whose sample lies inside an actor box (in place).
    -> (directions [N,3], hit_actor [N] int32: actor index or -1)"""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    a, keep2 = spec.c_actors()
    cnt, act, w2b, _ = cand
    n = r.n_rays * r.n_samples
    feats = _chk(features, "features")
    assert feats.data_ptr() == features.data_ptr(), "features must be contiguous (updated in place)"
    dirs = torch.empty((n, 3), dtype=torch.float32, device=feats.device)
    hit = torch.empty((n,), dtype=torch.int32, device=feats.device)
    launch("nrhip_actor_encode", a, r, cnt, act, w2b, feats.shape[1], feats, dirs, hit, _opt(ray_flip, "ray_flip"))
    return dirs, hit  # int32: actor index or -1


def actor_pair_positions(spec: ActorSpec, origins, directions, pixel_area, starts, ends, times, sample_idx: Tensor,
                         actor_idx: Tensor, ray_flip: Optional[Tensor] = None):
    """Box-frame, contracted position of (sample, actor) pairs.  sample_idx [P] int64 flat sample index, actor_idx [P]
    int32.  -> (x01 [P,3] in [0,1]^3, cstd [P])"""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    a, keep2 = spec.c_actors()
    si, ai = _chk(sample_idx, "sample_idx", torch.int64), _chk(actor_idx, "actor_idx", torch.int32)
    P_ = si.shape[0]
    x01 = torch.empty((P_, 3), dtype=torch.float32, device=si.device)
    cstd = torch.empty((P_,), dtype=torch.float32, device=si.device)
    launch("nrhip_actor_pair_positions_fwd", a, r, _chk(times.reshape(-1), "times"), si, ai, _opt(ray_flip, "ray_flip"), P_,
           x01, cstd)
    return x01, cstd


def actor_pair_positions_bwd(spec: ActorSpec, origins, directions, pixel_area, starts, ends, times, sample_idx, actor_idx,
                             ray_flip, grad_x01: Tensor, grad_cstd: Tensor, ray_grads: bool = False):
    """-> (grad actor_positions [Tn,A,3], grad actor_rotations_6d [Tn,A,6]); with ``ray_grads`` also (grad origins [R,3],
    grad directions [R,3]): the in-box samples' world positions move with the ray (camera optimizer)"""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    a, keep2 = spec.c_actors()
    si, ai = _chk(sample_idx, "sample_idx", torch.int64), _chk(actor_idx, "actor_idx", torch.int32)
    flat = torch.zeros((a.n_times * a.n_actors * 9,), dtype=torch.float32, device=si.device)
    gp = flat[: a.n_times * a.n_actors * 3].view(a.n_times, a.n_actors, 3)
    gr = flat[a.n_times * a.n_actors * 3:].view(a.n_times, a.n_actors, 6)
    common = (a, r, _chk(times.reshape(-1), "times"), si, ai, _opt(ray_flip, "ray_flip"), si.shape[0],
              _chk(grad_x01, "grad_x01"), _chk(grad_cstd, "grad_cstd"), gp, gr)
    if not ray_grads:
        launch("nrhip_actor_pair_positions_bwd", *common)
        return gp, gr
    god = torch.zeros((2, r.n_rays, 3), dtype=torch.float32, device=si.device)
    launch("nrhip_actor_pair_positions_bwd_rays", *common, god[0], god[1])
    return gp, gr, god[0], god[1]


def actor_hits(spec: ActorSpec, cand, origins, directions, pixel_area, starts, ends) -> Tensor:
    """-> hits [N,8] int32: the actors whose boxes contain the sample, ascending, padded with -1"""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    a, keep2 = spec.c_actors()
    cnt, act, w2b, _ = cand
    hits = torch.empty((r.n_rays * r.n_samples, _lib.MAX_SAMPLE_CONTAINMENTS), dtype=torch.int32, device=origins.device)
    launch("nrhip_actor_hits", a, r, cnt, act, w2b, hits)
    return hits


def actor_pairs(hits: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (sample_idx int64 [P], actor_idx int32 [P]): every (sample, containing actor) of a hits table in (sample, slot)
    order -- `(hits >= 0).nonzero()` + `hits[idx, slot]` without the rocprim partition, the gather and the casts (one host
    read of P, which nonzero needs as well)"""
    h = _chk(hits, "hits", torch.int32)
    n = h.shape[0]
    nblk = (n + 1023) // 1024
    off = torch.empty((max(nblk, 1),), dtype=torch.int32, device=h.device)
    total = torch.empty((1,), dtype=torch.int64, device=h.device)
    launch("nrhip_actor_pairs_count", h, n, off, total)
    P_ = int(total.item())
    si = torch.empty((P_,), dtype=torch.int64, device=h.device)
    ai = torch.empty((P_,), dtype=torch.int32, device=h.device)
    if P_:
        launch("nrhip_actor_pairs_write", h, n, off, total, si, ai)
    return si, ai


def actor_density(spec: ActorSpec, cand, origins, directions, pixel_area, starts, ends, decoder_weight: Tensor,
                  density: Tensor, ray_flip: Optional[Tensor] = None, return_actor: bool = False):
    """Overwrites density [R,S] (in place) where the sample lies inside an actor box.  -> hit [R,S] bool (return_actor: the
    int32 index of the actor the kernel used -- the highest index containing the sample -- or -1)"""
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends)
    a, keep2 = spec.c_actors()
    cnt, act, w2b, _ = cand
    dw = _chk(decoder_weight.reshape(-1), "decoder_weight")
    dens = _chk(density, "density")
    assert dens.data_ptr() == density.data_ptr(), "density must be contiguous (updated in place)"
    hit = torch.empty((r.n_rays, r.n_samples), dtype=torch.int32, device=dens.device)
    launch("nrhip_actor_density", a, r, cnt, act, w2b, dw, dw.numel(), dens, hit, _opt(ray_flip, "ray_flip"))
    return hit if return_actor else hit >= 0


def occgrid_level_aabbs(roi_aabb, levels: int) -> Tensor:
    """CPU fp32 [L,6]: level l is the level-0 box scaled by 2^l about its centre (centre and half extent in fp32)"""
    a = torch.as_tensor(roi_aabb, dtype=torch.float32).reshape(6).cpu()
    centre, half = (a[:3] + a[3:]) * 0.5, (a[3:] - a[:3]) * 0.5
    return torch.stack([torch.cat([centre - half * float(2 ** l), centre + half * float(2 ** l)]) for l in range(levels)])


@dataclass
class OccGridSpec:
    aabb: Tensor       # [6] min xyz, max xyz -- or [L,6], one box per level (any device; read on the host)
    binaries: Tensor   # [res,res,res] -- or [L,res,res,res] -- bool / uint8 on the GPU

    def _bytes(self, in_place: bool = False) -> Tensor:
        b = self.binaries
        if not b.is_cuda or b.dim() not in (3, 4) or b.shape[-3] != b.shape[-2] or b.shape[-2] != b.shape[-1]:
            raise ValueError("binaries must be a cubic [res,res,res] or [L,res,res,res] GPU tensor")
        if b.is_contiguous() and b.dtype in (torch.bool, torch.uint8):
            return b.view(torch.uint8)  # a bool is one byte, 0 or 1: no copy
        if in_place:
            raise ValueError("binaries must be a contiguous bool / uint8 tensor to be updated in place")
        return b.to(torch.uint8).contiguous()

    def c_grid(self):
        b8 = self._bytes()
        if b8.dim() != 3:
            raise ValueError("binaries must be a cubic [res,res,res] GPU tensor")
        g = _lib.OccGrid()
        for i, v in enumerate(self.aabb.reshape(-1).tolist()):
            g.aabb[i] = v
        g.resolution, g.binaries = b8.shape[0], b8.data_ptr()
        return g, b8

    @property
    def levels(self) -> int:
        return 1 if self.binaries.dim() == 3 else self.binaries.shape[0]

    @property
    def resolution(self) -> int:
        return self.binaries.shape[-1]

    def c_levels(self, in_place: bool = False):
        """nrhip_occgrid_levels of a [L,res,res,res] (or [res,res,res]) grid; aabb [6] is expanded to the L nested boxes"""
        b8 = self._bytes(in_place)
        L = self.levels
        if not 1 <= L <= _lib.OCCGRID_MAX_LEVELS:
            raise ValueError(f"occupancy grid with {L} levels (1..{_lib.OCCGRID_MAX_LEVELS})")
        boxes = torch.as_tensor(self.aabb, dtype=torch.float32)
        boxes = occgrid_level_aabbs(boxes, L) if boxes.numel() == 6 and L > 1 else boxes.reshape(-1, 6)
        if boxes.shape[0] != L:
            raise ValueError(f"{boxes.shape[0]} boxes for {L} levels")
        g = _lib.OccGridLevels()
        g.levels, g.resolution, g.binaries = L, b8.shape[-1], b8.data_ptr()
        for l, box in enumerate(boxes.tolist()):
            for i, v in enumerate(box):
                g.aabbs[l][i] = v
        return g, b8


def actor_density_splice_fwd(density: Tensor, rows: Tensor, weight: Tensor, sample_idx: Tensor, winner: Tensor):
    """density [N] is overwritten at the hit samples by trunc_exp(rows . weight) of their winning pair -> logit [P]"""
    rows, weight = _chk(rows, "rows"), _chk(weight, "weight")
    idx, win = _chk(sample_idx, "sample_idx", torch.int64), winner.contiguous().view(torch.uint8) if winner.dtype == torch.bool else _chk(winner, "winner", torch.uint8)
    P, la = rows.shape
    if weight.numel() != la or idx.shape[0] != P or win.shape[0] != P or density.dtype != torch.float32 or not density.is_contiguous():
        raise ValueError("actor_density_splice_fwd: shapes")
    logit = torch.empty((P,), device=rows.device, dtype=torch.float32)
    launch("nrhip_actor_density_splice_fwd", rows, la, weight, idx, win, P, density, logit)
    return logit


def actor_density_splice_bwd(rows, weight, sample_idx, winner, logit, density_out, grad_out: Tensor):
    """-> grad_density [N] (grad_out, zero at the hit samples), grad_rows [P, la], grad_weight [la]"""
    rows, weight = _chk(rows, "rows"), _chk(weight, "weight")
    idx = _chk(sample_idx, "sample_idx", torch.int64)
    win = winner.contiguous().view(torch.uint8) if winner.dtype == torch.bool else _chk(winner, "winner", torch.uint8)
    g = _chk(grad_out.reshape(-1), "grad_out")
    P, la = rows.shape
    g_dens = g.clone()
    g_rows = torch.empty_like(rows)
    g_w = torch.zeros((la,), device=rows.device, dtype=torch.float32)
    launch("nrhip_actor_density_splice_bwd", rows, la, weight, idx, win, _chk(logit, "logit"),
           _chk(density_out.reshape(-1), "density_out"), g, P, g_dens, g_rows, g_w)
    return g_dens, g_rows, g_w


def occgrid_march(grid: OccGridSpec, origins, directions, render_step_size, near_plane=0.0, far_plane=1e10,
                  t_min=None, t_max=None, cone_angle=0.0, t_rand=None, max_candidates=1 << 16, actor_boxes=None):
    """Two-pass packed march: count -> exclusive prefix sum (one host sync for the allocation, like nerfacc) -> write.
    -> (ray_indices int64 [M], t_starts [M], t_ends [M], segments int64 [R+1])
    max_candidates: candidate intervals per ray, counted before the occupancy test -- the first max_candidates intervals of
    the ray's tiling are looked at, kept or not, and the ray ends there.
    actor_boxes = (ActorSpec, cand): the box-aware march (nrhip_occgrid_march_levels_actors) -- an interval whose cell is
    empty is kept all the same when its sample lies inside the box of one of the ray's candidate actors (cand = the per-RAY
    lists of ``actor_prepare`` / ``actor_prepare_line`` at the ray's time).  None: the plain march."""
    o, d = _chk(origins, "origins"), _chk(directions, "directions")
    R, dev = o.shape[0], o.device
    head: tuple = ()
    if actor_boxes is not None:
        spec, cand = actor_boxes
        a, keep_a = spec.c_actors()
        cnt, act, w2b = (_chk(cand[0], "cand_count", torch.int32), _chk(cand[1], "cand_actor", torch.int32),
                         _chk(cand[2], "cand_w2b"))
        if cnt.shape != (R,) or act.shape != (R, a.max_candidates) or w2b.shape != (R, a.max_candidates, 12):
            raise ValueError(f"occgrid_march: candidate lists must be [R], [R,K], [R,K,12] with R = {R}, K = "
                             f"{a.max_candidates}: one list per ray")
        g, keep = grid.c_levels()
        entry, head = "nrhip_occgrid_march_levels_actors", (a, cnt, act, w2b)
    elif grid.binaries.dim() == 4:  # [L,res,res,res]: the levels-aware entry point (L = 1: the same samples bit for bit)
        g, keep = grid.c_levels()
        entry = "nrhip_occgrid_march_levels"
    else:
        g, keep = grid.c_grid()
        entry = "nrhip_occgrid_march"
    counts = torch.zeros((R,), dtype=torch.int32, device=dev)
    args = (g, *head, o, d, _opt(t_min, "t_min"), _opt(t_max, "t_max"), _opt(t_rand, "t_rand"), R, float(render_step_size),
            float(near_plane), float(far_plane), float(cone_angle), int(max_candidates))
    launch(entry, *args, counts, None, None, None, None)
    seg = torch.zeros((R + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=seg[1:])
    M = int(seg[-1].item()) if R else 0
    ri = torch.empty((M,), dtype=torch.int64, device=dev)
    ts = torch.empty((M,), dtype=torch.float32, device=dev)
    te = torch.empty((M,), dtype=torch.float32, device=dev)
    if M:
        launch(entry, *args, None, seg, ri, ts, te)
    return ri, ts, te, seg


# ---- occupancy-grid maintenance (csrc/occgrid_update.h states the rule; parity with nerfacc itself is unpinned) ----------
def occgrid_update_scratch(levels: int, resolution: int, device) -> dict:
    """The device scratch of a grid, allocated (zero-filled) once and kept by its owner -- shims.nerfacc.OccGridEstimator
    caches it: the kernels' workspace plus the fixed-capacity candidate buffers of both regimes, filled on first use."""
    ws, _ = _workspace("nrhip_occgrid_update_workspace", int(levels), int(resolution), device=device, dtype=torch.uint8)
    return {"levels": int(levels), "resolution": int(resolution), "workspace": ws.zero_()}


def _occ_scratch(grid: OccGridSpec, scratch: Optional[dict], device) -> dict:
    if scratch is None:
        return occgrid_update_scratch(grid.levels, grid.resolution, device)
    if scratch["levels"] != grid.levels or scratch["resolution"] != grid.resolution or scratch["workspace"].device != device:
        raise ValueError("occgrid scratch belongs to a grid of another shape or device")
    return scratch


def occgrid_update_capacity(resolution: int, warmup: bool, n: Optional[int] = None) -> Tuple[int, int]:
    """(n, capacity per level): n = res^3 // 4 draws; res^3 slots during warm-up, 2 n after it"""
    n = resolution ** 3 // 4 if n is None else int(n)
    return n, (resolution ** 3 if warmup else 2 * n)


def occgrid_update_candidates(grid: OccGridSpec, occs: Tensor, warmup: bool, n: Optional[int] = None,
                              cell_draws: Optional[Tensor] = None, sel_draws: Optional[Tensor] = None,
                              jitter: Optional[Tensor] = None, scratch: Optional[dict] = None):
    """-> cell_ids int32 [L,cap] (-1 behind the level's count), counts int32 [L], positions fp32 [L*cap,3].
    The draws (cell_draws int64 [L,n], sel_draws fp32 [L,n], jitter fp32 [L,cap,3]) are made on the device when not given.
    The outputs live in ``scratch`` when one is passed: the next call of the same regime overwrites them."""
    occs = _chk(occs, "occs")
    L, res, dev = grid.levels, grid.resolution, occs.device
    if occs.numel() != L * res ** 3:
        raise ValueError(f"occs has {occs.numel()} elements for {L} x {res}^3 cells")
    n, cap = occgrid_update_capacity(res, warmup, n)
    sc = _occ_scratch(grid, scratch, dev)
    if not warmup:
        if cell_draws is None:
            cell_draws = torch.randint(0, res ** 3, (L, n), dtype=torch.int64, device=dev)
        if sel_draws is None:
            sel_draws = torch.rand((L, n), dtype=torch.float32, device=dev)
        cell_draws, sel_draws = _chk(cell_draws, "cell_draws", torch.int64), _chk(sel_draws, "sel_draws")
        if tuple(cell_draws.shape) != (L, n) or tuple(sel_draws.shape) != (L, n):
            raise ValueError(f"cell_draws / sel_draws must be [{L},{n}]")
    if jitter is None:
        jitter = torch.rand((L, cap, 3), dtype=torch.float32, device=dev)
    jitter = _chk(jitter, "jitter")
    if tuple(jitter.shape) != (L, cap, 3):
        raise ValueError(f"jitter must be [{L},{cap},3], got {tuple(jitter.shape)}")
    key = ("cand", bool(warmup), n)
    if key not in sc:
        sc[key] = (torch.empty((L, cap), dtype=torch.int32, device=dev), torch.zeros((L,), dtype=torch.int32, device=dev),
                   torch.empty((L * cap, 3), dtype=torch.float32, device=dev))
    ids, counts, pos = sc[key]
    g, keep = grid.c_levels()
    ws = sc["workspace"]
    launch("nrhip_occgrid_update_candidates", g, occs, int(bool(warmup)), n, cell_draws if not warmup else None,
           sel_draws if not warmup else None, jitter, ids, counts, pos, ws, ws.numel())
    return ids, counts, pos


def occgrid_update_apply(grid: OccGridSpec, occs: Tensor, cell_ids: Tensor, counts: Tensor, occ_values: Tensor,
                         ema_decay: float = 0.95, occ_thre: float = 1e-2, scratch: Optional[dict] = None) -> None:
    """In place: the EMA of ``occs`` at the candidates' cells (max over a cell's candidates, decay once), then
    ``grid.binaries = occs > min(mean of the visible occs, occ_thre)``."""
    occs = _chk(occs, "occs")
    if not occs.is_contiguous():
        raise ValueError("occs must be contiguous (updated in place)")
    ids, counts = _chk(cell_ids, "cell_ids", torch.int32), _chk(counts, "counts", torch.int32)
    L, res = grid.levels, grid.resolution
    if ids.dim() != 2 or ids.shape[0] != L or counts.numel() != L or occs.numel() != L * res ** 3:
        raise ValueError("occgrid_update_apply: cell_ids [L,cap], counts [L], occs [L*res^3]")
    vals = _chk(occ_values.reshape(-1), "occ_values")
    if vals.numel() != ids.numel():
        raise ValueError(f"occ_values has {vals.numel()} elements for {ids.numel()} candidate slots")
    sc = _occ_scratch(grid, scratch, occs.device)
    g, keep = grid.c_levels(in_place=True)
    ws = sc["workspace"]
    launch("nrhip_occgrid_update_apply", g, occs, ids.shape[1], ids, counts, vals, float(ema_decay), float(occ_thre), ws,
           ws.numel())


def occgrid_update(grid: OccGridSpec, occs: Tensor, occ_eval_fn, step: int, occ_thre: float = 1e-2, ema_decay: float = 0.95,
                   warmup_steps: int = 256, n: Optional[int] = None, cell_draws=None, sel_draws=None, jitter=None,
                   scratch: Optional[dict] = None):
    """One update of (occs, grid.binaries), in place: candidates -> ``occ_eval_fn(positions [L*cap,3])`` once -> EMA ->
    threshold.  No host synchronisation and no allocation sized by data.  -> (cell_ids, counts, positions)"""
    ids, counts, pos = occgrid_update_candidates(grid, occs, step < warmup_steps, n, cell_draws, sel_draws, jitter, scratch)
    vals = occ_eval_fn(pos).reshape(-1).float() if pos.shape[0] else pos.new_empty((0,))
    occgrid_update_apply(grid, occs, ids, counts, vals, ema_decay, occ_thre, scratch)
    return ids, counts, pos


def occgrid_mark_invisible(grid: OccGridSpec, occs: Tensor, K: Tensor, c2w: Tensor, width: int, height: int,
                           near_plane: float = 0.0) -> None:
    """In place: occs = 0 on the cells some camera sees (and none sees closer than near_plane), -1 -- and the binary
    cleared -- on the others.  K [N,3,3] or [1,3,3], c2w [N,3,4] or [N,4,4], OpenCV convention."""
    occs = _chk(occs, "occs")
    if not occs.is_contiguous() or occs.numel() != grid.levels * grid.resolution ** 3:
        raise ValueError("occs must be a contiguous fp32 [L*res^3] tensor")
    if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or c2w.dim() != 3 or tuple(c2w.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError("K must be [N,3,3] or [1,3,3] and c2w [N,3,4] or [N,4,4]")
    if K.shape[0] not in (1, c2w.shape[0]):
        raise ValueError(f"{K.shape[0]} intrinsics for {c2w.shape[0]} cameras")
    Kc, Mc = _chk(K, "K"), _chk(c2w[:, :3, :4], "c2w")
    g, keep = grid.c_levels(in_place=True)
    launch("nrhip_occgrid_mark_invisible", g, Kc, Kc.shape[0], Mc, Mc.shape[0], int(width), int(height), float(near_plane),
           occs)


def packed_visibility_from_alpha(alphas: Tensor, segments: Tensor, early_stop_eps: float, alpha_thre: float) -> Tensor:
    a = _chk(alphas.reshape(-1), "alphas")
    mask = torch.empty((a.shape[0],), dtype=torch.uint8, device=a.device)
    if a.shape[0]:
        launch("nrhip_packed_visibility_from_alpha", a, segments, segments.shape[0] - 1, float(early_stop_eps),
               float(alpha_thre), mask)
    return mask.bool()


# ---- packed compositing (csrc/packed_composite.h): every op takes `segments` int64 [R+1], the march's fourth output ----
def _seg(segments: Tensor) -> Tuple[Tensor, int]:
    s = _chk(segments, "segments", torch.int64)
    if s.dim() != 1 or s.shape[0] < 1:
        raise ValueError("segments must be int64 [R+1]")
    return s, s.shape[0] - 1


def _flat(t: Tensor, name: str, m: Optional[int] = None) -> Tensor:
    t = _chk(t, name)
    t = t.reshape(-1)
    if m is not None and t.shape[0] != m:
        raise ValueError(f"{name}: {t.shape[0]} samples, expected {m}")
    return t


def packed_segments(ray_indices: Tensor, n_rays: int) -> Tensor:
    """sorted ray_indices int64 [M] with values in [0, n_rays) -> segments int64 [n_rays + 1]"""
    ri = _chk(ray_indices, "ray_indices", torch.int64).reshape(-1)
    seg = torch.empty((int(n_rays) + 1,), dtype=torch.int64, device=ri.device)
    launch("nrhip_packed_segments", ri, ri.shape[0], int(n_rays), seg)
    return seg


def packed_weight_from_density(t_starts, t_ends, sigmas, segments):
    """-> weights, trans, alphas [M]"""
    sg = _flat(sigmas, "sigmas")
    s, e = _flat(t_starts, "t_starts", sg.shape[0]), _flat(t_ends, "t_ends", sg.shape[0])
    seg, R = _seg(segments)
    w, t, a = torch.empty_like(sg), torch.empty_like(sg), torch.empty_like(sg)
    launch("nrhip_packed_weight_from_density", s, e, sg, seg, R, w, t, a)
    return w, t, a


def packed_weight_from_density_bwd(t_starts, t_ends, sigmas, segments, grad_w):
    sg = _flat(sigmas, "sigmas")
    s, e, gw = (_flat(v, n, sg.shape[0]) for v, n in ((t_starts, "t_starts"), (t_ends, "t_ends"), (grad_w, "grad_w")))
    seg, R = _seg(segments)
    gs = torch.empty_like(sg)
    launch("nrhip_packed_weight_from_density_bwd", s, e, sg, seg, gw, R, gs)
    return gs


def packed_weight_from_alpha(alphas, segments):
    """-> weights, trans [M]"""
    a = _flat(alphas, "alphas")
    seg, R = _seg(segments)
    w, t = torch.empty_like(a), torch.empty_like(a)
    launch("nrhip_packed_weight_from_alpha", a, seg, R, w, t)
    return w, t


def packed_weight_from_alpha_bwd(alphas, segments, grad_w, grad_t=None):
    a = _flat(alphas, "alphas")
    gw = _flat(grad_w, "grad_w", a.shape[0])
    gt = None if grad_t is None else _flat(grad_t, "grad_t", a.shape[0])
    seg, R = _seg(segments)
    ga = torch.empty_like(a)
    launch("nrhip_packed_weight_from_alpha_bwd", a, seg, gw, gt, R, ga)
    return ga


def packed_accumulate(weights, values, segments):
    """weights [M], values [M,C] or None -> [R,C] ([R,1] without values); rays without samples get zeros"""
    w = _flat(weights, "weights")
    seg, R = _seg(segments)
    v = None
    if values is not None:
        v = _chk(values, "values")
        if v.dim() != 2 or v.shape[0] != w.shape[0] or v.shape[1] < 1:
            raise ValueError("values must be [M,C] with one row per weight")
    Cc = 1 if v is None else v.shape[1]
    out = torch.empty((R, Cc), device=w.device, dtype=torch.float32)
    # an empty [0,C] tensor has no address, and NULL values mean "the plain sum": any non-null address stands in (no sample,
    # nothing is read through it; the rows of out are still zeroed by the kernel)
    launch("nrhip_packed_accumulate", w, out if (v is not None and v.numel() == 0) else v, seg, R, Cc, out)
    return out


def packed_accumulate_bwd(weights, values, g_out, segments, need_grad_weights=True, need_grad_values=True):
    """-> (grad weights [M] or None, grad values [M,C] or None)"""
    w = _flat(weights, "weights")
    seg, R = _seg(segments)
    v = None if values is None else _chk(values, "values")
    Cc = 1 if v is None else v.shape[1]
    g = _chk(g_out, "g_out")
    if g.shape != (R, Cc):
        raise ValueError(f"g_out must be [{R},{Cc}]")
    gw = torch.empty_like(w) if need_grad_weights else None
    gv = torch.empty_like(v) if (need_grad_values and v is not None) else None
    if w.numel():  # (no samples: nothing to write, and an empty values tensor has no address to tell it from "plain sum")
        launch("nrhip_packed_accumulate_bwd", w, v, g, seg, R, Cc, gw, gv)
    return gw, gv


def packed_composite_fwd(t_starts, t_ends, sigmas_or_alphas, features, segments, density_mode: bool,
                         return_weights: bool = True):
    """fused packed compositing -> features [R,C], depth [R,1] (sum w mid), accumulation [R,1], weights [M] or None"""
    x = _flat(sigmas_or_alphas, "sigmas" if density_mode else "alphas")
    M = x.shape[0]
    s, e = _flat(t_starts, "t_starts", M), _flat(t_ends, "t_ends", M)
    f = _chk(features, "features")
    if f.dim() != 2 or f.shape[0] != M or f.shape[1] < 1:
        raise ValueError("features must be [M,C] with one row per sample")
    seg, R = _seg(segments)
    Cc = f.shape[1]
    of = torch.empty((R, Cc), device=x.device, dtype=torch.float32)
    od = torch.empty((R, 1), device=x.device, dtype=torch.float32)
    oa = torch.empty((R, 1), device=x.device, dtype=torch.float32)
    ow = torch.empty_like(x) if return_weights else None
    launch("nrhip_packed_composite_fwd", s, e, x, f, seg, R, Cc, 1 if density_mode else 0, of, od, oa, ow)
    return of, od, oa, ow


# ---- median (quantile) depth (csrc/median_depth.hip; the contract: include/neurad_hip.h at nrhip_median_depth) ----
MEDIAN_MAX_THRESHOLDS = _lib.MEDIAN_MAX_THRESHOLDS


def _thresholds(thresholds) -> Tuple[C.Array, int]:
    """-> (host float array, K); the count and the values are checked by the library (1 <= K <= 8, finite)"""
    q = [float(v) for v in thresholds]
    return (C.c_float * len(q))(*q), len(q)


def median_depth(weights, starts, ends, thresholds=(0.5,), return_index: bool = False):
    """weights, starts, ends [R,S] -> depth [R,K]: per threshold q the midpoint of the first sample at which
    float32(float64 running sum of the weights) is not below q, the last sample if none is; with ``return_index`` also that
    sample's index, int32 [R,K].  One pass serves all K thresholds.  No gradient."""
    w = _chk(weights, "weights")
    if w.dim() != 2:
        raise ValueError("weights must be [R,S]")
    R, S = w.shape
    s, e = _chk(starts, "starts"), _chk(ends, "ends")
    if s.shape != w.shape or e.shape != w.shape:
        raise ValueError(f"starts / ends must be [{R},{S}] like weights")
    q, K = _thresholds(thresholds)
    od = torch.empty((R, K), device=w.device, dtype=torch.float32)
    oi = torch.empty((R, K), device=w.device, dtype=torch.int32) if return_index else None
    launch("nrhip_median_depth", w, s, e, R, S, q, K, od, oi)
    return (od, oi) if return_index else od


def median_depth_packed(weights, t_starts, t_ends, segments, thresholds=(0.5,), return_index: bool = False):
    """the same over packed samples: weights, t_starts, t_ends [M], segments int64 [R+1] -> depth [R,K] (, index int32
    [R,K]); a ray without samples gets depth 0 and index -1"""
    w = _flat(weights, "weights")
    M = w.shape[0]
    s, e = _flat(t_starts, "t_starts", M), _flat(t_ends, "t_ends", M)
    seg, R = _seg(segments)
    q, K = _thresholds(thresholds)
    od = torch.empty((R, K), device=w.device, dtype=torch.float32)
    oi = torch.empty((R, K), device=w.device, dtype=torch.int32) if return_index else None
    launch("nrhip_median_depth_packed", w if M else None, s if M else None, e if M else None, seg, R, M, q, K, od, oi)
    return (od, oi) if return_index else od


# ---- the per-sample loss terms on packed samples (csrc/losses.hip; the contracts: include/neurad_hip.h at
#      nrhip_packed_distortion_loss) ----
PACKED_DISTORTION_C = _lib.PACKED_DISTORTION_C


def packed_distortion_loss_rays(s_starts, s_ends, weights, segments, need_grad: bool = True):
    """distortion loss per ray of packed samples in its O(n) form: s_starts, s_ends, weights [M] (midpoints non-decreasing
    within a ray), segments int64 [R+1] -> loss_per_ray [R], d loss_per_ray / d weights [M] (or None); a ray without samples
    gets 0"""
    w = _flat(weights, "weights")
    M = w.shape[0]
    s, e = _flat(s_starts, "s_starts", M), _flat(s_ends, "s_ends", M)
    seg, R = _seg(segments)
    loss = torch.empty((R,), device=w.device, dtype=torch.float32)
    g = torch.empty_like(w) if need_grad else None
    launch("nrhip_packed_distortion_loss", s if M else None, e if M else None, w if M else None, seg, R, M, loss,
           g if M else None)
    return loss, g


def packed_lidar_carving(t_starts, t_ends, segments, is_lidar: Tensor, did_return: Optional[Tensor], distance: Tensor,
                         carving_epsilon: float, non_return_lidar_distance: float, weights: Optional[Tensor] = None,
                         want_mask: bool = True, want_grad: bool = True):
    """``lidar_carving`` on packed samples: t_starts / t_ends [M], segments int64 [R+1], per-ray is_lidar / did_return (bool,
    did_return may be None = all returned) / distance -> (is_close [M] bool or None, loss_per_ray [R] or None, grad_weights [M]
    or None); the loss terms need ``weights`` [M]."""
    s = _flat(t_starts, "t_starts")
    M = s.shape[0]
    e = _flat(t_ends, "t_ends", M)
    seg, R = _seg(segments)
    w = None if weights is None else _flat(weights, "weights", M)
    if w is None and not want_mask:
        raise ValueError("packed_lidar_carving: nothing to compute (no weights and no mask)")
    u8 = lambda m: None if m is None else m.reshape(-1).contiguous().view(torch.uint8)  # noqa: E731  (bool is 1 byte)
    lid, ret = u8(is_lidar), u8(did_return)
    dist = _chk(distance.reshape(-1), "distance")
    for v, n in ((lid, "is_lidar"), (ret, "did_return"), (dist, "distance")):
        if v is not None and (v.shape[0] != R or v.device != s.device):
            raise ValueError(f"{n}: expected one value per ray ({R}) on {s.device}")
    dev = s.device
    close = torch.empty((M,), dtype=torch.bool, device=dev) if want_mask else None
    loss = torch.empty((R,), dtype=torch.float32, device=dev) if w is not None else None
    gw = torch.empty((M,), dtype=torch.float32, device=dev) if (w is not None and want_grad) else None
    if loss is None and M == 0:  # a mask of no samples: nothing to write
        return close, None, None
    some = lambda t: t if (t is not None and M) else None  # noqa: E731  (an empty tensor has no address)
    launch("nrhip_packed_lidar_carving", some(s), some(e), some(w), seg, lid, ret, dist, float(carving_epsilon),
           float(non_return_lidar_distance), R, M, some(close), loss, some(gw))
    return close, loss, gw


def _c_packed_rays(who: str, origins, directions, pixel_area, t_starts, t_ends, segments: Optional[Tensor] = None,
                   order: Optional[Tensor] = None):
    """-> (nrhip_packed_rays, the tensors it points to): per-RAY origins [R,3] / directions [R,3] / pixel_area [R], per-sample
    t_starts / t_ends [M], segments int64 [R+1] (None: left NULL, for the entry points that take ray_indices instead), optional
    processing order int32 [R]"""
    o, d, a = _ray_constants(origins, directions, pixel_area)
    seg, R = (None, o.shape[0]) if segments is None else _seg(segments)
    if o.shape != (R, 3) or d.shape != (R, 3) or a.shape != (R,):
        raise ValueError(f"{who}: origins / directions [R,3] and pixel_area [R]"
                         + ("" if seg is None else f" with R = {R} = len(segments) - 1"))
    s = _flat(t_starts, "t_starts")
    e = _flat(t_ends, "t_ends", s.shape[0])
    r = _lib.PackedRays()
    r.n_rays, r.n_samples = R, s.shape[0]
    r.origins, r.directions, r.pixel_area = o.data_ptr(), d.data_ptr(), a.data_ptr()
    r.t_starts, r.t_ends = s.data_ptr(), e.data_ptr()
    if seg is not None:
        r.segments = seg.data_ptr()
    return r, (o, d, a, s, e, seg, _ray_order(r, order))


def _c_ray_candidates(who: str, cand, R: int, K: int):
    """one candidate list per RAY (``actor_prepare_line``), checked: -> cand_count int32 [R], cand_actor int32 [R,K],
    cand_w2b [R,K,12]"""
    cnt, act, w2b = (_chk(cand[0], "cand_count", torch.int32), _chk(cand[1], "cand_actor", torch.int32),
                     _chk(cand[2], "cand_w2b"))
    if cnt.shape != (R,) or act.shape != (R, K) or w2b.shape != (R, K, 12):
        raise ValueError(f"{who}: candidate lists must be [R], [R,K], [R,K,12] with R = {R}, K = {K}: one list per ray")
    return cnt, act, w2b


def render_fwd_packed(fs: FieldSpec, origins, directions, pixel_area, t_starts, t_ends, segments,
                      return_weights: bool = False, early_stop_eps: float = 0.0, order: Optional[Tensor] = None):
    """The fused render kernel on the march's packed samples: per-RAY origins [R,3] / directions [R,3] / pixel_area [R],
    per-sample t_starts / t_ends [M], segments int64 [R+1] -> features [R,32], depth [R,1] (sum w mid, not normalised),
    accumulation [R,1] (, weights [M]); compositing as ``packed_composite_fwd`` (no sky residual, zeros for a ray without
    samples).  early_stop_eps / order: see ``render_fwd``."""
    r, keep = _c_packed_rays("render_fwd_packed", origins, directions, pixel_area, t_starts, t_ends, segments, order)
    f, keep2 = fs.c_field()
    feats, depth, acc, _ = _render_outputs(r.n_rays, 0, keep[0].device, False)
    w = torch.empty_like(keep[3]) if return_weights else None
    launch("nrhip_render_fwd_packed", f, r, feats, depth, acc, w, float(early_stop_eps))
    return (feats, depth, acc, w) if return_weights else (feats, depth, acc)


def render_fwd_packed_actors(fs: FieldSpec, spec: "ActorSpec", cand, origins, directions, pixel_area, t_starts, t_ends,
                             segments, return_weights: bool = False, early_stop_eps: float = 0.0,
                             order: Optional[Tensor] = None, out=None):
    """``render_fwd_packed`` for a scene with dynamic actors, still one route of three launches and no per-sample tensor:
    cand = one candidate list per RAY (``actor_prepare_line``).  Same outputs and compositing as ``render_fwd_packed``.
    ``out``: the buffers to write into, (features [R,32], depth [R,1], accumulation [R,1], weights [M] or None)."""
    r, keep = _c_packed_rays("render_fwd_packed_actors", origins, directions, pixel_area, t_starts, t_ends, segments, order)
    f, keep2 = fs.c_field()
    a, keep3 = spec.c_actors()
    R, dev = r.n_rays, keep[0].device
    cnt, act, w2b = _c_ray_candidates("render_fwd_packed_actors", cand, R, a.max_candidates)
    feats, depth, acc, _ = _render_outputs(R, 0, dev, False, None if out is None else tuple(out[:3]))
    w = (torch.empty_like(keep[3]) if out is None or out[3] is None else _flat(out[3], "weights", keep[3].shape[0])) \
        if return_weights else None
    work = torch.empty((R + 4,), device=dev, dtype=torch.int32)
    launch("nrhip_render_fwd_packed_actors", f, a, r, cnt, act, w2b, feats, depth, acc, w, float(early_stop_eps), work)
    return (feats, depth, acc, w) if return_weights else (feats, depth, acc)


def field_fwd_train_packed(fs: FieldSpec, origins, directions, pixel_area, t_starts, t_ends, segments,
                           order: Optional[Tensor] = None, out=None, override=None):
    """``field_fwd_train`` on the march's packed samples (ray constants per RAY, every row at the packed sample index):
    -> (feature [M,32], geo_out [M], head [M]), (enc [M,L*F], geo_hidden [M,H], feat_in [M,48], feat_hidden [M,2H]).
    ``out``: the seven buffers to write into (rows past M are left alone).
    override = (ovr_row int32 [M] (row index or -1, at the packed sample index), ovr_rows [P,L*F], ovr_dirs [P,3]): as
    ``field_fwd_train`` (nrhip_field_fwd_train_packed_ovr)."""
    r, keep = _c_packed_rays("field_fwd_train_packed", origins, directions, pixel_area, t_starts, t_ends, segments, order)
    f, keep2 = fs.c_field()
    m, dev = r.n_samples, keep[0].device
    H, LF = fs.geo_w[0].shape[0], fs.grid.out_dim
    if out is None:
        mk = lambda *c: torch.empty((m, *c), device=dev, dtype=torch.float32)  # noqa: E731
        out = (mk(32), mk(), mk(), mk(LF), mk(H), mk(48), mk(2 * H))
    else:
        widths = (32, None, None, LF, H, 48, 2 * H)
        out = tuple(_chk(t, "out") for t in out)
        if len(out) != 7 or any(t.shape[0] < m or (t.shape[1:] != ((w,) if w else ())) for t, w in zip(out, widths)):
            raise ValueError("field_fwd_train_packed: out = (feature, geo_out, head, enc, geo_hidden, feat_in, feat_hidden)")
    if override is not None:
        ov, rows, dirs = override
        ov, rows, dirs = _chk(ov.reshape(-1), "ovr_row", torch.int32), _chk(rows, "ovr_rows"), _chk(dirs, "ovr_dirs")
        if ov.shape[0] != m or rows.dim() != 2 or rows.shape[1] != LF or dirs.shape != (rows.shape[0], 3):
            raise ValueError(f"field_fwd_train_packed: override = (int32 [M], [P,{LF}], [P,3])")
        launch("nrhip_field_fwd_train_packed_ovr", f, r, ov, rows, dirs, *out)
    else:
        launch("nrhip_field_fwd_train_packed", f, r, *out)
    return out[:3], out[3:]


# ---- surface normals from the geometry head (csrc/normals.hip; the contract: include/neurad_hip.h at nrhip_field_normals) ----
NORMALS_OUTPUTS = ("geo", "gradient", "normals", "ray_normals")
NORMALS_ACTOR_OUTPUTS = ("hit", "box_position")  # with ``actors`` only: whose normal a sample got, and where in that box
normals_c = _lib.normals_c  # NRHIP_NORMALS_C(L, F, H): the constant of the stated error bound
normals_actors_c = _lib.normals_actors_c  # NRHIP_NORMALS_ACTORS_C(La, F, H): the same for a sample inside a box


def _normals_want(who: str, want, weights, actors=None) -> Tuple[str, ...]:
    want = tuple(want) if want is not None else ("gradient", "normals") + (("ray_normals",) if weights is not None else ())
    names = NORMALS_OUTPUTS + (NORMALS_ACTOR_OUTPUTS if actors is not None else ())
    bad = [k for k in want if k not in names]
    if bad or not want:
        raise ValueError(f"{who}: want must name some of {names}, got {want}")
    if "ray_normals" in want and weights is None:
        raise ValueError(f"{who}: ray_normals needs weights")
    return want


def _normals_outputs(want, n: int, r: int, device) -> dict:
    mk = lambda *s: torch.empty(s, device=device, dtype=torch.float32)  # noqa: E731
    shapes = {"geo": (n,), "gradient": (n, 3), "normals": (n, 3), "ray_normals": (r, 3), "box_position": (n, 3)}
    out = {k: mk(*shapes[k]) for k in NORMALS_OUTPUTS + NORMALS_ACTOR_OUTPUTS[1:] if k in want}
    if "hit" in want:
        out["hit"] = torch.empty((n,), device=device, dtype=torch.int32)
    return out


def _normals_actor_args(who: str, actors, ray_flip, R: int):
    """``actors`` = (ActorSpec, cand), cand one candidate list per RAY (``actor_prepare`` / ``actor_prepare_line``), and the
    optional per-ray x flip -> (nrhip_actors, cand_count, cand_actor, cand_w2b, ray_flip, what keeps them alive)"""
    spec, cand = actors
    a, keep = spec.c_actors()
    cnt, act, w2b = _c_ray_candidates(who, cand, R, a.max_candidates)
    flip = _opt(ray_flip, "ray_flip")
    if flip is not None and flip.reshape(-1).shape[0] != R:
        raise ValueError(f"{who}: ray_flip must have one entry per ray ({R})")
    return a, cnt, act, w2b, flip, keep


def field_normals(fs: FieldSpec, origins, directions, pixel_area, starts, ends, weights: Optional[Tensor] = None,
                  want=None, order: Optional[Tensor] = None, actors=None, ray_flip: Optional[Tensor] = None) -> dict:
    """Normals of the geometry head at the samples' gaussian means, one kernel (nrhip_field_normals): ``geo`` [R,S] (the SDF
    or the pre-exp logit), ``gradient`` [R,S,3] = d geo / d position, ``normals`` [R,S,3] = +-gradient / max(|gradient|,
    1e-12) (+ for an SDF: towards free space; - in density mode) and, with ``weights`` [R,S] (a strided view is read in
    place), ``ray_normals`` [R,3] = sum_s w_s normals_s (not normalised; samples of weight zero are skipped).  ``want``
    names the outputs (default: gradient and normals, and ray_normals when weights are given) -> dict.  starts / ends as
    ``field_fwd`` (views into bin edges are read in place); ``order``: locality hint.  No gradient flows through any
    output.  Shapes the kernel is not instantiated for raise; ``field_normals_operators`` composes the same result.

    ``actors`` = (ActorSpec, cand) with cand one candidate list per RAY (``actor_prepare``): a scene with dynamic actors
    (nrhip_field_normals_actors).  A sample inside a box is differentiated through that actor's grid in the box frame and
    its gradient rotated to the world, g_world = W^T diag(f, 1, 1) g_box, of several boxes the highest actor index; a sample
    outside every box has the static call's bits.  ``ray_flip`` [R]: +-1 per ray (the training x flip).  ``want`` may then
    also name ``hit`` [R,S] int32 (the winning actor or -1) and ``box_position`` [R,S,3] (the box-frame position after the
    flip; untouched where hit < 0).  Without ``actors`` the call is the static one."""
    if actors is None and ray_flip is not None:
        raise ValueError("field_normals: ray_flip without actors")
    want = _normals_want("field_normals", want, weights, actors)
    r, keep = _c_rays(origins, directions, pixel_area, starts, ends, order)
    f, keep2 = fs.c_field()
    R, S = r.n_rays, r.n_samples
    w, wstride = None, 0
    if weights is not None:
        if not isinstance(weights, Tensor) or not weights.is_cuda or weights.dtype != torch.float32:
            raise _lib.NeuradHipError("field_normals: weights must be an fp32 GPU tensor (no CPU fallback)")
        if weights.shape != (R, S):
            raise ValueError(f"field_normals: weights must be [{R},{S}], got {tuple(weights.shape)}")
        w = weights if (S <= 1 or weights.stride(1) == 1) and (R <= 1 or weights.stride(0) >= S) else weights.contiguous()
        wstride = w.stride(0) if R > 1 and S > 0 else max(S, 1)
    out = _normals_outputs(want, R * S, R, keep[0].device)
    if not any(v.numel() for v in out.values()):  # (an empty batch has nothing to write, and no address to write it to)
        pass
    elif actors is None:
        launch("nrhip_field_normals", f, r, w, int(wstride), out.get("geo"), out.get("gradient"), out.get("normals"),
               out.get("ray_normals"))
    else:
        a, cnt, act, w2b, flip, keep3 = _normals_actor_args("field_normals", actors, ray_flip, R)
        launch("nrhip_field_normals_actors", f, a, r, cnt, act, w2b, flip, w, int(wstride), out.get("geo"),
               out.get("gradient"), out.get("normals"), out.get("ray_normals"), out.get("hit"), out.get("box_position"))
    return {k: (v if k == "ray_normals" else v.view(R, S, *v.shape[1:])) for k, v in out.items()}


def field_normals_packed(fs: FieldSpec, origins, directions, pixel_area, t_starts, t_ends, segments,
                         weights: Optional[Tensor] = None, want=None, order: Optional[Tensor] = None, actors=None,
                         ray_flip: Optional[Tensor] = None) -> dict:
    """``field_normals`` on the march's packed samples (nrhip_field_normals_packed): per-RAY origins / directions [R,3] and
    pixel_area [R], per-sample t_starts / t_ends [M], segments int64 [R+1], weights [M] -> ``geo`` [M], ``gradient`` [M,3],
    ``normals`` [M,3] at the packed sample index, ``ray_normals`` [R,3] (zeros for a ray without samples).  ``actors`` /
    ``ray_flip`` as ``field_normals`` (cand: ``actor_prepare_line``; nrhip_field_normals_packed_actors), with ``hit`` [M] and
    ``box_position`` [M,3]."""
    if actors is None and ray_flip is not None:
        raise ValueError("field_normals_packed: ray_flip without actors")
    want = _normals_want("field_normals_packed", want, weights, actors)
    r, keep = _c_packed_rays("field_normals_packed", origins, directions, pixel_area, t_starts, t_ends, segments, order)
    f, keep2 = fs.c_field()
    R, M = r.n_rays, r.n_samples
    w = None if weights is None else _flat(weights, "weights", M)
    out = _normals_outputs(want, M, R, keep[0].device)
    if not any(v.numel() for v in out.values()):
        pass
    elif actors is None:
        launch("nrhip_field_normals_packed", f, r, w if M else None, out.get("geo"), out.get("gradient"), out.get("normals"),
               out.get("ray_normals"))
    else:
        a, cnt, act, w2b, flip, keep3 = _normals_actor_args("field_normals_packed", actors, ray_flip, R)
        launch("nrhip_field_normals_packed_actors", f, a, r, cnt, act, w2b, flip, w if M else None, out.get("geo"),
               out.get("gradient"), out.get("normals"), out.get("ray_normals"), out.get("hit"), out.get("box_position"))
    return out


def field_normals_operators(fs: FieldSpec, origins, directions, pixel_area, starts, ends, weights: Optional[Tensor] = None,
                            want=None, actors=None, times: Optional[Tensor] = None, ray_flip: Optional[Tensor] = None,
                            edit: Optional[dict] = None) -> dict:
    """The result of ``field_normals`` composed from four operator kernels, for any grid and geometry MLP: encode_fwd ->
    mlp_fwd(save_hidden) -> mlp_bwd of a unit cotangent on column 0 -> encode_bwd_rays on [N,1] rays (the origin gradient
    of a one-sample ray is the gradient at its position).  Two [N, L*F] round trips and the MLP's weight gradients, which
    are dropped: the route for shapes the fused kernel does not cover and its timing baseline.  Same outputs and shapes.

    ``actors`` = (ActorSpec, cand) as ``field_normals``, with the rays' ``times`` [R] (the pair kernels place the boxes
    themselves): actor_encode splices the in-box rows over the static ones and names the winners; the winners' (sample,
    actor) pairs go through actor_pair_positions -> the actor grids' lookup and input gradient (hashgrid_multi_*) -> the
    rescale weights' std term -> actor_pair_positions_bwd with ray gradients on [N,1] rays, whose origin gradient is W^T
    diag(f, 1, 1) g_box; the static rows of in-box samples get a zero cotangent.  No new kernel.  The pair kernels know
    nothing of an eval-time actor ``edit``: with one the composition is refused by name."""
    want = _normals_want("field_normals_operators", want, weights, actors)
    if "box_position" in want:
        raise NotImplementedError("field_normals_operators: box_position is the fused kernel's output (the composition hands "
                                  "the pairs their contracted position only)")
    o, d, a = _ray_constants(origins, directions, pixel_area)
    starts, ends = _chk(starts, "starts"), _chk(ends, "ends")
    R, S = starts.shape
    n = R * S
    per = lambda t: t.repeat_interleave(S, dim=0) if S != 1 else t  # noqa: E731  (ray constants per sample)
    o1, d1, a1, s1, e1 = per(o), per(d), per(a), starts.reshape(n, 1), ends.reshape(n, 1)
    enc = encode_fwd(fs.grid, fs.table, fs.static_scale, o1, d1, a1, s1, e1)
    hit = None
    if actors is not None:
        if times is None:
            raise ValueError("field_normals_operators: actors need the rays' times")
        if edit is not None:
            raise NotImplementedError("field_normals_operators with dynamic actors and an eval-time actor edit: the pair "
                                      "position kernels place the boxes from the trajectories and know nothing of the edit")
        spec, cand = actors
        _, hit = actor_encode(spec, cand, o, d, a, starts, ends, enc, ray_flip)  # rows spliced in place
    y, hidden = mlp_fwd(enc, fs.geo_w, fs.geo_b, save_hidden=True)
    cot = torch.zeros_like(y)
    cot[:, 0] = 1.0
    g_enc, _, _ = mlp_bwd(enc, hidden, cot, fs.geo_w, fs.geo_b)
    if hit is None or not bool((hit >= 0).any()):
        g, _ = encode_bwd_rays(fs.grid, fs.table, fs.static_scale, o1, d1, a1, s1, e1, g_enc)
    else:
        inside = hit >= 0
        g, _ = encode_bwd_rays(fs.grid, fs.table, fs.static_scale, o1, d1, a1, s1, e1,
                               torch.where(inside[:, None], torch.zeros_like(g_enc), g_enc))
        idx = inside.nonzero()[:, 0]           # the winners' pairs, in sample order
        act = hit[idx].contiguous()
        t1 = per(_chk(times.reshape(-1), "times"))
        f1 = None if ray_flip is None else per(_chk(ray_flip.reshape(-1), "ray_flip"))
        x01, cstd = actor_pair_positions(spec, o1, d1, a1, s1, e1, t1, idx, act, f1)
        ag_, La, F = spec.grid, spec.grid.num_levels, spec.grid.features_per_level
        raw = hashgrid_multi_fwd(ag_, spec.tables, act, x01).view(-1, La, F)
        sc = ag_.scalings.to(x01.device)[None, :]
        a2 = sc * 2 * cstd[:, None]
        w = 1 / a2.clamp_min(1.0)                                  # the rescale weight and its derivative in cstd,
        ge = g_enc[idx, : La * F].view(-1, La, F)                  # which clamp_min passes at equality
        g_cstd = -((ge * raw).sum(-1) * torch.where(a2 >= 1, 2 * sc * w * w, torch.zeros_like(w))).sum(-1)
        g_x01 = hashgrid_multi_bwd_input(ag_, spec.tables, act, x01, (ge * w[..., None]).reshape(-1, La * F).contiguous())
        g_act = actor_pair_positions_bwd(spec, o1, d1, a1, s1, e1, t1, idx, act, f1, g_x01, g_cstd.contiguous(),
                                         ray_grads=True)[2]
        g = torch.where(inside[:, None], g_act, g)
    out = {}
    if "hit" in want:
        out["hit"] = hit.view(R, S)
    if "geo" in want:
        out["geo"] = y[:, 0].reshape(R, S)
    if "gradient" in want:
        out["gradient"] = g.reshape(R, S, 3)
    if "normals" in want or "ray_normals" in want:
        nrm = g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        nrm = (nrm if fs.use_sdf else -nrm).reshape(R, S, 3)
        if "normals" in want:
            out["normals"] = nrm
        if "ray_normals" in want:
            w = _chk(weights, "weights").reshape(R, S, 1)
            out["ray_normals"] = torch.where(w != 0, w * nrm, torch.zeros_like(nrm)).sum(1)
    return out


def _packed_ray_of(who: str, r, ray_indices: Tensor) -> Tensor:
    """the march's ray_indices for the packed descriptor ``r``: int64 [M], one per sample"""
    ri = _chk(ray_indices.reshape(-1), "ray_indices", torch.int64)
    if ri.shape[0] != r.n_samples:
        raise ValueError(f"{who}: ray_indices has {ri.shape[0]} entries, expected one per sample ({r.n_samples})")
    return ri


def actor_find_packed(spec: "ActorSpec", cand, origins, directions, pixel_area, t_starts, t_ends, ray_indices,
                      ray_flip: Optional[Tensor] = None):
    """``actor_hits`` and the geometry of ``actor_encode`` on packed samples, in one pass and without feature rows: cand = one
    candidate list per RAY, ray_indices int64 [M] names each sample's ray, ray_flip [R] +-1 or None.
    -> (hits [M,8] int32, hit [M] int32: the winning actor or -1, directions [M,3]: box frame where hit, else the ray's)"""
    r, keep = _c_packed_rays("actor_find_packed", origins, directions, pixel_area, t_starts, t_ends)
    a, keep2 = spec.c_actors()
    ri = _packed_ray_of("actor_find_packed", r, ray_indices)
    R, m, dev = r.n_rays, r.n_samples, keep[0].device
    cnt, act, w2b = _c_ray_candidates("actor_find_packed", cand, R, a.max_candidates)
    flip = _opt(ray_flip, "ray_flip")
    if flip is not None and flip.shape[0] != R:
        raise ValueError(f"actor_find_packed: ray_flip is per ray, [R = {R}]")
    hits = torch.empty((m, _lib.MAX_SAMPLE_CONTAINMENTS), dtype=torch.int32, device=dev)
    hit = torch.empty((m,), dtype=torch.int32, device=dev)
    dirs = torch.empty((m, 3), dtype=torch.float32, device=dev)
    launch("nrhip_actor_find_packed", a, r, ri, cnt, act, w2b, hits, hit, dirs, flip)
    return hits, hit, dirs


def _packed_pair_args(who: str, spec: "ActorSpec", origins, directions, pixel_area, t_starts, t_ends, ray_indices, times,
                      sample_idx, actor_idx, ray_flip):
    r, keep = _c_packed_rays(who, origins, directions, pixel_area, t_starts, t_ends)
    a, keep2 = spec.c_actors()
    ri = _packed_ray_of(who, r, ray_indices)
    si, ai = _chk(sample_idx, "sample_idx", torch.int64), _chk(actor_idx, "actor_idx", torch.int32)
    t, flip = _chk(times.reshape(-1), "times"), _opt(ray_flip, "ray_flip")
    if t.shape[0] != r.n_rays or (flip is not None and flip.shape[0] != r.n_rays) or ai.shape != si.shape:
        raise ValueError(f"{who}: times / ray_flip are per ray ([R = {r.n_rays}]), sample_idx / actor_idx [P]")
    return a, r, ri, t, si, ai, flip


def actor_pair_positions_packed(spec: "ActorSpec", origins, directions, pixel_area, t_starts, t_ends, ray_indices, times,
                                sample_idx: Tensor, actor_idx: Tensor, ray_flip: Optional[Tensor] = None):
    """``actor_pair_positions`` on packed samples: sample_idx [P] int64 is a packed sample index, ray_indices int64 [M] names
    each sample's ray, times / ray_flip are per ray.  -> (x01 [P,3], cstd [P])"""
    a, r, ri, t, si, ai, flip = _packed_pair_args("actor_pair_positions_packed", spec, origins, directions, pixel_area,
                                                  t_starts, t_ends, ray_indices, times, sample_idx, actor_idx, ray_flip)
    P_ = si.shape[0]
    x01 = torch.empty((P_, 3), dtype=torch.float32, device=si.device)
    cstd = torch.empty((P_,), dtype=torch.float32, device=si.device)
    launch("nrhip_actor_pair_positions_fwd_packed", a, r, ri, t, si, ai, flip, P_, x01, cstd)
    return x01, cstd


def actor_pair_positions_packed_bwd(spec: "ActorSpec", origins, directions, pixel_area, t_starts, t_ends, ray_indices, times,
                                    sample_idx, actor_idx, ray_flip, grad_x01: Tensor, grad_cstd: Tensor):
    """-> (grad actor_positions [Tn,A,3], grad actor_rotations_6d [Tn,A,6]), accumulated with atomics as
    ``actor_pair_positions_bwd``; the rays' gradient is ``actor_pair_positions_packed_bwd_rays``"""
    a, r, ri, t, si, ai, flip = _packed_pair_args("actor_pair_positions_packed_bwd", spec, origins, directions, pixel_area,
                                                  t_starts, t_ends, ray_indices, times, sample_idx, actor_idx, ray_flip)
    flat = torch.zeros((a.n_times * a.n_actors * 9,), dtype=torch.float32, device=si.device)
    gp = flat[: a.n_times * a.n_actors * 3].view(a.n_times, a.n_actors, 3)
    gr = flat[a.n_times * a.n_actors * 3:].view(a.n_times, a.n_actors, 6)
    launch("nrhip_actor_pair_positions_bwd_packed", a, r, ri, t, si, ai, flip, si.shape[0], _chk(grad_x01, "grad_x01"),
           _chk(grad_cstd, "grad_cstd"), gp, gr)
    return gp, gr


def actor_pair_positions_packed_bwd_rays(spec: "ActorSpec", origins, directions, pixel_area, t_starts, t_ends, segments, times,
                                         sample_idx, actor_idx, ray_flip, grad_x01: Tensor, grad_cstd: Tensor,
                                         lanes_per_ray: int = 0) -> Tuple[Tensor, Tensor]:
    """The ray share of ``actor_pair_positions_bwd(..., ray_grads=True)`` on packed samples: -> (dL/d origins, dL/d
    directions) [R,3] of the in-box samples.  segments int64 [R+1] bounds each ray's samples; sample_idx [P] int64 is a packed
    sample index and NON-DECREASING (``actor_pairs``' order), times / ray_flip are per ray.  One kernel, a group of lanes per
    ray over the ray's range of the pair list, no atomics: bit-reproducible, a ray's rows depend on its own pairs and the
    group size only; zeros for a ray without pairs.  lanes_per_ray: 16 / 32 / 64 forces the group size, 0 lets the library
    choose it from the mean count P / R."""
    who = "actor_pair_positions_packed_bwd_rays"
    r, keep = _c_packed_rays(who, origins, directions, pixel_area, t_starts, t_ends, segments)
    a, keep2 = spec.c_actors()
    si, ai = _chk(sample_idx, "sample_idx", torch.int64), _chk(actor_idx, "actor_idx", torch.int32)
    t, flip = _chk(times.reshape(-1), "times"), _opt(ray_flip, "ray_flip")
    if t.shape[0] != r.n_rays or (flip is not None and flip.shape[0] != r.n_rays) or ai.shape != si.shape or si.dim() != 1:
        raise ValueError(f"{who}: times / ray_flip are per ray ([R = {r.n_rays}]), sample_idx / actor_idx [P]")
    P_ = si.shape[0]
    gx, gc = _chk(grad_x01, "grad_x01"), _chk(grad_cstd, "grad_cstd")
    if gx.numel() != 3 * P_ or gc.numel() != P_:
        raise ValueError(f"{who}: grad_x01 [P,3] and grad_cstd [P] with P = {P_}")
    out = torch.empty((2, r.n_rays, 3), device=keep[0].device, dtype=torch.float32)
    launch("nrhip_actor_pair_positions_bwd_rays_packed", a, r, t, si, ai, flip, P_, gx, gc, int(lanes_per_ray), out[0], out[1])
    return out[0], out[1]


def sdf_render_packed_fwd(geo_out, beta: Optional[Tensor], beta_min: float, features, t_starts, t_ends, segments):
    """Head + packed compositing.  geo_out [M], beta = the raw learnable parameter (device, 1 element; None: the density
    head, sigma = trunc_exp(geo_out)), features [M,C] -> alpha [M], weights [M], features [R,C], depth [R,1], acc [R,1]"""
    x = _flat(geo_out, "geo_out")
    M = x.shape[0]
    s, e = _flat(t_starts, "t_starts", M), _flat(t_ends, "t_ends", M)
    f = _chk(features, "features")
    if f.dim() != 2 or f.shape[0] != M or f.shape[1] < 1:
        raise ValueError("features must be [M,C] with one row per sample")
    b = _opt(beta, "beta")
    if b is not None and b.numel() != 1:
        raise ValueError("sdf_render_packed_fwd: beta must have one element")
    seg, R = _seg(segments)
    Cc = f.shape[1]
    mk = lambda *shape: torch.empty(shape, device=x.device, dtype=torch.float32)  # noqa: E731
    alpha, w, of, od, oa = torch.empty_like(x), torch.empty_like(x), mk(R, Cc), mk(R, 1), mk(R, 1)
    launch("nrhip_sdf_render_packed_fwd", x, b, float(beta_min), f, s, e, seg, R, Cc, alpha, w, of, od, oa)
    return alpha, w, of, od, oa


def sdf_render_packed_bwd(geo_out, beta: Optional[Tensor], beta_min: float, alpha, features, t_starts, t_ends, segments,
                          g_features=None, g_depth=None, g_accumulation=None, g_weights=None):
    """-> grad_features [M,C], grad_geo_out [M], grad_beta [1] (None for the density head).  Each upstream may be None."""
    x = _flat(geo_out, "geo_out")
    M = x.shape[0]
    al, s, e = _flat(alpha, "alpha", M), _flat(t_starts, "t_starts", M), _flat(t_ends, "t_ends", M)
    f = _chk(features, "features")
    if f.dim() != 2 or f.shape[0] != M or f.shape[1] < 1:
        raise ValueError("features must be [M,C] with one row per sample")
    b = _opt(beta, "beta")
    seg, R = _seg(segments)
    Cc = f.shape[1]
    gF = None
    if g_features is not None:
        gF = _chk(g_features, "g_features")
        if gF.shape != (R, Cc):
            raise ValueError(f"g_features must be [{R},{Cc}]")
    gd = None if g_depth is None else _flat(g_depth, "g_depth", R)
    ga = None if g_accumulation is None else _flat(g_accumulation, "g_accumulation", R)
    gw = None if g_weights is None else _flat(g_weights, "g_weights", M)
    gf = torch.empty_like(f) if gF is not None else torch.zeros_like(f)  # (no upstream on the features: not written)
    gx = torch.empty_like(x)
    gbeta = None if b is None else torch.empty((1,), device=x.device, dtype=torch.float32)
    ws, _ = _workspace("nrhip_sdf_render_packed_bwd_workspace", R, device=x.device, dtype=torch.float32)
    launch("nrhip_sdf_render_packed_bwd", x, b, float(beta_min), al, f, s, e, seg, gF, gd, ga, gw, R, Cc, gf, gx, gbeta, ws)
    return gf, gx, gbeta


def packed_ray_indices(segments: Tensor, n_samples: int) -> Tensor:
    """segments int64 [R+1] -> the ray of every sample, int64 [M]; on the device, no host read"""
    seg, R = _seg(segments)
    i = torch.arange(int(n_samples), device=seg.device, dtype=torch.int64)
    return torch.searchsorted(seg[1:], i, right=True)


def encode_bwd_packed(spec: GridSpec, static_scale: float, origins, directions, pixel_area, t_starts, t_ends, ray_indices,
                      grad_out, out_dtype=torch.float32):
    """``encode_bwd`` for packed samples: ray_indices int64 [M] names each sample's ray.  -> grad table [L*T, F], in fp16
    where the partition writes an fp16-storage table's gradient itself (as ``encode_bwd``).  Below ``_BINNED_MIN_SAMPLES``,
    or for a table the partition cannot slice, the ray constants are gathered per sample for the atomic entry point."""
    ri = _chk(ray_indices.reshape(-1), "ray_indices", torch.int64)
    n = ri.shape[0]
    grad_out = _chk(grad_out, "grad_out")

    def binned(sfx, g, *tail):
        r, keep = _c_packed_rays("encode_bwd_packed", origins, directions, pixel_area, t_starts, t_ends)
        if r.n_samples != n:
            raise ValueError(f"t_starts: {r.n_samples} samples, expected {n}")
        launch("nrhip_encode_bwd_binned_packed" + sfx, g, float(static_scale), r, ri, grad_out, *tail)

    def atomic():  # on [M,1] rays
        o, d, a = _ray_constants(origins, directions, pixel_area)
        return encode_bwd(spec, static_scale, o[ri], d[ri], a[ri], _flat(t_starts, "t_starts", n).reshape(n, 1),
                          _flat(t_ends, "t_ends", n).reshape(n, 1), grad_out, out_dtype)

    return _table_grad(spec, n, grad_out.device, out_dtype, binned, atomic)


def encode_bwd_rays_packed(spec: GridSpec, table: Tensor, static_scale: float, origins, directions, pixel_area, t_starts,
                           t_ends, segments, grad_out, lanes_per_ray: int = 0) -> Tuple[Tensor, Tensor]:
    """``encode_bwd_rays`` for the march's packed samples: dL/d(origins), dL/d(directions) [R,3] from dL/d(rescaled
    features) [M, L*F] at the packed sample index.  One kernel, a group of lanes per ray over its segment, no atomics:
    bit-reproducible, a ray's rows depend on its own samples and the group size only; zeros for a ray without samples.
    lanes_per_ray: 16 / 32 / 64 forces the group size, 0 lets the library choose it from the mean count M / R."""
    if grad_out.numel() != t_starts.numel() * spec.out_dim:  # (shapes only: answered before any device is asked for)
        raise ValueError(f"grad_out has {grad_out.numel()} elements, expected {t_starts.numel() * spec.out_dim}")
    r, keep = _c_packed_rays("encode_bwd_rays_packed", origins, directions, pixel_area, t_starts, t_ends, segments)
    grad_out = _chk(grad_out, "grad_out")
    g = spec.c_grid(table)
    out = torch.empty((2, r.n_rays, 3), device=keep[0].device, dtype=torch.float32)
    launch("nrhip_encode_bwd_rays_packed", g, _chk(table, "table", table.dtype), float(static_scale), r, grad_out,
           int(lanes_per_ray), out[0], out[1])
    return out[0], out[1]


def packed_composite_bwd(t_starts, t_ends, sigmas_or_alphas, features, segments, density_mode: bool, g_features,
                         g_depth=None, g_accumulation=None, g_weights=None, need_grad_x=True, need_grad_features=True):
    """-> (grad sigmas / alphas [M] or None, grad features [M,C] or None)"""
    x = _flat(sigmas_or_alphas, "sigmas" if density_mode else "alphas")
    M = x.shape[0]
    s, e = _flat(t_starts, "t_starts", M), _flat(t_ends, "t_ends", M)
    f = _chk(features, "features")
    seg, R = _seg(segments)
    Cc = f.shape[1]
    gF = _chk(g_features, "g_features")
    if gF.shape != (R, Cc):
        raise ValueError(f"g_features must be [{R},{Cc}]")
    gd = None if g_depth is None else _flat(g_depth, "g_depth", R)
    ga = None if g_accumulation is None else _flat(g_accumulation, "g_accumulation", R)
    gw = None if g_weights is None else _flat(g_weights, "g_weights", M)
    gx = torch.empty_like(x) if need_grad_x else None
    gf = torch.empty_like(f) if need_grad_features else None
    launch("nrhip_packed_composite_bwd", s, e, x, f, seg, gF, gd, ga, gw, R, Cc, 1 if density_mode else 0, gx, gf)
    return gx, gf


def adam_step(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step: int, lr: float, beta1: float = 0.9,
              beta2: float = 0.999, eps: float = 1e-15, weight_decay: float = 0.0, grad_scale: float = 1.0) -> None:
    """torch.optim.Adam / AdamW update of one fp32 tensor, in place (csrc/adam.hip)"""
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if _chk(t, n).data_ptr() != t.data_ptr() or t.shape != param.shape:
            raise ValueError(f"adam_step: {n} must be a contiguous fp32 GPU tensor of the parameter's shape")
    launch("nrhip_adam_step", param, grad, exp_avg, exp_avg_sq, param.numel(), int(step), float(lr), float(beta1),
           float(beta2), float(eps), float(weight_decay), float(grad_scale))


def _adam_item(a, who: str, param: Tensor, grad: Tensor, m: Tensor, v: Tensor, image: Optional[Tensor]) -> None:
    """check one item of ``who`` and fill what nrhip_adam_tensor and nrhip_adam_tensor_dev share (all but ``step``)"""
    for t, n in ((param, "param"), (m, "exp_avg"), (v, "exp_avg_sq")):
        if _chk(t, n).data_ptr() != t.data_ptr() or t.shape != param.shape:
            raise ValueError(f"{who}: {n} must be a contiguous fp32 GPU tensor of the parameter's shape")
    if grad.dtype not in (torch.float32, torch.float16) or not grad.is_contiguous() or not grad.is_cuda or grad.shape != param.shape:
        raise ValueError(f"{who}: grad must be a contiguous fp32 / fp16 GPU tensor of the parameter's shape")
    if image is not None and (image.dtype != torch.float16 or not image.is_contiguous() or image.shape != param.shape):
        raise ValueError(f"{who}: image must be a contiguous fp16 tensor of the parameter's shape")
    a.param, a.grad, a.exp_avg, a.exp_avg_sq = param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr()
    a.image_fp16 = image.data_ptr() if image is not None else None
    a.n, a.grad_dtype = param.numel(), 1 if grad.dtype == torch.float16 else 0


def _f32_scalar(t, what: str) -> Tensor:
    if not (isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
        raise ValueError(f"{what} must be an fp32 GPU scalar")
    return t


def adam_step_many(items, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-15, weight_decay: float = 0.0,
                   grad_scale: float = 1.0) -> None:
    """torch.optim.Adam / AdamW update of MANY tensors in one launch per 24 (csrc/adam.hip).  items: (param fp32, grad fp32 |
    fp16, exp_avg, exp_avg_sq, step, image | None) -- ``image``: the fp16 table whose fp32 master copy ``param`` is; it
    receives the rounded new values in the same pass."""
    items = list(items)
    if not items:
        return
    arr = (_lib.AdamTensor * len(items))()
    for k, (param, grad, m, v, step, image) in enumerate(items):
        _adam_item(arr[k], "adam_step_many", param, grad, m, v, image)
        arr[k].step = int(step)
    launch("nrhip_adam_step_many", arr, len(items), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
           float(grad_scale))


_ADAM_CTL_BYTES = None


def adam_workspace_floats(n_tensors: int) -> int:
    """size of adam_step_many_dev's workspace for ``n_tensors`` tensors, in fp32 elements"""
    global _ADAM_CTL_BYTES
    if _ADAM_CTL_BYTES is None:
        nb = C.c_int64()
        call("nrhip_adam_step_many_workspace", 1, C.byref(nb))
        _ADAM_CTL_BYTES = int(nb.value)
    return (_ADAM_CTL_BYTES * max(int(n_tensors), 1) + 3) // 4


def adam_workspace(n_tensors: int, device) -> Tensor:
    """device workspace of adam_step_many_dev for up to ``n_tensors`` tensors (the caller keeps it across steps)"""
    return torch.empty((adam_workspace_floats(n_tensors),), device=device, dtype=torch.float32)


def adam_step_many_dev(items, lr, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-15, weight_decay: float = 0.0,
                       grad_scale: Optional[Tensor] = None, found_inf: Optional[Tensor] = None,
                       workspace: Optional[Tensor] = None, host_grad_scale: float = 1.0) -> None:
    """adam_step_many with everything a step decides ON THE DEVICE (csrc/adam.hip: GradScaler's protocol, graph capture).
    items: (param fp32, grad fp32 | fp16, exp_avg, exp_avg_sq, step = fp32 device scalar holding the count BEFORE this
    update, image | None).  lr: float, or an fp32 device scalar.  grad_scale / found_inf: fp32 device scalars (the
    GradScaler's scale and its found-inf flag): gradients are divided by the scale; a non-zero flag leaves parameters, moments
    and step counts untouched.  No host read."""
    items = list(items)
    if not items:
        return
    dev = items[0][0].device
    arr = (_lib.AdamTensorDev * len(items))()
    for k, (param, grad, m, v, step, image) in enumerate(items):
        _adam_item(arr[k], "adam_step_many_dev", param, grad, m, v, image)
        arr[k].step = _f32_scalar(step, "adam_step_many_dev: step").data_ptr()
    scalar = lambda t, what: None if t is None else _f32_scalar(t, f"adam_step_many_dev: {what}")  # noqa: E731
    lr_dev = scalar(lr, "lr") if isinstance(lr, Tensor) else None
    if workspace is None:
        workspace = adam_workspace(len(items), dev)
    if workspace.numel() < adam_workspace_floats(len(items)) or not workspace.is_cuda or workspace.dtype != torch.float32:
        raise ValueError("adam_step_many_dev: workspace too small (ops.adam_workspace)")
    launch("nrhip_adam_step_many_dev", arr, len(items), 0.0 if lr_dev is not None else float(lr), lr_dev, float(beta1),
           float(beta2), float(eps), float(weight_decay), float(host_grad_scale), scalar(grad_scale, "grad_scale"),
           scalar(found_inf, "found_inf"), workspace)


def nonfinite_check(tensors, found_inf: Tensor) -> Tensor:
    """GradScaler's inf check, read-only (csrc/adam.hip: nonfinite_check_kernel): ``found_inf`` (fp32 GPU scalar) becomes 1
    when any element of any of ``tensors`` (contiguous fp32 / fp16 GPU tensors, 16-byte aligned) is inf or NaN; it is never
    cleared here.  Same flag semantics as ``torch._amp_foreach_non_finite_check_and_unscale_`` at a scale of 1, without the
    write-back."""
    tensors = [t for t in tensors if t.numel()]
    _f32_scalar(found_inf, "nonfinite_check: found_inf")
    if not tensors:
        return found_inf
    arr = (_lib.CheckTensor * len(tensors))()
    for k, t in enumerate(tensors):
        if (not t.is_cuda or t.dtype not in (torch.float32, torch.float16) or not t.is_contiguous() or t.data_ptr() % 16
                or t.device != found_inf.device):
            raise ValueError("nonfinite_check: tensors must be contiguous, 16-byte aligned fp32 / fp16 tensors on found_inf's GPU")
        arr[k].data, arr[k].n, arr[k].dtype = t.data_ptr(), t.numel(), 1 if t.dtype == torch.float16 else 0
    launch("nrhip_nonfinite_check_many", arr, len(tensors), found_inf)
    return found_inf


def reload_tuning() -> None:
    """the library reads its NRHIP_* A/B switches once at load; call this after changing one inside a running process"""
    call("nrhip_tuning_reload")


def device_info():
    cus, xcds, hbm = C.c_int32(), C.c_int32(), C.c_int64()
    call("nrhip_device_info", C.byref(cus), C.byref(xcds), C.byref(hbm))
    return {"cus": cus.value, "xcds": xcds.value, "hbm_bytes": hbm.value}


# ------------------------------------------------------------------------------------------------
# losses on the sampler outputs
def interlevel_loss_level(c: Tensor, w: Tensor, cp: Tensor, wp: Tensor, pulse_width: float, need_grad: bool = True):
    """one proposal level of zipnerf_interlevel_loss: -> loss_per_ray [R], d loss_per_ray / d wp [R,Sp] (or None)"""
    c, w, cp, wp = _chk(c, "c"), _chk(w, "w"), _chk(cp, "cp"), _chk(wp, "wp")
    R, sf, sp = w.shape[0], w.shape[1], wp.shape[1]
    if c.shape != (R, sf + 1) or cp.shape != (R, sp + 1) or wp.shape[0] != R:
        raise ValueError(f"interlevel_loss: shapes c {tuple(c.shape)} w {tuple(w.shape)} cp {tuple(cp.shape)} wp {tuple(wp.shape)}")
    loss = torch.empty((R,), device=w.device, dtype=torch.float32)
    g = torch.empty_like(wp) if need_grad else None
    launch("nrhip_interlevel_loss", c, w, sf, cp, wp, sp, float(pulse_width), R, loss, g)
    return loss, g


def distortion_loss_rays(c: Tensor, w: Tensor, need_grad: bool = True):
    """lossfun_distortion per ray: -> loss_per_ray [R], d loss_per_ray / d w [R,S] (or None)"""
    c, w = _chk(c, "c"), _chk(w, "w")
    R, s = w.shape
    if c.shape != (R, s + 1):
        raise ValueError(f"distortion_loss: c {tuple(c.shape)} does not match w {tuple(w.shape)}")
    loss = torch.empty((R,), device=w.device, dtype=torch.float32)
    g = torch.empty_like(w) if need_grad else None
    launch("nrhip_distortion_loss", c, w, s, R, loss, g)
    return loss, g


# ------------------------------------------------------------------------------------------------
# The training step's glue as kernels (csrc/train_fused.hip): bin EDGES [R,S+1] in, no [R,S,1] views
def _edges(e: Tensor, S: int, name: str = "edges"):
    if not (isinstance(e, Tensor) and e.is_cuda and e.dtype == torch.float32 and e.dim() == 2):
        raise _lib.NeuradHipError(f"{name}: expected a 2-D float32 GPU tensor")
    if e.shape[1] < S + 1:
        raise ValueError(f"{name}: {tuple(e.shape)} holds fewer than S+1 = {S + 1} edges per ray")
    if e.stride(1) != 1:
        e = e.contiguous()
    return e, (e.stride(0) if e.shape[0] > 1 else e.shape[1])


def prop_weights_fwd(edges: Tensor, densities: Tensor, want_depth: bool = True):
    """RaySamples.get_weights + render_depth_simple of one proposal round -> (weights [R,S], depth [R,1] or None)"""
    dens = _chk(densities, "densities")
    R, S = dens.shape
    e, es = _edges(edges, S)
    w = torch.empty_like(dens)
    depth = torch.empty((R, 1), device=dens.device, dtype=torch.float32) if want_depth else None
    launch("nrhip_prop_weights_fwd", e, es, dens, R, S, w, depth)
    return w, depth


def prop_weights_bwd(edges: Tensor, densities: Tensor, grad_w: Optional[Tensor], grad_depth: Optional[Tensor]) -> Tensor:
    dens = _chk(densities, "densities")
    R, S = dens.shape
    e, es = _edges(edges, S)
    gw = None if grad_w is None else _chk(grad_w, "grad_w")
    gd = _opt(grad_depth, "grad_depth")
    gdens = torch.empty_like(dens)
    launch("nrhip_prop_weights_bwd", e, es, dens, gw, gd, R, S, gdens)
    return gdens


def sdf_render_fwd(sdf: Tensor, beta: Tensor, beta_min: float, features: Tensor, edges: Tensor, extra_cols: int = 0):
    """SDF head + weights + compositing.  sdf [R,S], beta = the raw learnable parameter (device, 1 element), features
    [R,S,C], edges [R,S+1] (last edge = sky distance).  -> alpha [R,S], weights_ns [R,S-1], out [R,C+extra_cols] (the
    first C columns written), depth [R,1], acc [R,1].  beta = None: the density head (use_sdf = False) -- ``sdf`` is the
    raw geometry output x, sigma = trunc_exp(x), alpha = 1 - exp(-sigma (end - start)) (render_weight_from_density)."""
    sdf, feat = _chk(sdf, "sdf"), _chk(features, "features")
    b = _opt(beta, "beta")
    R, S = sdf.shape
    C_ = feat.shape[-1]
    if feat.numel() != R * S * C_ or (b is not None and b.numel() != 1):
        raise ValueError("sdf_render_fwd: features must be [R,S,C], beta one element")
    e, es = _edges(edges, S)
    dev = sdf.device
    alpha = torch.empty_like(sdf)
    w_ns = torch.empty((R, S - 1), device=dev, dtype=torch.float32)
    out = torch.empty((R, C_ + extra_cols), device=dev, dtype=torch.float32)
    depth = torch.empty((R, 1), device=dev, dtype=torch.float32)
    acc = torch.empty((R, 1), device=dev, dtype=torch.float32)
    launch("nrhip_sdf_render_fwd", sdf, b, float(beta_min), feat, e, es, R, S, C_, alpha, w_ns, out, C_ + extra_cols, depth,
           acc)
    return alpha, w_ns, out, depth, acc


def _strided_rows(t: Tensor, name: str):
    """[R, C] float32 GPU view with unit inner stride -> (tensor, row stride); copies only when it has to"""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
        raise _lib.NeuradHipError(f"{name}: expected a 2-D float32 GPU tensor")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def sdf_render_bwd(sdf, beta, beta_min, alpha, features, edges, g_out: Tensor, g_depth: Optional[Tensor],
                   g_acc: Optional[Tensor], g_weights_ns: Optional[Tensor]):
    """-> grad_features [R,S,C], grad_sdf [R,S], grad_beta [1] (None for the density head, beta = None).  g_out: [R,C] view
    (row stride free) of the gradient of the composited features."""
    sdf, feat, alpha = _chk(sdf, "sdf"), _chk(features, "features"), _chk(alpha, "alpha")
    b = _opt(beta, "beta")
    R, S = sdf.shape
    C_ = feat.shape[-1]
    e, es = _edges(edges, S)
    g, gs = _strided_rows(g_out, "g_out")
    if g.shape != (R, C_):
        raise ValueError(f"sdf_render_bwd: g_out {tuple(g.shape)} != {(R, C_)}")
    if g.data_ptr() % 16 or (gs * 4) % 16:
        g, gs = g.contiguous(), C_
    gd = _opt(g_depth, "g_depth")
    ga = _opt(g_acc, "g_acc")
    gw = None if g_weights_ns is None else _chk(g_weights_ns.reshape(R, S - 1), "g_weights_ns")
    dev = sdf.device
    gfeat = torch.empty_like(feat)
    gsdf = torch.empty_like(sdf)
    gbeta = None if b is None else torch.empty((1,), device=dev, dtype=torch.float32)
    ws, _ = _workspace("nrhip_sdf_render_bwd_workspace", R, device=dev, dtype=torch.float32)
    launch("nrhip_sdf_render_bwd", sdf, b, float(beta_min), alpha, feat, e, es, g, gs, gd, ga, gw, R, S, C_, gfeat, gsdf,
           gbeta, ws)
    return gfeat, gsdf, gbeta


def appearance_fwd(weight: Tensor, sensor_idx: Optional[Tensor], times: Optional[Tensor], duration: float,
                   n_per_sensor: int, temporal: bool, n_rays: int, out: Optional[Tensor] = None) -> Tensor:
    """appearance embedding rows (models/neurad.py:423-441) written into ``out`` ([R,D] view, row stride free)"""
    w = _chk(weight, "weight")
    E, D = w.shape
    s = _opt(sensor_idx, "sensor_idx", torch.int64)
    t = _opt(times, "times")
    if out is None:
        out = torch.empty((n_rays, D), device=w.device, dtype=torch.float32)
    if not (out.is_cuda and out.dtype == torch.float32 and out.shape == (n_rays, D) and out.stride(1) == 1):
        raise ValueError("appearance_fwd: out must be a float32 [R,D] GPU view with unit inner stride")
    launch("nrhip_appearance_fwd", w, s, t, float(duration), int(n_per_sensor), 1 if temporal else 0, n_rays, E, D, out,
           out.stride(0) if n_rays > 1 else D)
    return out


def appearance_bwd(g_out: Tensor, sensor_idx, times, duration: float, n_per_sensor: int, temporal: bool,
                   n_embed: int) -> Tensor:
    g, gs = _strided_rows(g_out, "g_out")
    R, D = g.shape
    s = _opt(sensor_idx, "sensor_idx", torch.int64)
    t = _opt(times, "times")
    gw = torch.empty((n_embed, D), device=g.device, dtype=torch.float32)  # the entry point zero-fills it
    launch("nrhip_appearance_bwd", g, gs, s, t, float(duration), int(n_per_sensor), 1 if temporal else 0, R, n_embed, D, gw)
    return gw


def mask_compact(mask: Tensor, n_out: int):
    """rows (int64 [n_out], ascending) where ``mask`` [R] is set + inverse (int32 [R]: slot or -1), without the host sync of
    ``mask.nonzero()`` -- the caller knows n_out (the lidar part of a batch comes with the batch)"""
    m = mask.reshape(-1)
    if not m.is_cuda:
        raise _lib.NeuradHipError("mask_compact: mask is on the CPU (no CPU fallback)")
    m = (m if m.dtype == torch.uint8 else (m.contiguous().view(torch.uint8) if m.dtype == torch.bool else m.ne(0).view(torch.uint8)))
    m = m.contiguous()
    # n_out is the caller's word for mask.sum(); should it be too large, the rows past the real count stay 0 (a valid
    # gather index) instead of uninitialised memory
    rows = torch.zeros((n_out,), device=m.device, dtype=torch.int64)
    inverse = torch.empty((m.shape[0],), device=m.device, dtype=torch.int32)
    launch("nrhip_mask_compact", m, m.shape[0], rows, n_out, inverse, None)
    return rows, inverse


def lidar_losses(depths: Sequence[Tensor], lidar_rows: Tensor, distance: Tensor, did_return: Tensor, intensity: Tensor,
                 intensity_target: Tensor, ray_drop_logits: Tensor, non_return_distance: float, non_return_mult: float,
                 quantile: float):
    """-> metrics [2 + n_levels] (depth_loss, intensity_loss, ray_drop_loss, depth_loss_0, ...), and what the backward
    needs (per-ray gradients, scratch with the errors / threshold / counts, did_return as uint8)"""
    nl = len(depths)
    ds = [_chk(d.reshape(-1), f"depth[{i}]") for i, d in enumerate(depths)]
    rows = _chk(lidar_rows, "lidar_rows", torch.int64)
    n = rows.shape[0]
    dist, inten = _chk(distance.reshape(-1), "distance"), _chk(intensity.reshape(-1), "intensity")
    tgt, lg = _chk(intensity_target.reshape(-1), "intensity_target"), _chk(ray_drop_logits.reshape(-1), "ray_drop_logits")
    ret = did_return.reshape(-1).contiguous()
    ret = ret.view(torch.uint8) if ret.dtype == torch.bool else ret.to(torch.uint8)
    for v, nm in ((dist, "distance"), (inten, "intensity"), (tgt, "intensity_target"), (lg, "ray_drop_logits"), (ret, "did_return")):
        if v.shape[0] != n:
            raise ValueError(f"lidar_losses: {nm} has {v.shape[0]} rows, expected {n}")
    dev = rows.device
    metrics = torch.empty((2 + nl,), device=dev, dtype=torch.float32)
    unit = torch.empty((nl + 2, n), device=dev, dtype=torch.float32)
    scratch, _ = _workspace("nrhip_lidar_losses_workspace", n, device=dev, dtype=torch.float32)
    launch("nrhip_lidar_losses", _host_ptrs(ds), nl, rows, dist, ret, inten, tgt, lg, n, float(non_return_distance),
           float(non_return_mult), float(quantile), metrics, unit, scratch)
    return metrics, (unit, scratch, ret)


def lidar_losses_bwd(saved, inverse: Tensor, upstream: Tensor, n_levels: int, n_rays: int, need_depth: Sequence[bool],
                     need_intensity: bool = True, need_logits: bool = True):
    """saved = what lidar_losses returned beside the metrics.  -> ([grad depth [R,1] or None per level], grad intensity
    [n,1] or None, grad logits [n,1] or None)"""
    unit, scratch, ret = saved
    unit, inv, up = _chk(unit, "unit"), _chk(inverse, "inverse", torch.int32), _chk(upstream.reshape(-1), "upstream")
    n, dev = unit.shape[1], unit.device
    gds = [torch.empty((n_rays, 1), device=dev, dtype=torch.float32) if nd else None for nd in need_depth]
    gi = torch.empty((n, 1), device=dev, dtype=torch.float32) if need_intensity else None
    gl = torch.empty((n, 1), device=dev, dtype=torch.float32) if need_logits else None
    launch("nrhip_lidar_losses_bwd", unit, scratch, ret, inv, up, n_levels, n_rays, n, _host_ptrs(gds, n_levels), gi, gl)
    return gds, gi, gl


# ---- lidar scan evaluation (csrc/lidar_eval.hip): nearest neighbour and chamfer distance, no autograd -------------------------
NEAREST_TILE = _lib.NEAREST_TILE
NEAREST_QS = (1, 2, 4)  # query points per lane the kernel is instantiated for


def _points(t: Tensor, name: str) -> Tuple[Tensor, int]:
    """a point set [n, >= 3] fp32 -> (the tensor, its row stride in floats): a strided view of rows goes in as it is
    (``scan[:, :3]`` of an [N,5] scan, homogeneous [N,4] points); anything else is made contiguous"""
    if not isinstance(t, Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise _lib.NeuradHipError(f"{name}: tensor is on {t.device}; the HIP path needs a GPU tensor (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError(f"{name}: expected [n, >= 3], got {tuple(t.shape)}")
    if t.shape[0] >= 2 ** 31:
        raise _lib.NeuradHipError(f"{name}: {t.shape[0]} points >= 2^31")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < 3):
        t = t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), 3))


def _valid(v: Optional[Tensor], n: int, name: str) -> Optional[Tensor]:
    if v is None:
        return None
    v = v.reshape(-1)
    if not v.is_cuda:
        raise _lib.NeuradHipError(f"{name}: tensor is on {v.device}; the HIP path needs a GPU tensor (no CPU fallback)")
    if v.shape[0] != n:
        raise ValueError(f"{name}: {v.shape[0]} entries for {n} points")
    v = v.contiguous()
    return v.view(torch.uint8) if v.dtype == torch.bool else _chk(v, name, torch.uint8)


def _nearest_plan_arg(plan) -> int:
    """None -> 0 (the library chooses from N and M); (Q, split) -> Q | split << 8"""
    if plan is None:
        return 0
    q, split = plan
    if int(q) not in NEAREST_QS or not 1 <= int(split) <= 64:
        raise ValueError(f"plan=(Q, split): Q in {NEAREST_QS}, split in [1, 64]; got {plan}")
    return int(q) | int(split) << 8


def nearest_plan(n: int, m: int) -> Tuple[int, int]:
    """(Q, split) the library picks for n queries against m targets (host logic)"""
    q, split = C.c_int32(0), C.c_int32(0)
    call("nrhip_nearest_plan", int(n), int(m), C.byref(q), C.byref(split))
    return q.value, split.value


def nearest_sq_dist(query: Tensor, target: Tensor, query_valid: Optional[Tensor] = None,
                    target_valid: Optional[Tensor] = None, plan=None) -> Tensor:
    """-> [N] fp32: for every query the squared distance to its nearest valid target (direct differences; +inf without a
    valid target, 0 for an invalid query).  query / target [*, >= 3] fp32, strided rows allowed; *_valid bool / uint8 [*].
    plan=(Q, split) forces the launch plan; every plan gives the same bits."""
    q, sq = _points(query, "query")
    t, st = _points(target, "target")
    n, m = q.shape[0], t.shape[0]
    qv, tv = _valid(query_valid, n, "query_valid"), _valid(target_valid, m, "target_valid")
    out = torch.empty((n,), device=q.device, dtype=torch.float32)
    launch("nrhip_nearest_sq_dist", q if n else None, sq, qv if n else None, n, t if m else None, st, tv if m else None, m,
           _nearest_plan_arg(plan), out if n else None)
    return out


def chamfer_distance(source: Tensor, target: Tensor, source_valid: Optional[Tensor] = None,
                     target_valid: Optional[Tensor] = None, normalize_with_target: bool = False,
                     return_per_point: bool = False, plan=None):
    """utils/math.py:745-798 on masked point sets -> 0-dim fp32 tensor on the device (no host read): the sum over the valid
    sources of their nearest squared distance to the valid targets, plus the same the other way round, divided by the number
    of valid targets when ``normalize_with_target``.  return_per_point: -> (value, source_sq_dist [N], target_sq_dist [M])."""
    s, ss = _points(source, "source")
    t, st = _points(target, "target")
    n, m = s.shape[0], t.shape[0]
    sv, tv = _valid(source_valid, n, "source_valid"), _valid(target_valid, m, "target_valid")
    dev = s.device
    result = torch.empty((), device=dev, dtype=torch.float32)
    ds = torch.empty((n,), device=dev, dtype=torch.float32) if return_per_point else None
    dt = torch.empty((m,), device=dev, dtype=torch.float32) if return_per_point else None
    ws, need = _workspace("nrhip_chamfer_workspace", n, m, device=dev, dtype=torch.uint8)
    launch("nrhip_chamfer_distance", s if n else None, ss, sv if n else None, n, t if m else None, st, tv if m else None, m,
           1 if normalize_with_target else 0, _nearest_plan_arg(plan), result, ds if n else None, dt if m else None, ws, need)
    return (result, ds, dt) if return_per_point else result


# ---- camera image evaluation (csrc/image_eval.hip): PSNR and SSIM, no autograd ------------------------------------------------
SSIM_TILE = _lib.SSIM_TILE
SSIM_WINDOW = 11
IMAGE_STAT_ITEMS = _lib.IMAGE_STAT_ITEMS


def _image(t: Tensor, name: str) -> Tensor:
    """[H,W,C] or [1,C,H,W] (the view the reference's moveaxis makes of an [H,W,C] image costs no copy on the way back)
    -> contiguous channel-last fp32 [H,W,C] on the device"""
    if not isinstance(t, Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise _lib.NeuradHipError(f"{name}: tensor is on {t.device}; the HIP path needs a GPU tensor (no CPU fallback)")
    if t.dim() == 4:
        if t.shape[0] != 1:
            raise ValueError(f"{name}: one image per call, got a batch of {t.shape[0]}")
        t = t[0].permute(1, 2, 0)
    if t.dim() != 3 or t.shape[2] not in (1, 3):
        raise ValueError(f"{name}: expected [H,W,C] or [1,C,H,W] with C in (1, 3), got {tuple(t.shape)}")
    return t.detach().float().contiguous()


def image_metrics(a: Tensor, b: Tensor, psnr_range: float = 1.0, return_map: bool = False):
    """-> (psnr, ssim[, ssim_map [H-10, W-10, C]]): 0-dim fp32 tensors on the device, no host read.  torchmetrics'
    PeakSignalNoiseRatio(data_range=psnr_range) and structural_similarity_index_measure with its defaults (11 x 11 Gaussian
    window, sigma 1.5, data range from the two images) as include/neurad_hip.h states them."""
    a, b = _image(a, "a"), _image(b, "b")
    if a.shape != b.shape:
        raise ValueError(f"image shapes differ: {tuple(a.shape)} and {tuple(b.shape)}")
    h, w, c = a.shape
    if h < SSIM_WINDOW or w < SSIM_WINDOW:
        raise ValueError(f"image {h} x {w} is smaller than the {SSIM_WINDOW} x {SSIM_WINDOW} SSIM window")
    out = torch.empty((2,), device=a.device, dtype=torch.float32)
    ssim_map = torch.empty((h - SSIM_WINDOW + 1, w - SSIM_WINDOW + 1, c), device=a.device, dtype=torch.float32) \
        if return_map else None
    ws, need = _workspace("nrhip_image_metrics_workspace", h, w, c, device=a.device, dtype=torch.uint8)
    launch("nrhip_image_metrics", a, b, h, w, c, float(psnr_range), ssim_map, ws, need, out)
    return (out[0], out[1], ssim_map) if return_map else (out[0], out[1])


def image_psnr(a: Tensor, b: Tensor, psnr_range: float = 1.0) -> Tensor:
    """PSNR over all elements of two equally shaped tensors -> 0-dim fp32 tensor on the device, no host read (the training
    step's metric, models/neurad.py:465)"""
    a, b = _chk(a.detach().float().reshape(-1), "a"), _chk(b.detach().float().reshape(-1), "b")
    if a.shape != b.shape or a.shape[0] == 0:
        raise ValueError(f"image_psnr: {a.shape[0]} and {b.shape[0]} elements")
    n = a.shape[0]
    ws = torch.empty(((n + IMAGE_STAT_ITEMS - 1) // IMAGE_STAT_ITEMS,), device=a.device, dtype=torch.float64)
    out = torch.empty((1,), device=a.device, dtype=torch.float32)
    launch("nrhip_image_psnr", a, b, n, float(psnr_range), ws, out)
    return out[0]


# ---- camera pose correction (csrc/pose_opt.hip): the SO3xR3 camera optimizer's apply_to_raybundle and its gradient -------------
def _pose_args(pose: Tensor, weights: Optional[Tensor], camera_indices: Tensor):
    pose = _chk(pose, "pose")
    if pose.dim() != 2 or pose.shape[1] != 6:
        raise ValueError(f"pose: expected [num_cameras, 6], got {tuple(pose.shape)}")
    weights = _opt(weights, "weights")
    if weights is not None and weights.shape[0] != 6:
        raise ValueError(f"weights: expected [6], got {tuple(weights.shape)}")
    return pose, weights, _chk(camera_indices.reshape(-1), "camera_indices", torch.int64)


def _rays3(t: Tensor, name: str, r: int) -> Tensor:
    t = _chk(t, name)
    if t.dim() != 2 or tuple(t.shape) != (r, 3):
        raise ValueError(f"{name}: expected [{r}, 3], got {tuple(t.shape)}")
    return t


def pose_apply(pose: Tensor, weights: Optional[Tensor], camera_indices: Tensor, origins: Tensor, directions: Tensor):
    """-> (origins + t, R directions), fp32 [R, 3]: the exponential map of SO(3) x R^3 of ``pose[camera_indices] * weights`` per
    ray, as include/neurad_hip.h states it.  pose [C, 6] fp32, weights [6] fp32 or None, camera_indices int64 [R] inside
    [0, C) (a ray outside comes back unchanged).  One launch, no autograd (autograd.PoseApplyFn)."""
    pose, weights, idx = _pose_args(pose, weights, camera_indices)
    r = idx.shape[0]
    origins, directions = _rays3(origins, "origins", r), _rays3(directions, "directions", r)
    if r == 0 or pose.shape[0] == 0:
        return origins.clone(), directions.clone()
    out_o, out_d = torch.empty_like(origins), torch.empty_like(directions)
    launch("nrhip_pose_apply", pose, weights, pose.shape[0], idx, origins, directions, r, out_o, out_d)
    return out_o, out_d


def pose_apply_bwd(pose: Tensor, weights: Optional[Tensor], camera_indices: Tensor, directions: Tensor, grad_origins: Tensor,
                   grad_directions: Tensor, need_grad_origins: bool = False, need_grad_directions: bool = False):
    """-> (grad_pose [C, 6] dense fp32, grad_in_origins or None, grad_in_directions or None).  Per-camera integer sums: the same
    bits for every order of the rays, no float atomics, no host read; a camera with a non-finite ray gradient gets a NaN row,
    a camera without a ray exact zeros (include/neurad_hip.h)."""
    pose, weights, idx = _pose_args(pose, weights, camera_indices)
    r, c = idx.shape[0], pose.shape[0]
    directions = _rays3(directions, "directions", r)
    grad_origins, grad_directions = _rays3(grad_origins, "grad_origins", r), _rays3(grad_directions, "grad_directions", r)
    gi_o = torch.empty_like(grad_origins) if need_grad_origins else None
    gi_d = torch.empty_like(grad_directions) if need_grad_directions else None
    if r == 0 or c == 0:
        return torch.zeros_like(pose), gi_o, gi_d
    grad_pose = torch.empty_like(pose)
    ws, _ = _workspace("nrhip_pose_apply_bwd_workspace", r, c, device=pose.device, dtype=torch.uint8)
    launch("nrhip_pose_apply_bwd", pose, weights, c, idx, directions, grad_origins, grad_directions, r, ws, grad_pose, gi_o, gi_d)
    return grad_pose, gi_o, gi_d


# ---- the level-sparse gradient exchange's device side (csrc/grad_rows.hip; parallel/data_parallel.py) ----------
def grad_rows_count(grad: Tensor, n_levels: int):
    """grad [n_levels * T, F] fp32 -> (level_counts [n_levels] int64 = non-zero rows per level, block_offsets [n_levels, nblk]
    uint32 as int32 storage: the per-block exclusive prefix ``grad_rows_compact`` needs)"""
    g = _chk(grad, "grad")
    T, F = g.shape[0] // n_levels, g.shape[1]
    nblk = (T + _lib.GRAD_ROWS_PER_BLOCK - 1) // _lib.GRAD_ROWS_PER_BLOCK
    blocks = torch.empty((n_levels, nblk), dtype=torch.int32, device=g.device)
    counts = torch.empty((n_levels,), dtype=torch.int64, device=g.device)
    launch("nrhip_grad_rows_count", g, n_levels, T, F, blocks, counts)
    return counts, blocks


_MAX_LIST_LEVELS = 32  # kMaxListLevels of csrc/grad_rows.hip


def _list_args(levels: Sequence[int], caps: Sequence[int]):
    n = len(levels)
    return (C.c_int32 * n)(*levels), (C.c_int64 * n)(*caps), n


def grad_rows_compact(grad: Tensor, n_levels: int, block_offsets: Tensor, levels: Sequence[int], caps: Sequence[int],
                      scale: float = 1.0):
    """the levels ``levels`` of grad as ordered (row, values) lists, level i padded to caps[i] entries with row -1 / zeros
    -> (rows [sum caps] int32, vals [sum caps, F] fp32 = grad * scale)"""
    g = _chk(grad, "grad")
    T, F = g.shape[0] // n_levels, g.shape[1]
    total = int(sum(caps))
    rows = torch.full((total,), -1, dtype=torch.int32, device=g.device)
    vals = torch.zeros((total, F), dtype=torch.float32, device=g.device)
    bo = _chk(block_offsets, "block_offsets", torch.int32)
    off = 0
    for k in range(0, len(levels), _MAX_LIST_LEVELS):  # the kernel takes at most 32 list levels per launch
        lvk, cpk = list(levels[k:k + _MAX_LIST_LEVELS]), list(caps[k:k + _MAX_LIST_LEVELS])
        tk = int(sum(cpk))
        if tk:
            lv, cp, n = _list_args(lvk, cpk)
            launch("nrhip_grad_rows_compact", g, n_levels, T, F, bo, lv, cp, n, float(scale), rows[off:], vals[off:])
        off += tk
    return rows, vals


def grad_rows_apply(grad: Tensor, n_levels: int, levels: Sequence[int], caps: Sequence[int], rows: Tensor,
                    vals: Optional[Tensor], add: bool) -> None:
    """in place on grad: rows of the list -> 0 (add=False) or += vals (add=True); entries with row -1 are padding"""
    if not grad.is_contiguous():
        raise ValueError("grad_rows_apply: contiguous gradient only (it is updated in place)")
    g = _chk(grad, "grad")
    T, F = g.shape[0] // n_levels, g.shape[1]
    if int(sum(caps)) == 0:
        return
    rows = _chk(rows, "rows", torch.int32)
    vals = None if vals is None else _chk(vals, "vals")
    off = 0
    for k in range(0, len(levels), _MAX_LIST_LEVELS):
        lvk, cpk = list(levels[k:k + _MAX_LIST_LEVELS]), list(caps[k:k + _MAX_LIST_LEVELS])
        tk = int(sum(cpk))
        if tk:
            lv, cp, n = _list_args(lvk, cpk)
            launch("nrhip_grad_rows_apply", g, n_levels, T, F, lv, cp, n, rows[off:], None if vals is None else vals[off:],
                   1 if add else 0)
        off += tk
