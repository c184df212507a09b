"""Sizes, input builders and numpy models for the tests of the single-workgroup scans and the chunk carries: rows_scan_kernel
(csrc/grad_rows.hip), actor_pairs_scan_kernel (csrc/actors.hip), compact_scan_kernel / mean_final_kernel
(csrc/occgrid_update.h) and packed_visibility_kernel (csrc/occgrid.hip) -- TEST INFRASTRUCTURE ONLY.

Each of these kernels has a branch that runs only above a size threshold: a carry across passes of 1024 blocks, more than one
block per scan thread, a strided loop over more than 256 partial sums, a carry into a ray's second 64-sample chunk.  The
sizes here are the smallest that enter each branch; the models restate each scan once as written and once with that branch
broken, so that tests/test_scan_refs_host.py can show -- without a GPU -- that the inputs tell the two apart at the new sizes
and could not at the sizes the suite had before."""
import functools

import numpy as np

import occgrid_update_restatement as UR

f32, f64 = np.float32, np.float64


def exclusive_cumsum(c):
    c = np.asarray(c, np.int64)
    return np.concatenate([[0], np.cumsum(c)[:-1]]) if len(c) else c


def block_counts(flags, per_block):
    """flags bool [n] -> set flags per block of ``per_block`` (the last block may be ragged)"""
    flags = np.asarray(flags).reshape(-1)
    pad = -len(flags) % per_block
    return np.concatenate([flags, np.zeros(pad, flags.dtype)]).reshape(-1, per_block).sum(1).astype(np.int64)


# ---- rows_scan_kernel: passes of 1024 blocks with a carry ----------------------------------------------------------------
GRAD_ROWS_PER_BLOCK, GRAD_SCAN_WIDTH = 256, 1024
GRAD_T_OLD = 4096                      # nblk = 16: the largest the suite reached
GRAD_T_NEW = (262144, 262145, 262657)  # nblk = 1024, 1025, 1027: one full pass, a second pass of one block, a ragged one


def grad_nblk(T):
    return -(-T // GRAD_ROWS_PER_BLOCK)


def sparse_grad(T, F, seed, L=2):
    """fp32 [L, T, F].  The share of non-zero rows differs between the two levels and between the rows of the first pass
    (the first 1024 blocks) and the rest; each of the last three blocks and row T - 1 hold a non-zero row."""
    rng = np.random.default_rng(seed)
    first = GRAD_SCAN_WIDTH * GRAD_ROWS_PER_BLOCK
    share = np.empty((L, T))
    for l in range(L):
        share[l, :first], share[l, first:] = ((0.02, 0.6), (0.3, 0.05))[l % 2]
    nz = rng.random((L, T)) < share
    for b in range(max(grad_nblk(T) - 3, 0), grad_nblk(T)):
        nz[:, b * GRAD_ROWS_PER_BLOCK] = True
    nz[:, T - 1] = True
    v = rng.standard_normal((L, T, F)).astype(f32)
    v[v == 0] = 1.0
    keep = rng.random((L, T, F)) < 0.7  # a non-zero row may hold zeros, but never only zeros
    keep[..., rng.integers(0, F)] = True
    return np.where(keep & nz[..., None], v, f32(0))


def rows_scan_model(counts, carry=True):
    """rows_scan_kernel on one level's block counts -> exclusive offsets (uint32 arithmetic); carry=False drops the running
    total between the passes of 1024 blocks"""
    counts = np.asarray(counts, np.int64)
    out, run = np.zeros_like(counts), 0
    for b0 in range(0, len(counts), GRAD_SCAN_WIDTH):
        c = counts[b0:b0 + GRAD_SCAN_WIDTH]
        out[b0:b0 + GRAD_SCAN_WIDTH] = run + exclusive_cumsum(c)
        run = run + int(c.sum()) if carry else 0
    return out & 0xFFFFFFFF


# ---- actor_pairs_scan_kernel: 1024 threads, per = ceil(nblk / 1024) blocks each ------------------------------------------
PAIR_BLOCK, PAIR_SCAN_THREADS, HIT_SLOTS = 1024, 1024, 8
PAIRS_N_OLD = 70001                        # nblk = 69
PAIRS_N_NEW = (1048576, 1049600, 1049601)  # nblk = 1024 (per = 1, every thread busy), 1025 and 1026 (per = 2, idle threads)


def pairs_nblk(n):
    return -(-n // PAIR_BLOCK)


def empty_block_run(n):
    """[first, last) of the 1024-sample blocks that hits_table leaves without a hit"""
    nblk = pairs_nblk(n)
    return nblk // 2 - max(2, nblk // 25), nblk // 2


def hits_table(n, seed):
    """int32 [n, 8] in nrhip_actor_hits' layout (ascending actors compacted to the front, -1 behind), built without a loop
    over rows.  12 % of the rows of the first half hold 1-3 hits, 2 % of the second; a run of whole 1024-sample blocks just
    before the middle holds none; row n - 1 is full."""
    rng = np.random.default_rng(seed)
    hits = np.full((n, HIT_SLOTS), -1, np.int32)
    hit = rng.random(n) < np.where(np.arange(n) < n // 2, 0.12, 0.02)
    b0, b1 = empty_block_run(n)
    hit[b0 * PAIR_BLOCK:b1 * PAIR_BLOCK] = False
    rows = np.flatnonzero(hit)
    actors = np.sort(np.argsort(rng.random((len(rows), 32)), axis=1)[:, :3], axis=1).astype(np.int32)  # 3 distinct of 32
    k = rng.integers(1, 4, len(rows))
    hits[rows, :3] = np.where(np.arange(3)[None] < k[:, None], actors, -1)
    hits[n - 1] = np.arange(HIT_SLOTS)
    return hits


def chunked_scan_model(counts, threads, per=None):
    """The scan shared by actor_pairs_scan_kernel (threads = 1024) and compact_scan_kernel (threads = 256), in place on the
    block counts: thread t owns blocks [t per, t per + per), per = ceil(n / threads).  -> (offsets, total).  A forced
    ``per`` (the broken variant) leaves the blocks no thread owns holding their counts, and out of the total."""
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    per = -(-n // threads) if per is None else per
    owned = min(n, threads * per)
    pad = np.zeros(threads * per, np.int64)
    pad[:owned] = counts[:owned]
    part = pad.reshape(threads, per).sum(1)
    start = exclusive_cumsum(part)
    within = np.cumsum(pad.reshape(threads, per), 1) - pad.reshape(threads, per)
    out = counts.copy()
    out[:owned] = (start[:, None] + within).reshape(-1)[:owned]
    return out, int(part.sum())


pairs_scan_model = functools.partial(chunked_scan_model, threads=PAIR_SCAN_THREADS)


# ---- compact_scan_kernel and mean_final_kernel ----------------------------------------------------------------------------
COMPACT_ITEMS, SUM_ITEMS, OCC_SCAN_THREADS = 1024, 2048, 256
OCC_RES_OLD, OCC_RES_NEW = 32, 65  # n_blk = 32 (per = 1) and 269 (per = 2, a ragged last block, idle scan threads)

compact_scan_model = functools.partial(chunked_scan_model, threads=OCC_SCAN_THREADS)


def occ_sizes(res, L):
    """(cells, n_blk, n_part) of csrc/occgrid_update.h's scratch layout"""
    cells = res ** 3
    return cells, -(-cells // COMPACT_ITEMS), -(-L * cells // SUM_ITEMS)


def grid_state(res, L, seed, p_invisible=0.2, p_occupied=0.5):
    """random occs fp32 [L res^3] (-1 = invisible) and binaries bool [L, res, res, res]; p_occupied per level or one for all"""
    rng = np.random.default_rng(seed)
    occs = rng.random(L * res ** 3).astype(f32)
    occs[rng.random(occs.shape) < p_invisible] = -1.0
    binaries = rng.random((L, res, res, res)) < np.reshape(p_occupied, (-1, 1, 1, 1))
    return occs, binaries


CANDIDATE_CASES = {"warmup_with_invisible": 0.5, "few_occupied": 0.1, "many_occupied": 0.6, "two_levels": [0.6, 0.1]}


def candidates_case(case, res):
    """the inputs of one candidates case and the restatement's answer -> dict(L, warmup, occs, binaries, draws, n, cap, ids,
    counts, n_occ)"""
    L, warmup = (2 if case == "two_levels" else 1), case == "warmup_with_invisible"
    occs, binaries = grid_state(res, L, 11, p_occupied=CANDIDATE_CASES[case])
    d = UR.draws(res, L, warmup, 12)
    n, cap = UR.capacity(res, warmup)
    ids, counts = UR.candidates(occs, binaries, res, L, warmup, None, d["cell_draws"], d["sel_draws"])
    n_occ = (binaries.reshape(L, -1) & (occs.reshape(L, -1) >= 0)).sum(1)
    return dict(L=L, warmup=warmup, occs=occs, binaries=binaries, draws=d, n=n, cap=cap, ids=ids, counts=counts, n_occ=n_occ)


EMA_DECAY = 0.95
EMA_OCC_THRE = {"mean_above_occ_thre": 0.03, "mean_below_occ_thre": 0.5}


def ema_case(res, L, seed):
    """Injected candidates over the whole grid -> dict(occs, ids, counts, vals).  Capacity res^3 per level, cells drawn with
    replacement (duplicates; about a third of the cells untouched), 20 % of the cells invisible, the last 1000 slots of
    level 1 behind its count.  Every value is a multiple of 2^-10: k / 1024 with k <= 40, except in the cells behind the
    first 256 blocks of the visible-sum pass (256 * 2048 cells), which hold k in [900, 1000].  A mean over the first 256
    partial sums alone therefore falls far below the true one."""
    rng = np.random.default_rng(seed)
    cells = res ** 3
    head = OCC_SCAN_THREADS * SUM_ITEMS
    occs = (rng.integers(0, 41, L * cells) / 1024.0).astype(f32)
    occs[rng.random(L * cells) < 0.2] = -1.0
    ids = rng.integers(0, cells, (L, cells)).astype(np.int32)
    counts = np.full(L, cells, np.int32)
    counts[-1] -= 1000
    glob = np.arange(L)[:, None] * cells + ids
    vals = (np.where(glob < head, rng.integers(0, 41, (L, cells)), rng.integers(900, 1001, (L, cells))) / 1024.0).astype(f32)
    return dict(occs=occs, ids=ids, counts=counts, vals=vals)


def visible_partials(occs):
    """ema_apply_sum_kernel's per-block float64 sums and counts of the visible cells (blocks of 2048 cells)"""
    occs = np.asarray(occs, f32).reshape(-1)
    pad = -len(occs) % SUM_ITEMS
    o = np.concatenate([occs, np.full(pad, -1, f32)]).reshape(-1, SUM_ITEMS)
    vis = o >= 0
    return np.where(vis, o, 0).astype(f64).sum(1), vis.sum(1).astype(np.int64)


def mean_final_model(psum, pcnt, occ_thre, strided=True):
    """mean_final_kernel -> (thre fp32, mean float64): thread t adds the partials t, t + 256, ...; then the fixed-order block
    sum (a shuffle-down tree per wave, the four waves left to right).  strided=False stops after the first 256 partials."""
    psum, pcnt = np.asarray(psum, f64), np.asarray(pcnt, np.int64)
    if not strided:
        psum, pcnt = psum[:OCC_SCAN_THREADS], pcnt[:OCC_SCAN_THREADS]
    pad = -len(psum) % OCC_SCAN_THREADS
    s = np.concatenate([psum, np.zeros(pad)]).reshape(-1, OCC_SCAN_THREADS)
    acc = np.zeros(OCC_SCAN_THREADS)
    for row in s:  # in order: s += psum[i] for i = t, t + 256, ...
        acc = acc + row
    acc = acc.reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, np.where(lane + off < 64, lane + off, lane)]
    bs, bn = ((acc[0, 0] + acc[1, 0]) + acc[2, 0]) + acc[3, 0], int(pcnt.sum())
    if bn == 0:
        return f32(np.inf), np.nan
    return min(f32(bs / bn), f32(occ_thre)), bs / bn


@functools.lru_cache(maxsize=None)
def shell_run_default(occ_thre):
    """UR.shell_run at OccGridEstimator's default resolution, one level: n_blk = 2048 (per = 8), n_part = 1024"""
    return list(UR.shell_run(occ_thre, res=128, levels=1))


# ---- packed_visibility_kernel: 64-sample chunks with a carried transmittance ---------------------------------------------
CHUNK = 64
VIS_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 191, 0, 300, 700, 512, 0)  # 13 rays: a ragged last workgroup, empty rays anywhere
VIS_EXACT_EPS = 2.0 ** -20
# Per ray: the first sample whose transmittance lies below eps (None: never), and whether the sample before it sees
# T == eps exactly.  65 -> chunk 1 is zero-filled one chunk after the stop, 129 -> two, 300 -> four; 128 crosses at 65 with
# the carry out of chunk 0 EQUAL to eps (no stop yet); 191 crosses inside chunk 2, its ragged last; 700 inside chunk 10, its
# ragged last; 512 reaches T == eps in chunk 3 and stays there.
VIS_EXACT_CROSS = (None, None, 30, 63, 64, 65, 64, 150, None, 20, 670, None, None)
VIS_EXACT_TOUCH = (False, False, True, False, True, True, True, True, False, False, True, True, False)
VIS_ALPHA_THRES = (0.0, 0.5, 0.6)


def vis_segments(lengths=VIS_LENGTHS):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def vis_exact_alphas(seed=0):
    """fp32 alphas with 1 - alpha in {1, 1/2, 1/4}: every transmittance is a power of two.  A ray that touches eps collects
    exactly 20 halvings (12 halves and 4 quarters) before sample c - 1, which then halves again; the others collect 19
    (13 and 3) and sample c - 1 quarters: 2^-19 -> 2^-21.  The halvings are spread over all the samples before c - 1, so
    every chunk before the crossing contributes to the carry.  Behind the crossing the alphas are random."""
    rng = np.random.default_rng(seed)
    out = []
    for n, c, touch in zip(VIS_LENGTHS, VIS_EXACT_CROSS, VIS_EXACT_TOUCH):
        h = np.zeros(n, np.int64)
        if touch or c is not None:
            stop = c - 1 if c is not None else n // 2  # (never crossing: 20 halvings in the first half, none behind)
            at = np.sort(rng.choice(stop, 16, replace=False))
            h[at] = 1
            h[rng.choice(at, 4 if touch else 3, replace=False)] = 2
        if c is not None:
            h[c - 1] = 1 if touch else 2
            h[c:] = rng.integers(0, 3, n - c)
        out.append(1.0 - 0.5 ** h)
    return np.concatenate(out).astype(f32)


def vis_generic_alphas(seed=3):
    return (np.random.default_rng(seed).random(int(sum(VIS_LENGTHS)), dtype=f32) * f32(0.05)).astype(f32)


VIS_GENERIC_EPS, VIS_GENERIC_ALPHA_THRE, VIS_BAND, VIS_MAX_LEFT_OUT = 1e-3, 0.02, 1e-4, 0.005


def transmittance64(alphas, seg):
    """float64 T_i = prod_{j < i} (1 - alpha_j) within each ray's segment, from the fp32 alphas"""
    T = np.ones(len(alphas), f64)
    for b, e in zip(seg[:-1], seg[1:]):
        if e > b:
            T[b:e] = np.concatenate([[1.0], np.cumprod(1.0 - alphas[b:e].astype(f64))[:-1]])
    return T


def visibility64(alphas, seg, eps, alpha_thre):
    """-> (mask, T): keep sample i iff T_i >= eps and alpha_i >= alpha_thre, both thresholds as the fp32 numbers the kernel
    receives"""
    T = transmittance64(alphas, seg)
    return (T >= f64(f32(eps))) & (alphas >= f32(alpha_thre)), T


def first_below(T, seg, eps):
    """per ray: the first local sample index with T < eps, or None"""
    out = []
    for b, e in zip(seg[:-1], seg[1:]):
        k = np.flatnonzero(T[b:e] < eps)
        out.append(int(k[0]) if len(k) else None)
    return tuple(out)


def visibility_model(alphas, seg, eps, alpha_thre, carry=True):
    """packed_visibility_kernel in fp32, chunk by chunk (the product within a chunk taken left to right); carry=False starts
    every chunk from T = 1"""
    alphas = np.asarray(alphas, f32)
    mask = np.zeros(len(alphas), bool)
    for b, e in zip(seg[:-1], seg[1:]):
        run = f32(1)
        for i0 in range(b, e, CHUNK):
            a = alphas[i0:min(i0 + CHUNK, e)]
            incl = np.cumprod(f32(1) - a, dtype=f32)
            T = run * np.concatenate([[f32(1)], incl[:-1]]).astype(f32)
            mask[i0:i0 + len(a)] = (T >= f32(eps)) & (a >= f32(alpha_thre))
            run = f32(run * incl[-1]) if carry else f32(1)
            if len(a) == CHUNK and run < f32(eps):
                break  # the rest of the ray stays 0
    return mask
