"""tests/mlp_refs.py on the CPU: the int64 reference against the oracle, the conditions that make bit equality a fair
demand on every case of tests/test_gpu_mlp_exact.py, and the restated launch plans at the values that module relies on."""
import numpy as np
import pytest

import mlp_refs as MR
import neurad_oracle as O

CASES = MR.gpu_cases()
FEATURE = [(h, n) for h in (32, 64) for n in MR.FEATURE_NS]


def _id(v):
    d, n, kw = v
    return "-".join(map(str, d)) + f"_n{n}"


@pytest.mark.parametrize("spec", CASES, ids=_id)
def test_reference_agrees_with_the_oracle_and_the_case_is_exact_and_informative(spec):
    dims, n, kw = spec
    c = MR.case(dims, n, **kw)
    MR.assert_exact_operands(c)
    MR.assert_informative(c)
    ws = [w.numpy() for w in c["weights"]]
    bs = [None if b is None else b.numpy() for b in c["biases"]]
    y, acts = O.mlp_fwd(c["x"].numpy(), ws, bs, return_hidden=True)
    assert np.array_equal(y, c["y"])
    if c["nl"] > 1:
        assert np.array_equal(np.concatenate(acts[1:-1], 1), c["hidden"])
    gx, dws, dbs = O.mlp_bwd(acts, ws, c["grad_y"].numpy())
    assert np.array_equal(gx, c["grad_x"])
    for l in range(c["nl"]):
        assert np.array_equal(dws[l], c["dW"][l]) and np.array_equal(dbs[l], c["db"][l]), l
    # the mask is z > 0 on the integers, and every dZ follows from it
    g = c["grad_y"].numpy().astype(np.int64)
    for l in reversed(range(c["nl"])):
        if l < c["nl"] - 1:
            g = np.where(c["z"][l] > 0, g, 0)
        assert np.array_equal(g, c["dz"][l]), l
        g = g @ c["W"][l] if n <= 2000 else MR.imatmul(g, c["W"][l])


@pytest.mark.parametrize("h,n", FEATURE)
def test_feature_head_cases(h, n):
    c = MR.feature_case(h, n)
    MR.assert_exact_operands(c)
    MR.assert_informative(c)
    assert c["dims"] == (48, h, h, 32) and all(b is not None for b in c["biases"])
    col0, gf = c["grad_geo0"].numpy().astype(np.int64), c["grad_y"].numpy().astype(np.int64)
    assert np.array_equal(c["grad_geo"][:, 0], col0)
    assert np.array_equal(c["grad_geo"][:, 1:] - gf, c["grad_x"][:, :32])
    ws = [w.numpy() for w in c["weights"]]
    _, acts = O.mlp_fwd(c["x"].numpy(), ws, [b.numpy() for b in c["biases"]], return_hidden=True)
    gx, dws, dbs = O.mlp_bwd(acts, ws, c["grad_y"].numpy())
    assert np.array_equal(gx, c["grad_x"])
    for l in range(3):
        assert np.array_equal(dws[l], c["dW"][l]) and np.array_equal(dbs[l], c["db"][l])


def test_large_products_equal_the_plain_int64_product_on_sampled_rows():
    rng = np.random.RandomState(3)
    a, b = rng.randint(-50, 51, size=(70001, 64)), rng.randint(-1, 2, size=(64, 48))
    assert a.shape[0] * a.shape[1] * b.shape[1] > 1 << 24  # the float64 route
    rows = np.r_[0:64, rng.randint(0, 70001, size=193), 70001 - 64:70001]
    assert np.array_equal(MR.imatmul(a, b)[rows], a[rows].astype(np.int64) @ b.astype(np.int64))
    assert MR.imatmul(a, b).dtype == np.int64


def test_grad_y_has_its_zero_rows_and_hidden_layers_their_zero_unit():
    c = MR.case((48, 64, 64, 32), 1000)
    gy = c["grad_y"].numpy()
    assert not gy[32:64].any() and not gy[4::5].any() and not gy[-3:].any() and gy[:4].any() and gy[64:].any()
    assert MR.zero_rows(1).sum() == 0 and MR.zero_rows(15).tolist() == [r in (4, 9, 14) for r in range(15)]
    for l in range(2):
        k0 = (3 + 5 * l) % 64
        assert not c["z"][l][:, k0].any() and c["W"][l + 1][:, k0].any()  # masked, though a gradient arrives at it
    sums = MR.largest_sums(MR.case((64, 64, 64, 32), 70001))
    assert max(sums.values()) < 2 ** 21  # ample room below 2^24


def test_assert_equal_names_the_first_differing_element():
    import torch

    want = np.arange(12).reshape(3, 4)
    got = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    MR.assert_equal(got, want, "same")
    got[1, 2] = MR.SENTINEL
    with pytest.raises(AssertionError, match=r"1 of 12 elements differ; first at row 1, column 2: got -98765.25, want 6"):
        MR.assert_equal(got, want, "one off")
    got[1, 2] = float("nan")
    with pytest.raises(AssertionError, match="row 1, column 2"):
        MR.assert_equal(got, want, "nan")


def test_conditions_reject_what_they_should():
    c = dict(MR.case((5, 7, 3), 17), _cache={})
    c["dz"] = [d * 2 ** 22 for d in c["dz"]]
    with pytest.raises(AssertionError, match="2\\^24"):
        MR.assert_exact_operands(c)
    c = dict(MR.case((5, 7, 3), 17))
    c["z"] = [np.abs(z) + 1 for z in c["z"]]
    with pytest.raises(AssertionError, match="live"):
        MR.assert_informative(c)


# ---- the restated plans ----------------------------------------------------------------------------------------------------
def test_fused_masks():
    full = {(32, 32, 33): 4 + 6, (32, 64, 33): 20, (48, 32, 32, 32): 14, (64, 32, 32, 32): 16}  # accumulator tiles
    for dims in MR.CHAINED:
        nl = len(dims) - 1
        if dims in full:
            assert MR.wg_mask(dims) == (1 << nl) - 1
            nb, ib, ob = dims[1] // 16, dims[0] // 16, -(-dims[-1] // 16)
            assert nb * ib + (nb * nb if nl == 3 else 0) + ob * nb == full[dims] <= 24
        else:
            assert dims in ((48, 64, 64, 32), (64, 64, 64, 32)) and MR.wg_mask(dims) == 0b110  # layers 1 and 2
        masks = ((1 << nl) - 1, ((1 << nl) - 1) & ~1, 0)
        assert len({MR.nslot(dims, m) for m in masks}) == 3 and MR.nslot(dims, 0) == 0  # NSLOT tells the mask
        for n in (1, 17, 70001):
            dz = (n * (nl - 1) * dims[1] + 3) & ~3
            assert MR.mask_from_workspace(dims, n, dz + MR.part_floats(dims) * 1024) == MR.wg_mask(dims)
    assert MR.wg_mask((64, 128, 128, 32)) == 0  # 8 x 8 + 2 x 8 tiles: no layer fits (not a chained shape: the rule alone)
    # NSLOT by hand, 32 -> 32 -> 33: 10 accumulators x 4 floats, 2 x 4 bias slots of layer 0, 48 / 4 grad_y columns
    assert MR.nslot((32, 32, 33)) == 40 + 8 + 12 and MR.part_floats((32, 32, 33)) == 60 * 64
    # 48 -> 64 -> 64 -> 32, layers 1 and 2: (16 + 8) x 4, 4 x 4 bias slots of layer 1, 32 / 4 columns
    assert MR.nslot((48, 64, 64, 32)) == 96 + 16 + 8


def test_lds_plans():
    for dims, _ in MR.GENERIC + ((MR.SINGLE, {}), (MR.FWD_CAPPED[0], {}), (MR.WGRAD_CAPPED[0], {})):
        waves = 2 if dims == MR.WGRAD_RAGGED else 4  # 83,712 B of weights and slabs of 162 floats a row: 166,656 B with 4
        assert MR.pick_waves(dims) == MR.pick_waves(dims, True) == waves, dims
    for dims in MR.CHAINED:
        assert MR.pick_waves(dims) == 4  # under NRHIP_MLP_GENERIC
    for tr in (False, True):
        assert MR.pick_waves(MR.TWO_WAVES, tr) == 2 and MR.pick_waves(MR.ONE_WAVE, tr) == 1 and MR.pick_waves(MR.TOO_LARGE, tr) == 0
    assert MR.act_ld(MR.TWO_WAVES) == 130 and MR.act_ld(MR.ONE_WAVE) == 162 and MR.act_ld((3, 7, 5)) == 34
    assert MR.act_ld((200, 7)) == 226  # one layer: the hidden width of the descriptor is 0
    assert MR.lds_bytes(MR.TWO_WAVES, 0) == 98304 and MR.lds_bytes(MR.TWO_WAVES, 4) == 164864 > 160 * 1024
    assert MR.lds_bytes(MR.TWO_WAVES, 2) == 131584 > 64 * 1024
    assert MR.lds_bytes(MR.ONE_WAVE, 1) == 129024 + 20736 and MR.lds_bytes(MR.ONE_WAVE, 2) > 160 * 1024
    assert MR.frag_floats((70, 130, 65), 0, False) == 144 * 72 and MR.frag_floats((70, 130, 65), 0, True) == 80 * 132
    assert [-(-w // 16) for w in (70, 130)] == [5, 9]  # odd numbers of sixteen-blocks: layer_tile's unpaired last block


def test_grids():
    assert MR.blocks_for_tiles(1, 4) == 1 and MR.blocks_for_tiles(100, 4) == 2 and MR.blocks_for_tiles(100, 1) == 7
    dims, n = MR.FWD_CAPPED
    assert -(-n // 16) == 8194 > 4 * 2048 and MR.blocks_for_tiles(n, 4) == 2048 == MR.blocks_for_tiles(n - 32, 4)
    assert MR.blocks_for_tiles(16 * 4 * 2047, 4) == 2047
    assert MR.wgrad_grid(MR.WGRAD_RAGGED, 1023) == (1, 12, [0, 6]) and MR.wgrad_grid(MR.WGRAD_RAGGED, 1025)[0] == 2
    assert MR.wgrad_grid(MR.WGRAD_RAGGED, 5, layers=[1]) == (1, 6, [0])
    dims, n = MR.WGRAD_CAPPED
    assert MR.wgrad_grid(dims, n) == (256, 2, [0, 1]) and MR.wgrad_grid(dims, 262144)[0] == 256
    assert MR.wgrad_grid(dims, 4 * 256 * 255)[0] == 255
    for k in MR.MERGE_COUNTS:
        assert MR.chain_workgroups(64 * k - 7, 256) == k
    assert MR.chain_workgroups(1, 256) == 1 and MR.chain_workgroups(70001, 1024) == 1024 and MR.chain_workgroups(70001, 10 ** 9) == 1094
    assert MR.chain_workgroups(1000, 5) == 5 and MR.chain_workgroups(1000, 1) == 1 and MR.chain_workgroups(1000, 256) == 16
