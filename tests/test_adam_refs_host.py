"""tests/adam_refs.py on the CPU: the exact fma, the replay against fp64 Adam within the counted bound and against
torch.optim.Adam / AdamW, the dead rule, the robustness of every (step, hyper-parameter) combination the GPU tests use, the
launch plan at every named size, and the case lists against each plausible wrong kernel."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import adam_refs as A

f32, f64, f16 = np.float32, np.float64, np.float16


def _round32(x: Fraction) -> np.float32:
    """the fp32 nearest to an exact rational, ties to even (normal range, or zero)"""
    if x == 0:
        return f32(0)
    s, x = (-1 if x < 0 else 1), abs(x)
    e = math.floor(math.log2(x))
    e += (x >= Fraction(2) ** (e + 1)) - (x < Fraction(2) ** e)  # (log2 of a rational through a float: mend the last unit)
    assert -126 <= e <= 127
    q = x / Fraction(2) ** (e - 23)  # in [2^23, 2^24)
    n = q.numerator // q.denominator
    rest = q - n
    n += (rest > Fraction(1, 2)) or (rest == Fraction(1, 2) and n % 2 == 1)
    return f32(s * float(Fraction(n) * Fraction(2) ** (e - 23)))


def test_fma32_is_the_single_rounding_of_the_exact_value():
    r = np.random.default_rng(0)
    n = 3000
    a = (r.choice([-1.0, 1.0], n) * r.uniform(1, 2, n) * 2.0 ** r.integers(-33, 33, n)).astype(f32)
    b = (r.choice([-1.0, 1.0], n) * r.uniform(1, 2, n) * 2.0 ** r.integers(-33, 33, n)).astype(f32)
    c = (r.choice([-1.0, 1.0], n) * r.uniform(1, 2, n) * 2.0 ** r.integers(-66, 66, n)).astype(f32)
    # a third each: any c; c of the product's size and the other sign (cancellation); c far below the product's last bit
    c[n // 3:2 * n // 3] = (-(a * b) * r.uniform(0.5, 2, n).astype(f32))[n // 3:2 * n // 3]
    c[2 * n // 3:] = ((a * b) * f32(2.0) ** r.integers(-60, -20, n).astype(f32))[2 * n // 3:]
    # double-rounding cases: the product is 1 + 2^-24 (a tie of fp32) or 1 + 3 * 2^-24 exactly, c decides the side
    ties = [(24929 * 2.0 ** -24, 673.0, 2.0 ** -80, 1 + 2.0 ** -23), (24929 * 2.0 ** -24, 673.0, -2.0 ** -80, 1.0),
            (24929 * 2.0 ** -24, 673.0, 0.0, 1.0), (-24929 * 2.0 ** -24, 673.0, -2.0 ** -80, -(1 + 2.0 ** -23)),
            (24929 * 2.0 ** -24, 673.0, 2.0 ** -149, 1 + 2.0 ** -23)]
    assert 24929 * 673 == 2 ** 24 + 1
    for k in range(200):  # more products of the form 1 + odd * 2^-24: ties of the 24-bit grid, c far below decides the side
        x = 2 ** 24 + 2 * k + 1
        d = next((d for d in range(3, 5000, 2) if x % d == 0), None)
        if d is not None:
            for cc in (2.0 ** -90, -2.0 ** -90):
                ties.append((x // d * 2.0 ** -24, float(d), cc, float(_round32(Fraction(x, 2 ** 24) + Fraction(cc)))))
    assert len(ties) > 20
    ta, tb, tc, tw = (np.array(x, f64) for x in zip(*ties))
    assert np.array_equal(ta.astype(f32).astype(f64), ta) and np.array_equal(tb.astype(f32).astype(f64), tb)
    got = A.fma32(ta.astype(f32), tb.astype(f32), tc.astype(f32))
    assert not A.mismatches(got, tw.astype(f32)).size
    with np.errstate(all="ignore"):  # the naive fp64 evaluation rounds twice and gets the first one wrong
        assert f32(f64(ta[0]) * f64(tb[0]) + f64(tc[0])) == f32(1.0)
    got = A.fma32(a, b, c)
    checked = 0
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        if exact != 0 and not (2.0 ** -120 < abs(exact) < 2.0 ** 120):
            continue
        want = _round32(exact)
        assert got[i].view(np.uint32) == want.view(np.uint32) or (exact == 0 and got[i] == 0), (i, a[i], b[i], c[i], got[i], want)
        checked += 1
    assert checked > 0.9 * n
    # zeros, infinities and NaN pass through as IEEE says
    z = A.fma32(f32([0.0, -0.0, np.inf, np.nan, 1.0]), f32([1.0, 1.0, 1.0, 1.0, np.inf]), f32([-0.0, -0.0, 1.0, 1.0, -np.inf]))
    assert np.signbit(z[1]) and not np.signbit(z[0]) and z[2] == np.inf and np.isnan(z[3]) and np.isnan(z[4])


def _every_case():
    return A.all_cases()


def test_every_step_and_hyper_parameter_of_the_case_lists_is_robust():
    seen = set()
    for c, _ in _every_case():
        for k, n in enumerate(c.ns):
            seen.add((c.steps[k],) + tuple(c.hyper))
    seen |= {(s,) + tuple(A.Hyper()) for s in range(1, 8)}  # the HashGridAdam test: six steps at the defaults
    assert len(seen) > 60
    for s in sorted(seen):
        assert A.robust(*s), s
    # the predicate is not vacuous: a scalar that sits on an fp32 tie is refused
    tie = float(f32(1e-15)) + float(np.spacing(f32(1e-15))) / 2
    assert not A.robust(1, 1e-2, 0.9, 0.999, tie, 0.0, 1.0) and A.robust(1, 1e-2, 0.9, 0.999, tie * (1 + 2.0 ** -40), 0.0, 1.0)


def test_adam_args_round_once_from_fp64():
    a = A.adam_args(3, 1e-2, 0.9, 0.999, 1e-15, 1e-2, 0.5)
    assert a.omb2 == f32(1.0 - 0.999) and a.omb2 != f32(1.0) - f32(0.999)
    assert a.step_size == f32(1e-2 / (1.0 - 0.9 ** 3)) and a.inv_bc2_sqrt == f32(1.0 / math.sqrt(1.0 - 0.999 ** 3))
    assert a.decay == f32(1.0 - 1e-2 * 1e-2) and a.eps == f32(1e-15) and a.grad_scale == f32(0.5)
    assert A.adam_args(1, 1e-2, 0.9, 0.999, 1e-50, 0.0, 1.0).eps == 0


def _small_single_tensor_cases():
    return [c for c, single in _every_case() if not single and len(c.ns) == 1 and c.ns[0] <= 2000]


def test_replay_stays_within_the_counted_bound_of_fp64_adam():
    inside = total = 0
    for c in _small_single_tensor_cases() + [A.dev_lr_decay_case(), A.dev_scales_case()]:
        s = A.Slabs(c)
        for k, n in enumerate(c.ns):
            p, g, m, v = s.view("p", k), s.g(k), s.view("m", k), s.view("v", k)
            h = c.hyper
            p1, m1, v1, _ = A.replay(p, g, m, v, A.case_args(c, k), plain=True)
            q1, _, _ = A.adam64(p, g, m, v, c.steps[k], *h)
            b = A.bound64(p, g, m, v, c.steps[k], *h)
            ok = np.isfinite(b)
            with np.errstate(all="ignore"):
                err = np.abs(p1.astype(f64) - q1)
            assert np.all(err[ok] <= b[ok]), (c.name, np.flatnonzero(ok & ~(err <= b))[:5], err[ok].max())
            # by class where fp64 itself is not finite
            bad = ~np.isfinite(q1)
            assert np.array_equal(np.isnan(p1[bad]), np.isnan(q1[bad])) and np.array_equal(p1[bad][~np.isnan(q1[bad])], q1[bad][~np.isnan(q1[bad])].astype(f32))
            inside, total = inside + int(ok.sum()), total + n
    assert inside > 0.6 * total, (inside, total)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_replay_follows_torch_adam_on_the_cpu(wd):
    r = np.random.default_rng(5)
    n = 4099
    p = r.uniform(-1, 1, n).astype(f32) * f32(1e-3)
    a = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = (torch.optim.AdamW([a], lr=1e-2, eps=1e-15, weight_decay=wd, foreach=False) if wd
           else torch.optim.Adam([a], lr=1e-2, eps=1e-15, foreach=False))
    m, v = np.zeros(n, f32), np.zeros(n, f32)
    for step in range(1, 6):
        g = (r.standard_normal(n) * 10.0 ** (step % 4 - 2)).astype(f32)
        g[r.random(n) < 0.5] = 0
        a.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v, _ = A.replay(p, g, m, v, A.adam_args(step, 1e-2, 0.9, 0.999, 1e-15, wd, 1.0))
        assert torch.allclose(torch.from_numpy(p), a.detach(), rtol=2e-6, atol=3e-8), step
    st = opt.state[a]
    assert torch.allclose(torch.from_numpy(m), st["exp_avg"], rtol=1e-6, atol=1e-12)
    assert torch.allclose(torch.from_numpy(v), st["exp_avg_sq"], rtol=1e-6, atol=1e-20)


def test_the_dead_rule_is_the_plain_arithmetic_when_eps_is_positive():
    n = 64
    p = np.tile(f32([0.0, -0.0, 0.3, -1.7, 1e30, -1e-40, 65504.0, 3.1e-5]), n // 8)
    z = np.zeros(n, f32)
    for g in (z, -z, z.astype(f16), (-z).astype(f16)):
        for eps in (1e-15, 1e-8, 1e-40):  # (1e-40: a denormal fp32, still > 0)
            for step in (1, 2, 1000):
                a = A.adam_args(step, 1e-2, 0.9, 0.999, eps, 0.0, 0.5)
                assert a.decay == 1 and a.eps > 0
                img0 = A.half_rn(p)
                plain = A.replay(p, g, z, z, a, img0, plain=True)
                ruled = A.replay(p, g, z, z, a, img0)
                for x, y, start in zip(plain, ruled, (p, z, z, img0)):
                    assert not A.mismatches(x, y).size and not A.mismatches(x, start).size
    for eps in (0.0, 1e-50):  # rounds to 0 in fp32: 0 / 0, and no rule hides it
        a = A.adam_args(2, 1e-2, 0.9, 0.999, eps, 0.0, 1.0)
        for plain in (True, False):
            p1, m1, v1, _ = A.replay(p, z, z, z, a, plain=plain)
            assert np.isnan(p1).all() and not m1.any() and not v1.any()
    # torch gives NaN there too
    t = torch.nn.Parameter(torch.ones(4))
    t.grad = torch.zeros(4)
    torch.optim.Adam([t], lr=1e-2, eps=0.0, foreach=False).step()
    assert torch.isnan(t).all()
    # under AdamW a dead element decays: p * decay rounded once
    a = A.adam_args(2, 1e-2, 0.9, 0.999, 1e-15, 1e-2, 1.0)
    p1, m1, v1, _ = A.replay(p, z, z, z, a)
    with np.errstate(all="ignore"):
        assert not A.mismatches(p1, p * a.decay).size and not m1.any() and not v1.any()


def test_launch_plan_reports_the_intended_branch_at_every_named_size():
    for n in A.SMALL_NS:
        pl = A.launch_plan([n])[0][0]
        assert pl.blocks == (2 if n >= 1028 else 1) and pl.tail == n % 4
        assert pl.passes_first == (1 if n >= 4 else 0) and pl.passes_last == (1 if n in (1024, 1025) else 0)  # (256 lanes, 256 groups)
    want = {A.ALONE_NS[0]: (1, 1, 0), A.ALONE_NS[1]: (2, 1, 0), A.ALONE_NS[2]: (2, 1, 3)}
    for n, (first, last, tail) in want.items():
        for single in (True, False):
            pl = A.launch_plan([n], single=single)[0][0]
            assert (pl.blocks, pl.passes_first, pl.passes_last, pl.tail) == (4096, first, last, tail), n
        assert A._passes(299, n // 4, 4096 * 256) == (2 if tail else 1) and A._passes(300, n // 4, 4096 * 256) == 1
    # in company the cap is 1024; alone, the same length stays below 4096 workgroups and takes one pass
    want = {A.COMPANY_NS[0]: (1, 1, 0), A.COMPANY_NS[1]: (2, 1, 0), A.COMPANY_NS[2]: (2, 1, 3)}
    for n, (first, last, tail) in want.items():
        plans, launches = A.launch_plan([A.COMPANION, n])
        assert launches == [[0, 1]] and plans[0].blocks == 1
        assert (plans[1].blocks, plans[1].passes_first, plans[1].passes_last, plans[1].tail) == (1024, first, last, tail), n
        assert A.launch_plan([n])[0][0].passes_first == 1
    # the batching: 24 per launch, empties hold no slot, a launch without a live tensor does not happen
    by_name = {c.name: c for c in A.batch_cases()}
    count = lambda name: [len(l) for l in A.launch_plan(by_name[name].ns)[1]]  # noqa: E731
    assert count("live23") == [23] and count("live24") == [24] and count("live25") == [24, 1]
    assert count("live48") == [24, 24] and count("live49") == [24, 24, 1]
    assert count("only-empties") == [] and count("24-then-empties") == [24]
    c = by_name["empties-between"]
    assert c.ns[0] == c.ns[12] == c.ns[24] == c.ns[-1] == 0 and sum(n > 0 for n in c.ns) == 30
    plans, launches = A.launch_plan(c.ns)
    assert [len(l) for l in launches] == [24, 6] and 24 not in launches[0] + launches[1] and launches[1][0] == 27
    for name in ("live25", "live49", "empties-between"):
        c = by_name[name]
        plans = [p for p in A.launch_plan(c.ns)[0] if p]
        assert {p.tail for p in plans} == {0, 1, 2, 3} and min(p.blocks for p in plans) == 1 and max(p.blocks for p in plans) > 2
        assert len(set(c.steps)) == len(c.steps) and min(c.steps) == 1
        live = [k for k, n in enumerate(c.ns) if n]
        assert {(c.ghalf[k], c.image[k]) for k in live} == {(False, False), (False, True), (True, False), (True, True)}
    assert A.launch_plan(A.error_case().ns)[1][1][0] <= 27 and len(A.error_case().ns) == 30  # the 28th sits in the second launch
    assert A.launch_plan([A.DEAD_N])[0][0].blocks == 2 and A.DEAD_GROUP < 256 and A.DEAD_N % 4 == 3
    # the check kernel: one unrolled iteration for every lane, one remainder iteration for every lane, a second one for
    # lanes 0 .. 699, a full tail
    for name, blocks in (("fp32-company", 1024), ("fp16-company", 1024), ("fp32-alone", 4096)):
        n, half, where, pl = A.check_positions(name)
        assert pl.blocks == blocks
        assert (pl.unrolled_first, pl.unrolled_last, pl.rem_first, pl.rem_last, pl.rem2_lanes) == (1, 1, 2, 1, 700), (name, pl)
        assert pl.tail == (7 if half else 3) and len(where) == (5 * 3 + 3) * (8 if half else 4) + pl.tail
    assert A.launch_plan([262144, 5], check_half=[False, False])[0][0].unrolled_first == 0  # (the largest size tested before)


def _variant_cases(variant):
    """the cases on which each wrong kernel has to show"""
    if variant == "no_second_pass":
        return [(c, single) for c, single in _every_case()
                if not single and c.ns[-1] in (A.ALONE_NS[2], A.COMPANY_NS[2]) and c.name.endswith("-f")]
    return [(c, single) for c, single in _every_case() if max(c.ns, default=0) < 1 << 16]


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_the_case_lists_tell_a_correct_kernel_from_a_wrong_one(variant):
    cases = _variant_cases(variant)
    assert cases
    hits = [c.name for c, single in cases if A.differs(c, variant, single)]
    assert hits, variant
    if variant == "no_second_pass":
        assert len(hits) == len(cases) >= 2  # the alone and the in-company size, each on its own
    if variant.startswith("skip_ignores_"):  # the pattern made for it catches it, in fp32 and in fp16
        assert hits.count(f"dead-one-{variant[-2:]}") == 2, hits
    if variant == "dead_no_decay":
        assert hits.count("dead-decay") == 2
    if variant == "neighbour_args":
        assert all(len([n for n in c.ns if n]) < 2 or c.name in hits for c, _ in cases if c.name.startswith("live"))


def test_the_dead_cases_are_what_they_say():
    for ghalf in (False, True):
        d = A.dead_cases(ghalf)
        assert len(d) == 16
        s = 4 * A.DEAD_GROUP
        for name, c in d.items():
            sl = A.Slabs(c)
            g, m, v, p = sl.g(0), sl.view("m", 0), sl.view("v", 0), sl.view("p", 0)
            nz = sum(int(np.count_nonzero(x[s:s + 4])) for x in (g, m, v))
            assert nz == (1 if name.startswith("one-") else 0) and not any(x[-3:].any() for x in (g, m, v))
            assert not A.mismatches(sl.view("image", 0)[s:s + 4], A.half_rn(p[s:s + 4])).size
            e = A.expected(c, sl)
            o = sl.off[0] + s
            t = sl.off[0] + A.DEAD_N - 3
            if name in ("zero",):
                assert all(not A.mismatches(e[k][o:o + 4], sl.a[k][o:o + 4]).size for k in A.Slabs.KINDS)
            if name == "decay":
                with np.errstate(all="ignore"):
                    assert not A.mismatches(e["p"][o:o + 4], p[s:s + 4] * A.case_args(c, 0).decay).size
            if name.startswith("eps"):
                assert np.isnan(e["p"][o:o + 4]).all() and np.isnan(e["p"][t:t + 3]).all() and np.isnan(e["image"][t:t + 3]).all()
            if name.startswith("one-"):
                assert A.mismatches(e["p"][o:o + 4], sl.a["p"][o:o + 4]).size + A.mismatches(e["m"][o:o + 4], sl.a["m"][o:o + 4]).size \
                    + A.mismatches(e["v"][o:o + 4], sl.a["v"][o:o + 4]).size > 0


def test_slabs_are_aligned_and_fenced():
    c = A.batch_cases()[2]
    s = A.Slabs(c)
    ends = [0] + [o + n for o, n in zip(s.off, c.ns)]
    for k, o in enumerate(s.off):
        assert o % 8 == 0 and o - ends[k] >= A.SENTINEL
    assert s.size - ends[-1] >= A.SENTINEL
    p, g, m, v = A.tensor_values(1031, 3, False)
    with np.errstate(all="ignore"):
        assert np.isnan(g).any() and np.isinf(g).any() and (g == 0).any() and np.signbit(g[g == 0]).any() and (g * g == np.inf).any()
        assert ((g != 0) & (g * g == 0)).any() and ((np.abs(g) < 2.0 ** -126) & (g != 0)).any() and (p == 1e30).any()
        assert np.signbit(p[p == 0]).any() and ((np.abs(m) < 2.0 ** -126) & (m != 0)).any() and ((v < 2.0 ** -126) & (v != 0)).any()
        ok = np.isfinite(g) & (g != 0)
        assert np.log10(np.abs(g[ok]).max() / np.abs(g[ok & (np.abs(g) > 1e-10)]).min()) > 7
    p, g, m, v = A.tensor_values(1031, 3, True)
    assert g.dtype == f16 and np.isnan(g).any() and np.isinf(g).any() and (np.abs(g) == 65504).any()
    assert ((np.abs(g) < 2.0 ** -14) & (g != 0)).any()
