"""tests/norm_refs.py on the CPU: the float64 references against torch's own group_norm / layer_norm (float64, autograd), what
each sweep of tests/test_hip_norm_geometry.py promises to cover, as set assertions over its case dicts, and the conditioning
rule -- no case of any sweep outside it."""
import pytest
import torch
import torch.nn.functional as F

import norm_refs as R
from conftest import max_rel


def _cases(name):
    return R.sweep_cases(name)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,c,groups,film", [(2, 33, 12, 3, True), (1, 5, 32, 32, False), (3, 64, 40, 8, True), (2, 7, 6, 1, False)])
def test_group_norm_references_equal_torch_float64(n, hw, c, groups, film):
    g = torch.Generator().manual_seed(n * 100 + c)
    x = torch.randn(n, hw, c, generator=g) * 2 + 0.3
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    fl = torch.randn(n, 2 * c + 4, generator=g) if film else None
    want = F.group_norm(x.double().transpose(1, 2), groups, gamma.double(), beta.double(), R.EPS)
    if film:
        want = want * (1 + fl.double()[:, :c, None]) + fl.double()[:, c:2 * c, None]
    assert max_rel(R.ref_group_norm(x, groups, gamma, beta, fl), want.transpose(1, 2)) < 1e-13
    # the same coefficients from the per-channel sums, and from a partial table of the sums of three row ranges
    sums = R.ref_chan_sums(x)
    assert max_rel(sums[..., 0], x.double().sum(1)) < 1e-15 and max_rel(sums[..., 1], (x.double() ** 2).sum(1)) < 1e-15
    a, b = R.ref_gn_coef(*R.ref_group_stats(x, groups), gamma, beta, fl)
    a1, b1 = R.ref_gn_coef(*R.ref_stats_from_sums(sums, groups, hw), gamma, beta, fl)
    assert max_rel(a1, a) < 1e-12 and max_rel(b1, b) < 1e-12
    cuts = [0, hw // 3, hw // 2 + 1, hw]
    part = torch.stack([R.ref_chan_sums(x[:, lo:hi]).transpose(1, 2) for lo, hi in zip(cuts, cuts[1:])], 1)     # [n, 3, 2, c]
    assert max_rel(R.ref_fold(part), sums) < 1e-14


@pytest.mark.parametrize("gu_mode,gres_mode", [(0, None), (0, 2), (1, 1), (2, 0), (1, 2), (2, 1)])
@pytest.mark.parametrize("silu,film,drop", [(1, True, 0.25), (0, False, 0.0)])
def test_group_norm_backward_reference_equals_torch_float64(gu_mode, gres_mode, silu, film, drop):
    """ref_gn_backward differentiates its own GroupNorm; the same chain through torch.nn.functional.group_norm must agree"""
    g = torch.Generator().manual_seed(31 + gu_mode)
    n, h, w, c, groups = 2, 4, 6, 12, 3
    x = torch.randn(n, h, w, c, generator=g) * 2 + 0.3
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    fl = torch.randn(n, 2 * c, generator=g) if film else None
    keep = torch.rand(n, h, w, c, generator=g) > drop if drop else None
    gu = torch.randn(n, *R.resampled_hw(h, w, gu_mode), c, generator=g)
    gres = torch.randn(n, *R.resampled_hw(h, w, gres_mode), c, generator=g) if gres_mode is not None else None
    args = (x, groups, gamma, beta, fl, silu, keep, drop, gu, gu_mode, gres, gres_mode)
    own, ref = R.ref_gn_backward(*args), R.ref_gn_backward(*args, torch_norm=True)
    for nm in ("dx", "dgamma", "dbeta", "dfilm"):
        assert (own[nm] is None) == (not film) if nm == "dfilm" else own[nm] is not None
        if own[nm] is not None:
            assert max_rel(own[nm], ref[nm]) < 1e-12, nm
    # ... and the resample adjoints are what the kernels' fetch rule says: a quarter of the pooled gradient, the sum of the 2x2 block
    if gres_mode is not None and not silu and not film:
        only_res = R.ref_gn_backward(x, groups, gamma * 0, beta, None, 0, None, 0.0, gu, gu_mode, gres, gres_mode)["dx"]
        gd = gres.double()
        want = {0: lambda: gd, 1: lambda: 0.25 * gd.repeat_interleave(2, 1).repeat_interleave(2, 2),
                2: lambda: gd.reshape(n, h, 2, w, 2, c).sum((2, 4))}[gres_mode]()
        assert max_rel(only_res, want) < 1e-12


@pytest.mark.parametrize("rows,c", [(5, 65), (3, 2), (4, 1), (2, 320)])
def test_layer_norm_references_equal_torch_float64(rows, c):
    g = torch.Generator().manual_seed(rows * 1000 + c)
    x = (torch.randn(rows, c, generator=g) * 3 + 1)
    gamma, beta, res = torch.randn(c, generator=g), torch.randn(c, generator=g), torch.randn(rows, c, generator=g)
    gy, gres, base = (torch.randn(rows, c, generator=g) for _ in range(3))
    xx, gam = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    y = F.layer_norm(xx, (c,), gam, beta.double(), R.EPS)
    y.backward(gy.double())
    assert max_rel(R.ref_ln_apply(x, gamma, beta, res), y.detach() + res.double()) < 1e-13
    assert max_rel(R.ref_ln_apply(x, gamma), y.detach() - beta.double()) < 1e-12
    mean, rstd = R.ref_ln_stats(x)
    assert max_rel(mean, x.double().mean(1)) < 1e-14
    assert max_rel(rstd, 1 / torch.sqrt(x.double().var(1, unbiased=False) + R.EPS)) < 1e-13
    got = R.ref_ln_backward(x, gy, gamma, gres, base)
    assert float((got["dst"] - (xx.grad + gres.double() + base.double())).abs().max()) < 1e-9 * float(gy.abs().max())
    assert float((got["gxhat"].sum(0) - gam.grad).abs().max()) < 1e-12 * rows * float(gy.abs().max())      # (one channel: exactly 0)
    assert max_rel(R.ref_ln_backward(x, gy, gamma)["dst"], got["dst"] - gres.double() - base.double()) < 1e-9


def test_guarded_buffer_on_the_cpu():
    buf = R.Guarded(3, 12, 4, 4, device="cpu")
    assert buf.untouched() and not buf.written()
    buf.fill(torch.ones(3, 4))
    assert buf.untouched() and buf.written() and torch.equal(buf.owned(), torch.ones(3, 4))
    buf.tensor()[1, 3] = 0.0
    assert not buf.untouched()
    for row in (-1, 3, 4, 5):            # the guard row in front, and each of the three behind (a last block of four rows)
        buf = R.Guarded(3, 12, 4, 4, device="cpu")
        buf.bits.view(torch.float32).view(-1, 12)[1 + row, 5] = 0.0
        assert not buf.untouched(), row
    assert torch.isnan(R.padded(torch.zeros(2, 3), 5)[:, 3:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# what the sweeps cover
# ---------------------------------------------------------------------------------------------------------------------
def _values(cases, key):
    return {cs[key] for cs in cases}


def test_sweep_sizes_and_seeds():
    for name, want in (("chan_stats", 24), ("parts", 29), ("forward", 24), ("backward", 30), ("layernorm", 24), ("degenerate", 6),
                       ("ln_degenerate", 3), ("offset", 12)):
        cases = _cases(name)
        assert len(cases) == want, (name, len(cases))
        assert all("seed" in cs for cs in cases)
        assert cases == _cases(name), "a sweep is a function of its seed alone"
    for name in ("chan_stats", "parts", "forward", "backward", "layernorm"):
        assert 24 <= len(_cases(name)) <= 32


def test_chan_stats_sweep_covers_its_docstring():
    cases = _cases("chan_stats")
    assert _values(cases, "c") == set(R.CS_C) and _values(cases, "hw") == set(R.CS_HW) and _values(cases, "n") == {1, 2, 3}
    assert any(cs["c"] % 4 for cs in cases) and any(cs["c"] % 4 == 0 for cs in cases)          # both branches of the kernel
    assert any(cs["c"] % 4 and cs["c"] > 32 for cs in cases)                                   # the scalar branch over two slabs
    assert any(cs["c"] % 4 == 0 and cs["c"] % 32 for cs in cases)                              # a ragged last slab of quads
    assert any(cs["c_off"] & 1 for cs in cases) and any(cs["c_off"] == 0 for cs in cases)
    assert all(cs["c_total"] > cs["c_off"] + cs["c"] for cs in cases)
    assert any(cs["hw"] < 32 for cs in cases) and any(cs["hw"] > 32 and cs["hw"] % 32 for cs in cases)


def test_parts_sweep_covers_its_docstring():
    cases = _cases("parts")
    assert _values(cases, "parts0") >= set(R.PARTS) and _values(cases, "c0") >= set(R.PARTS_C0)
    assert _values(cases, "c1") == set(R.PARTS_C1)
    assert any(cs["c1"] > 0 and cs["parts1"] == 0 for cs in cases) and any(cs["c1"] > 0 and cs["parts1"] > 0 for cs in cases)
    assert _values(cases, "film") == {False, True} and all(cs["film_ld"] > 2 * (cs["c0"] + cs["c1"]) for cs in cases)
    # thread groups G = 512 // c with a remainder, and one thread per channel
    cs_all = {cs["c0"] + cs["c1"] for cs in cases}
    assert {96, 160} <= cs_all and any(c >= 512 for c in cs_all) and any(c < 512 and 512 % c == 0 for c in cs_all)
    # every tail of the fold: the 8-wide loop, the 4-wide block, the scalar loop -- alone and behind one another
    trips = set()
    for cs in cases:
        trips |= R.fold_trips(cs["parts0"], cs["c0"] + cs["c1"])
        if cs["parts1"]:
            trips |= R.fold_trips(cs["parts1"], cs["c0"] + cs["c1"])
    assert any(t8 and not t4 and not t1 for t8, t4, t1 in trips)
    assert any(t4 and not t8 and not t1 for t8, t4, t1 in trips)
    assert any(t1 and not t8 and not t4 for t8, t4, t1 in trips)
    assert any(t8 and t4 and t1 for t8, t4, t1 in trips) and any(t4 and t1 for t8, t4, t1 in trips)
    assert any(t8 >= 2 for t8, _, _ in trips)
    # the raised dynamic-LDS launch: 24 bytes per channel above the 64 KB default, inside 160 KB
    assert any(64 * 1024 < 24 * (cs["c0"] + cs["c1"]) <= 160 * 1024 for cs in cases)
    assert R.fold_trips(12, 1024) == {(1, 1, 0)} and R.fold_trips(7, 96) == {(0, 0, 2), (0, 0, 1)}


def test_forward_sweep_covers_its_docstring():
    cases = _cases("forward")
    assert _values(cases, "groups") == set(R.FWD_GROUPS)
    assert {sum(cs["srcs"]) // cs["groups"] for cs in cases} == set(R.FWD_CPG)
    assert _values(cases, "h") <= set(R.CS_HW) and len(_values(cases, "h")) >= len(R.CS_HW) - 1
    assert any(len(cs["srcs"]) == 2 for cs in cases) and all(len(set(cs["srcs"])) == len(cs["srcs"]) for cs in cases)
    assert any(len(cs["srcs"]) == 2 and cs["srcs"][0] % 4 for cs in cases)               # a channel offset off the quad grid
    assert any(len(cs["srcs"]) == 2 and cs["srcs"][0] % (sum(cs["srcs"]) // cs["groups"]) for cs in cases)   # a group across both sources
    assert _values(cases, "film") == {False, True} and all(cs["film_ld"] > 2 * sum(cs["srcs"]) for cs in cases)


def test_backward_sweep_covers_its_docstring():
    cases = _cases("backward")
    plain = [cs for cs in cases if not cs["rows"]]
    assert {(cs["h"], cs["w"]) for cs in plain} == set(R.BWD_HW)
    # the four-pixels-in-flight loop of gn_bwd_reduce_kernel (same-resolution gradient): no trip, one trip of every lane and no
    # tail, one trip and a tail, two trips -- hw on both sides of 96 and of 128
    trips = [R.reduce_trips(cs["h"] * cs["w"]) for cs in plain if cs["gu_mode"] == R.RS_NONE]
    assert any(all(wide == 0 for wide, _ in t) for t in trips) and any(t == {(1, 0)} for t in trips)
    assert any((1, 1) in t for t in trips) and any(any(wide == 2 for wide, _ in t) for t in trips)
    assert R.reduce_trips(96) == {(0, 3)} and R.reduce_trips(97) == {(1, 0), (0, 3)} and R.reduce_trips(144) == {(1, 1), (1, 0)}
    assert {cs["srcs"][-1] for cs in plain} == set(R.BWD_C)
    assert {cs["srcs"][0] if len(cs["srcs"]) == 2 else 0 for cs in plain} == set(R.BWD_OFF)
    assert {(cs["gu_mode"], cs["gres_mode"]) for cs in plain} == set(R.BWD_MODE_PAIRS)
    assert all(R.RS_AVGPOOL2 not in (cs["gu_mode"], cs["gres_mode"]) for cs in cases if (cs["h"] | cs["w"]) & 1)
    assert any((cs["h"] | cs["w"]) & 1 and cs["gu_mode"] == R.RS_UP2 for cs in cases) or \
        any((cs["h"] | cs["w"]) & 1 and cs["gres_mode"] == R.RS_UP2 for cs in cases)
    for key, want in (("silu", {0, 1}), ("film", {False, True}), ("drop_p", set(R.DROPS)), ("accumulate", {0, 1}), ("dst_off", {0, 4})):
        assert _values(cases, key) == want, key
    assert all(cs["gu_ld"] > sum(cs["srcs"]) and cs["gres_ld"] > sum(cs["srcs"]) and cs["dst_pad"] > 0 for cs in cases)
    assert any(cs["drop_p"] > 0 and cs["gu_mode"] != R.RS_NONE for cs in cases)
    assert any(len(cs["srcs"]) == 2 and cs["srcs"][0] % (sum(cs["srcs"]) // cs["groups"]) for cs in cases)   # a group across both sources
    rows = [cs for cs in cases if cs["rows"]]
    assert sorted(cs["srcs"] for cs in rows) == [(16,), (64,)] and all((cs["n"], cs["h"], cs["w"]) == (1, 32, 32) for cs in rows)
    assert all(cs["gu_mode"] == R.RS_NONE for cs in rows)


def test_layernorm_sweep_covers_its_docstring():
    cases = _cases("layernorm")
    assert _values(cases, "rows") == set(R.LN_ROWS) and _values(cases, "c") == set(R.LN_C)
    for key in ("beta", "res", "gres", "gxhat"):
        assert _values(cases, key) == {False, True}, key
    assert _values(cases, "accumulate") == {0, 1}
    assert any(cs["c"] % 64 and cs["c"] > 64 for cs in cases) and any(cs["rows"] % 4 for cs in cases)
    assert all(cs["gres"] for cs in cases if cs["c"] <= 2)


def test_degenerate_and_offset_families():
    deg = _cases("degenerate")
    assert {cs["degenerate"][0] for cs in deg} == {0.0, 0.25}
    assert any(cs["film"] for cs in deg) and any(not cs["film"] and cs["degenerate"][0] == 0.0 for cs in deg)
    for cs, t, _, _ in R.sweep_reference("degenerate"):
        value, grp = cs["degenerate"]
        cpg = sum(cs["srcs"]) // cs["groups"]
        assert bool((t["x"][..., grp * cpg:(grp + 1) * cpg] == value).all()) and float(t["x"].std()) > 1.0
    for cs, t, ref, _ in R.sweep_reference("ln_degenerate"):
        r, v = cs["constant_row"]
        assert bool((t["x"][r] == v).all()) and abs(float(ref["rstd"][r]) - R.EPS ** -0.5) < 1e-9 * R.EPS ** -0.5
    off = _cases("offset")
    assert {(cs["r"], cs["h"]) for cs in off} == {(r, hw) for r in R.OFFSET_R for hw in R.OFFSET_HW}
    assert R.offset_bound(4) < 1.5e-6 < R.offset_bound(5) and R.offset_bound(16) > 2e-5
    for cs, t, ref, _ in R.sweep_reference("offset"):            # the data's own largest r: what the bound is evaluated at
        if cs["r"] <= 4:
            assert R.offset_bound(ref["r"]) < 2e-6, (cs["r"], ref["r"])
        else:
            assert 0.9 * cs["r"] <= ref["r"] <= 1.5 * cs["r"], (cs["r"], ref["r"])


# ---------------------------------------------------------------------------------------------------------------------
# the conditioning rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chan_stats", "parts", "forward", "backward", "layernorm", "degenerate", "ln_degenerate"])
def test_every_case_meets_the_conditioning_rule(name):
    """recomputed from the case dicts alone: torch's fp32 arithmetic on a case's inputs is within a quarter of the tolerance the
    GPU test applies to it, and no GroupNorm group is offset by more than R_MAX standard deviations.  At most 0 cases may miss."""
    missed = []
    for cs in _cases(name):
        t = R.case_tensors(cs)
        ref, cond = R.case_reference(cs, t)
        assert cond and all(tol in R.TOL.values() for _, tol in cond.values())
        bad = R.rule_misses(cs, ref, cond)
        if bad:
            missed.append((cs, bad))
    assert len(missed) == 0, missed


def test_the_rule_rejects_what_it_should():
    """a group far from zero mean passes torch's fp32 arithmetic and misses the rule through its offset ratio alone; the offset
    family is exempt and carries its own bound"""
    cs = dict(kind="gn", n=1, h=64, w=1, srcs=(32,), groups=8, film=False, film_ld=0, mu=32.0, sigma=1.0, seed=7)
    ref, cond = R.case_reference(cs, R.case_tensors(cs))
    bad = R.rule_misses(cs, ref, cond)
    assert [b[0] for b in bad] == ["group offset ratio"] and ref["r"] > 16
    assert R.rule_misses(dict(cs, r=32), ref, cond) == []
    cs = dict(kind="ln", rows=4, c=2, beta=True, res=False, gres=False, gxhat=True, accumulate=0, seed=7)
    ref, cond = R.case_reference(cs, R.case_tensors(cs))
    assert any(b[0] == "dst" for b in R.rule_misses(cs, ref, cond)), "two channels without gres: dL/dx is of order eps"
