"""Float64 references, seeded case generators and guarded device buffers for the geometry tests of the GroupNorm / LayerNorm
kernels (tests/test_hip_norm_geometry.py; the references, the generators' promises and the conditioning rule are checked on the
CPU by tests/test_norm_refs_cpu.py).  A plain module: nothing here is collected by pytest and nothing touches the GPU on import.

Layouts are the kernels': activations channel-last, x [n, h, w, c] (forward-only cases: h = hw, w = 1), per-channel sums
[n, c, 2] = (sum, sum of squares), partial tables [n, parts, 2, c], FiLM rows [n, film_ld] with the scale at +0 and the shift at +c.

The conditioning rule.  A tolerance only means something where the operation itself is well conditioned in fp32.  Every case of
a sweep is therefore admitted by the generator only if
  (1) the reference's own arithmetic in fp32 -- torch's CPU group_norm / layer_norm, fp32 autograd for the backward chains, an
      fp32 sum for the statistics, the coefficient formula in fp32 for the partial tables, which have no torch operator -- is
      within ONE QUARTER of the tolerance the GPU test applies (TOL), and
  (2) GroupNorm only: every group has |mean| / sqrt(var + eps) <= R_MAX = 4.  The kernels form the variance in one pass,
      ss / cnt - mean^2, from sums rounded to float; the relative error of rstd that one rounding of each sum leaves is at most
      2^-25 (1 + 3 r^2) (offset_bound), 1.5e-6 at r = 4 and beyond every tolerance here from r ~ 16 on.  torch's two-pass
      arithmetic does not see r, so (1) alone would admit cases the one-pass form cannot hold; what happens above 4 is measured,
      not asserted, by the "offset" family.  A group that is exactly constant at 0 or 0.25 is exempt: its lane sums, sums and
      variance are exact in fp32 (multiples of 2^-4 far below 2^24).
A case that misses the rule is redrawn (a new tensor seed, the geometry stays), so a sweep keeps its size; the CPU test asserts
that no case of the final lists misses it.
"""
import functools
import random

import torch
import torch.nn.functional as F

EPS = 1e-5
RS_NONE, RS_AVGPOOL2, RS_UP2 = 0, 1, 2
R_MAX = 4.0
# the project's standing tolerances (max |a - b| / max |b|), now against float64
TOL = dict(sums=2e-6,        # test_hip_kernels.test_stem_conv_narrow_kernel: of the largest exact sum
           fold=1e-6,        # test_groupnorm_coefficients_from_partial_statistics: folded sums, and one launch against two
           affine=5e-6,      # test_groupnorm_coefficients: a * x + b (partial tables, which have no x: a and b themselves)
           ln_fwd=2e-6,      # test_layernorm: output, mean, rstd
           gn_bwd=2e-5,      # test_groupnorm_silu_backward: dx, dgamma, dbeta, dfilm
           ln_bwd=2e-5)      # test_layernorm_backward: dx, g * xhat and its column sum


def max_rel(a, b):
    """conftest.max_rel (this module imports no conftest)"""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# references (float64 on the fp32 inputs)
# ---------------------------------------------------------------------------------------------------------------------
def ref_chan_sums(x):
    """x [n, hw, c] -> [n, c, 2] = (sum, sum of squares) over the rows"""
    x = x.double()
    return torch.stack([x.sum(1), (x * x).sum(1)], -1)


def ref_fold(partial):
    """partial [n, parts, 2, c] -> [n, c, 2]"""
    return partial.double().sum(1).transpose(1, 2).contiguous()


def ref_group_stats(x, groups):
    """x [n, hw, c] -> (mean, var), each [n, c] (a group's value repeated over its channels), two passes"""
    n, hw, c = x.shape
    xg = x.double().reshape(n, hw, groups, c // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    rep = lambda t: t.expand(n, 1, groups, c // groups).reshape(n, c)
    return rep(mean), rep(var)


def ref_stats_from_sums(sums, groups, hw):
    """sums [n, c, 2] float64 -> (mean, var) [n, c] (one pass, in float64)"""
    n, c, _ = sums.shape
    sg = sums.double().reshape(n, groups, c // groups, 2).sum(2)
    cnt = float(c // groups * hw)
    mean = sg[..., 0] / cnt
    var = (sg[..., 1] / cnt - mean * mean).clamp_min(0.0)
    rep = lambda t: t[:, :, None].expand(n, groups, c // groups).reshape(n, c)
    return rep(mean), rep(var)


def ref_gn_coef(mean, var, gamma, beta, film=None, eps=EPS):
    """(a, b) [n, c] with GN(x) * (1 + scale) + shift == a * x + b; film [n, >= 2 c] or None"""
    c = gamma.numel()
    a = gamma.double()[None] / torch.sqrt(var + eps)
    b = beta.double()[None] - mean * a
    if film is not None:
        sc, sh = 1.0 + film.double()[:, :c], film.double()[:, c:2 * c]
        a, b = a * sc, b * sc + sh
    return a, b


def ref_group_norm(x, groups, gamma, beta, film=None, eps=EPS):
    """x [n, hw, c] -> GN(x) (* (1 + scale) + shift), [n, hw, c]"""
    a, b = ref_gn_coef(*ref_group_stats(x, groups), gamma, beta, film, eps)
    return x.double() * a[:, None] + b[:, None]


def resampled(t, mode):
    """[n, c, h, w] through the forward resample of a mode"""
    if mode == RS_AVGPOOL2:
        return F.avg_pool2d(t, 2)
    if mode == RS_UP2:
        return F.interpolate(t, scale_factor=2, mode="nearest")
    return t


def resampled_hw(h, w, mode):
    return {RS_NONE: (h, w), RS_AVGPOOL2: (h // 2, w // 2), RS_UP2: (2 * h, 2 * w)}[mode]


def _gn_own(x, groups, gamma, beta, eps):
    n, c, h, w = x.shape
    xg = x.reshape(n, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(-1, keepdim=True)
    return ((xg - mean) / torch.sqrt(var + eps)).reshape(n, c, h, w) * gamma[None, :, None, None] + beta[None, :, None, None]


def ref_gn_backward(x, groups, gamma, beta, film, silu, keep, drop_p, gu, gu_mode, gres, gres_mode, eps=EPS,
                    dtype=torch.float64, torch_norm=False):
    """autograd (float64) of  sum(gu * R_u(drop(act(GN(x) (+FiLM))))) + sum(gres * R_r(x)):
    x [n, h, w, c]; keep: bool [n, h, w, c] or None (the kernels' dropout keep mask, supplied by the caller: kept elements are
    scaled by 1 / (1 - drop_p)); gu / gres [n, h', w', c] at the resolution of their mode; gres may be None.
    -> dict(dx [n, h, w, c], dgamma [c], dbeta [c], dfilm [n, 2 c] or None).  dtype float32 with torch_norm: the same chain in
    torch's fp32 arithmetic (the conditioning rule)."""
    c = x.shape[-1]
    nchw = lambda t: t.to(dtype).permute(0, 3, 1, 2)
    xx = nchw(x).detach().clone().requires_grad_(True)
    gam, bet = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    leaves = [xx, gam, bet]
    y = F.group_norm(xx, groups, gam, bet, eps) if torch_norm else _gn_own(xx, groups, gam, bet, eps)
    fl = None
    if film is not None:
        fl = film[:, :2 * c].to(dtype).clone().requires_grad_(True)
        leaves.append(fl)
        y = y * (1 + fl[:, :c, None, None]) + fl[:, c:, None, None]
    u = F.silu(y) if silu else y
    if keep is not None and drop_p > 0:
        u = u * nchw(keep) / (1.0 - drop_p)
    loss = (resampled(u, gu_mode) * nchw(gu)).sum()
    if gres is not None:
        loss = loss + (resampled(xx, gres_mode) * nchw(gres)).sum()
    loss.backward()
    return dict(dx=xx.grad.permute(0, 2, 3, 1).double(), dgamma=gam.grad.double(), dbeta=bet.grad.double(),
                dfilm=None if fl is None else fl.grad.double())


def ref_ln_stats(x, eps=EPS):
    """x [rows, c] -> (mean [rows], rstd [rows])"""
    x = x.double()
    mean = x.mean(1)
    return mean, 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + eps)


def ref_ln_apply(x, gamma, beta=None, res=None, eps=EPS):
    """(res or 0) + LN(x) * gamma + (beta or 0)"""
    mean, rstd = ref_ln_stats(x, eps)
    y = (x.double() - mean[:, None]) * rstd[:, None] * gamma.double()[None]
    if beta is not None:
        y = y + beta.double()[None]
    return y if res is None else y + res.double()


def ref_ln_backward(x, g, gamma, gres=None, base=None, eps=EPS):
    """g = dL/dy of y = xhat * gamma + beta -> dict(dst = (base or 0) + dL/dx (+ gres), gxhat = g * xhat [rows, c])"""
    mean, rstd = ref_ln_stats(x, eps)
    xhat = (x.double() - mean[:, None]) * rstd[:, None]
    gw = g.double() * gamma.double()[None]
    dx = rstd[:, None] * (gw - gw.mean(1, keepdim=True) - xhat * (gw * xhat).mean(1, keepdim=True))
    if gres is not None:
        dx = dx + gres.double()
    if base is not None:
        dx = dx + base.double()
    return dict(dst=dx, gxhat=g.double() * xhat)


def offset_bound(r):
    """a-priori relative error of rstd from one rounding to float of each of the two sums of a one-pass variance"""
    return 2.0 ** -25 * (1.0 + 3.0 * r * r)


def group_offset_ratio(x, groups, skip_group=None, eps=EPS):
    """largest |mean| / sqrt(var + eps) over the groups of x [n, hw, c] (skip_group: the exactly constant group of a
    degenerate case)"""
    n, hw, c = x.shape
    mean, var = ref_group_stats(x, groups)
    r = mean.abs() / torch.sqrt(var + eps)
    if skip_group is not None:
        cpg = c // groups
        r[:, skip_group * cpg:(skip_group + 1) * cpg] = 0.0
    return float(r.max())


def reduce_trips(hw):
    """{(trips of the four-pixels-in-flight loop, trips of the tail loop)} over the 32 row lanes of gn_bwd_reduce_kernel with a
    same-resolution gradient: lane p0 runs `for (; p + 96 < hw; p += 128)`, then `for (; p < hw; p += 32)`"""
    out = set()
    for p in range(32):
        wide = 0
        while p + 96 < hw:
            p, wide = p + 128, wide + 1
        out.add((wide, len(range(p, hw, 32))))
    return out


def fold_trips(parts, c):
    """{(8-wide trips, 4-wide trips, scalar trips)} over the thread groups of gn_coef_parts_kernel folding `parts` partials of
    a c-channel GroupNorm: G = 512 // c groups (1 from 512 channels on), group j takes parts j, j + G, ..."""
    G = 512 // c if c < 512 else 1
    out = set()
    for grp in range(G):
        cnt = len(range(grp, parts, G))
        out.add((cnt // 8, (cnt % 8) // 4, cnt % 4))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
CS_C = (1, 3, 4, 6, 30, 32, 33, 36, 64, 96, 100, 224)          # chan_stats: both branches, ragged slabs, several slabs
CS_HW = (1, 5, 31, 32, 33, 64, 100, 1024)                      # below / at / above the 32 row lanes, many rows per lane
CS_OFF = (0, 1, 3, 4, 7, 8)
PARTS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 31, 32, 33, 40, 128)
PARTS_C0 = (32, 64, 96, 128, 160, 256, 512, 544, 1024)
PARTS_C1 = (0, 32, 96, 128)
FWD_GROUPS = (1, 8, 32)
FWD_CPG = (1, 2, 3, 4, 7, 8, 32)
BWD_HW = ((1, 1), (2, 2), (3, 5), (6, 10), (8, 12), (8, 16), (12, 12), (16, 16))
BWD_C = (4, 32, 36, 96, 128)
BWD_OFF = (0, 32, 36)
BWD_MODE_PAIRS = tuple((u, r) for u in (0, 1, 2) for r in (0, 1, 2, None))      # (gu_mode, gres_mode; None: no gres)
DROPS = (0.0, 0.1, 0.25)
LN_ROWS = (1, 3, 4, 5, 37)
LN_C = (1, 2, 63, 64, 65, 100, 320, 1000, 1023, 1024)
OFFSET_R = (0, 2, 4, 16, 32, 128)
OFFSET_HW = (16, 4096)


def _spread(rnd, values, count):
    """`count` draws from `values` in which every value appears (count >= len(values)), in random order"""
    assert count >= len(values), (count, values)
    out = list(values) + [rnd.choice(values) for _ in range(count - len(values))]
    rnd.shuffle(out)
    return out


def chan_stats_cases(rnd, count=24):
    """sgd_chan_stats: every c of CS_C (c % 4 != 0: the scalar branch), every hw of CS_HW, n in 1..3, every channel offset of
    CS_OFF (odd ones included) into a sums table wider than c_off + c"""
    cases = [dict(kind="chan_stats") for _ in range(count)]
    for key, values in (("c", CS_C), ("hw", CS_HW), ("n", (1, 2, 3)), ("c_off", CS_OFF)):
        for cs, val in zip(cases, _spread(rnd, values, count)):
            cs[key] = val
    for cs in cases:
        cs["c_total"] = cs["c_off"] + cs["c"] + rnd.randrange(1, 6)
    return cases


def parts_cases(rnd, count=28):
    """sgd_stats_reduce / sgd_gn_coef_parts on synthetic partial tables: every part count of PARTS for source 0, every c0 of
    PARTS_C0, every c1 of PARTS_C1 (c1 > 0: parts1 from PARTS, or 0 = sums pre-written by sgd_chan_stats), 96 and 160 channels
    alone (G = 512 // c thread groups with a remainder), FiLM on and off with film_ld > 2 c; and, last, the raised dynamic-LDS
    launch n = 1, c = 4096, parts = 2"""
    cases = [dict(kind="parts", groups=32) for _ in range(count)]
    for key, values in (("parts0", PARTS), ("c0", PARTS_C0), ("n", (1, 2)), ("film", (False, True))):
        for cs, val in zip(cases, _spread(rnd, values, count)):
            cs[key] = val
    alone = [next(i for i, cs in enumerate(cases) if cs["c0"] == c) for c in (96, 160)]
    rest = [i for i in range(count) if i not in alone]
    for i, val in zip(rest, _spread(rnd, PARTS_C1, len(rest))):
        cases[i]["c1"] = val
    for i in alone:
        cases[i]["c1"] = 0
    two = [cs for cs in cases if cs["c1"] > 0]
    for cs, val in zip(two, _spread(rnd, (0, 0, 1, 3, 5, 8, 12, 33), len(two))):
        cs["parts1"] = val
    for cs in cases:
        cs.setdefault("parts1", 0)
    cases.append(dict(kind="parts", groups=32, parts0=2, c0=4096, n=1, film=False, c1=0, parts1=0))
    for cs in cases:
        c = cs["c0"] + cs["c1"]
        cs["film_ld"] = 2 * c + rnd.choice((4, 8))
        cs["hw"] = 4 * max(cs["parts0"], cs["parts1"]) + rnd.randrange(0, 9)
    return cases


def forward_cases(rnd, count=24):
    """sgd_chan_stats -> sgd_gn_coef -> a x + b: every group count of FWD_GROUPS, every channels-per-group of FWD_CPG, every hw
    of CS_HW (a group of one element has no variance to normalise by: r is infinite, hw is redrawn), n in 1..2, FiLM on and
    off; from three channels on, a virtual concat of two sources with unequal channel counts at an arbitrary channel offset"""
    cases = [dict(kind="gn", w=1) for _ in range(count)]
    for key, values in (("groups", FWD_GROUPS), ("cpg", FWD_CPG), ("h", CS_HW), ("n", (1, 2)), ("film", (False, True))):
        for cs, val in zip(cases, _spread(rnd, values, count)):
            cs[key] = val
    for cs in cases:
        c = cs["groups"] * cs.pop("cpg")
        if c // cs["groups"] * cs["h"] == 1:
            cs["h"] = 5
        if c >= 3:
            c0 = rnd.choice([k for k in range(1, c) if 2 * k != c])
            cs["srcs"] = (c0, c - c0)
        else:
            cs["srcs"] = (c,)
        cs["film_ld"] = 2 * c + rnd.choice((4, 8))
    return cases


def backward_cases(rnd, count=28):
    """chan_stats -> gn_coef -> gn_bwd_reduce -> gn_bwd_coef -> gn_bwd_apply: every (h, w) of BWD_HW (hw on both sides of 96 and
    128: the four-pixels-in-flight loop of the reduce takes 0 trips, 1 trip, 1 trip and a tail), every c of BWD_C, alone or
    behind a first source of 32 or 36 channels, every (gu_mode, gres_mode / no gres) pair of BWD_MODE_PAIRS (odd h or w: without
    the pooled mode), padded gu / gres / dst row strides, dst_off 0 and 4, accumulate, SiLU, FiLM, every dropout rate of DROPS;
    and, last, the two smallest shapes the row-stream reduce serves (n = 1, 32 x 32, c 16 and 64)"""
    cases = [dict(kind="gn") for _ in range(count)]
    for key, values in (("hw", BWD_HW), ("c", BWD_C), ("c_off", BWD_OFF), ("n", (1, 2)), ("silu", (0, 1)), ("film", (False, True)),
                        ("drop_p", DROPS), ("accumulate", (0, 1)), ("dst_off", (0, 4))):
        for cs, val in zip(cases, _spread(rnd, values, count)):
            cs[key] = val
    for hw in ((8, 16), (12, 12), (16, 16)):     # the unrolled loop of the reduce serves the same-resolution gradient only
        pinned = next(cs for cs in cases if cs["hw"] == hw)
        pinned["gu_mode"], pinned["gres_mode"] = RS_NONE, rnd.choice((RS_NONE, RS_AVGPOOL2, RS_UP2, None))
    even = [cs for cs in cases if not (cs["hw"][0] | cs["hw"][1]) & 1 and "gu_mode" not in cs]
    for cs, val in zip(even, _spread(rnd, BWD_MODE_PAIRS, len(even))):
        cs["gu_mode"], cs["gres_mode"] = val
    for cs in cases:
        if "gu_mode" not in cs:
            cs["gu_mode"], cs["gres_mode"] = rnd.choice([p for p in BWD_MODE_PAIRS if RS_AVGPOOL2 not in p])
    for c in (16, 64):
        cases.append(dict(kind="gn", hw=(32, 32), c=c, c_off=0, n=1, silu=1, film=c == 64, drop_p=0.1 if c == 16 else 0.0,
                          accumulate=0, dst_off=0, gu_mode=RS_NONE, gres_mode=RS_NONE if c == 16 else None, rows=True))
    for cs in cases:
        cs["h"], cs["w"] = cs.pop("hw")
        c, off = cs.pop("c"), cs.pop("c_off")
        cs["srcs"] = (off, c) if off else (c,)
        ct = off + c
        cs["groups"] = rnd.choice([g for g in (1, 2, 4, 8, 32) if ct % g == 0 and ct // g * cs["h"] * cs["w"] >= 2])
        cs["film_ld"] = 2 * ct + rnd.choice((4, 8))
        cs["gu_ld"], cs["gres_ld"], cs["dst_pad"] = ct + rnd.choice((4, 8)), ct + rnd.choice((4, 12)), rnd.choice((4, 8))
        cs["drop_seed"] = rnd.randrange(1 << 31)
        cs.setdefault("rows", False)
    return cases


def degenerate_cases(rnd):
    """GroupNorm chains (forward and backward) in which ONE group is exactly constant over the whole image -- 0.0, what a
    zero_module conv puts out at initialisation, or 0.25 -- and the others are random: the `var < 0 -> 0` clamp, rstd =
    1 / sqrt(eps)"""
    cases = []
    for value in (0.0, 0.25):
        for (h, w), srcs, groups, grp, silu, film in (((8, 8), (64,), 32, 5, 1, False), ((6, 10), (32, 4), 4, 3, 0, True),
                                                      ((16, 16), (128,), 32, 31, 1, True)):
            ct = sum(srcs)
            cases.append(dict(kind="gn", n=2, h=h, w=w, srcs=srcs, groups=groups, silu=silu, film=film, drop_p=0.0,
                              accumulate=0, dst_off=0, gu_mode=RS_NONE, gres_mode=None, rows=False, film_ld=2 * ct + 4,
                              gu_ld=ct + 4, gres_ld=ct + 4, dst_pad=4, drop_seed=0, degenerate=(value, grp)))
    return cases


def offset_cases(rnd):
    """GroupNorm forward on x = mu + sigma randn, r = |mu| / sigma over OFFSET_R x OFFSET_HW (32 channels in 8 groups)"""
    return [dict(kind="gn", n=1, h=hw, w=1, srcs=(32,), groups=8, film=False, film_ld=0, mu=float(r), sigma=1.0, r=r)
            for r in OFFSET_R for hw in OFFSET_HW]


def layernorm_cases(rnd, count=24):
    """sgd_ln_stats / sgd_ln_apply / sgd_ln_bwd: every row count of LN_ROWS (a ragged last block of four rows), every c of LN_C
    (one lane, a ragged last 64-lane group, the 1024-channel limit), beta / res / gres / gxhat each present and NULL, plain
    and accumulating.  One channel: dL/dx is identically zero; two: xhat = +-1 and dL/dx is a difference of order eps.  Neither has
    a maximum of its own to measure an error against, so gres is always present there"""
    cases = [dict(kind="ln") for _ in range(count)]
    for key, values in (("rows", LN_ROWS), ("c", LN_C), ("beta", (False, True)), ("res", (False, True)), ("gres", (False, True)),
                        ("gxhat", (False, True)), ("accumulate", (0, 1))):
        for cs, val in zip(cases, _spread(rnd, values, count)):
            cs[key] = val
    for cs in cases:
        if cs["c"] <= 2:
            cs["gres"] = True
    return cases


def ln_degenerate_cases(rnd):
    """LayerNorm rows that are exactly constant (row 1 of each case): rstd = 1 / sqrt(eps), out = beta + res"""
    return [dict(kind="ln", rows=3, c=c, beta=True, res=True, gres=True, gxhat=True, accumulate=0, constant_row=(1, v))
            for c, v in ((64, 0.0), (100, 0.25), (1024, 0.25))]


SWEEPS = {"chan_stats": (chan_stats_cases, 20261101), "parts": (parts_cases, 20261102), "forward": (forward_cases, 20261103),
          "backward": (backward_cases, 20261104), "layernorm": (layernorm_cases, 20261105),
          "degenerate": (degenerate_cases, 20261106), "ln_degenerate": (ln_degenerate_cases, 20261107),
          "offset": (offset_cases, 20261108)}
MAX_DRAWS = 200
REDRAWS = {}                     # {(sweep, part of the rule): draws it rejected}, filled by sweep_reference


# ---------------------------------------------------------------------------------------------------------------------
# tensors and references of a case
# ---------------------------------------------------------------------------------------------------------------------
def case_tensors(cs):
    """fp32 CPU inputs of a case, from cs["seed"] alone"""
    g = torch.Generator().manual_seed(cs["seed"])
    rn = lambda *shape: torch.randn(*shape, generator=g)
    if cs["kind"] == "chan_stats":
        return dict(x=rn(cs["n"], cs["hw"], cs["c"]) * 2 + 0.3)
    if cs["kind"] == "parts":
        n, hw, c = cs["n"], cs["hw"], cs["c0"] + cs["c1"]
        t = dict(gamma=rn(c), beta=rn(c), film=rn(n, cs["film_ld"]) if cs["film"] else None, p1=None, x1=None)
        for key, parts, cc in (("p0", cs["parts0"], cs["c0"]), ("p1", cs["parts1"], cs["c1"])):
            if parts == 0:
                continue
            # the statistics of `parts` row ranges of uneven length: range k holds cnt_k rows of mean m and variance v
            cuts = sorted(torch.randperm(hw - 1, generator=g)[:parts - 1].add(1).tolist()) if parts > 1 else []
            cnt = torch.tensor([b - a for a, b in zip([0] + cuts, cuts + [hw])], dtype=torch.float64)[None, :, None]
            m = 0.4 + 0.5 * rn(n, parts, cc).double()
            v = 0.5 + torch.rand(n, parts, cc, generator=g).double()
            t[key] = torch.stack([cnt * m, cnt * (v + m * m)], 2).float()
        if cs["c1"] > 0 and cs["parts1"] == 0:
            t["x1"] = rn(n, hw, cs["c1"]) * 1.2 + 0.4
        return t
    if cs["kind"] == "gn":
        n, h, w, ct = cs["n"], cs["h"], cs["w"], sum(cs["srcs"])
        x = cs.get("mu", 0.3) + cs.get("sigma", 2.0) * rn(n, h, w, ct)
        if cs.get("degenerate"):
            value, grp = cs["degenerate"]
            cpg = ct // cs["groups"]
            x[..., grp * cpg:(grp + 1) * cpg] = value
        t = dict(x=x, gamma=rn(ct), beta=rn(ct), film=rn(n, cs["film_ld"]) if cs["film"] else None)
        if "gu_mode" in cs:
            t["gu"] = rn(n, *resampled_hw(h, w, cs["gu_mode"]), ct)
            t["gres"] = rn(n, *resampled_hw(h, w, cs["gres_mode"]), ct) if cs["gres_mode"] is not None else None
            t["base"] = rn(n, h, w, ct) if cs["accumulate"] else None
        return t
    if cs["kind"] == "ln":
        rows, c = cs["rows"], cs["c"]
        x = rn(rows, c) * 3 + 1
        if cs.get("constant_row"):
            x[cs["constant_row"][0]] = cs["constant_row"][1]
        return dict(x=x, gamma=rn(c), beta=rn(c) if cs["beta"] else None, res=rn(rows, c) if cs["res"] else None, g=rn(rows, c),
                    gres=rn(rows, c) if cs["gres"] else None, base=rn(rows, c) if cs["accumulate"] else None)
    raise ValueError(cs["kind"])


def case_keep_mask(cs):
    """the kernels' dropout keep mask of a GroupNorm-backward case, bool [n, h, w, c] over the concatenated tensor, or None:
    the host restatement of the device hash (numpy, no device)"""
    if not cs.get("drop_p"):
        return None
    from test_hip_train import _host_keep_mask
    n, h, w, ct = cs["n"], cs["h"], cs["w"], sum(cs["srcs"])
    return torch.from_numpy(_host_keep_mask(cs["drop_seed"], n * h * w, ct, cs["drop_p"])).reshape(n, h, w, ct)


def _gn_backward_of(cs, t, keep, **kw):
    film = t["film"][:, :2 * sum(cs["srcs"])] if t["film"] is not None else None
    return ref_gn_backward(t["x"], cs["groups"], t["gamma"], t["beta"], film, cs["silu"], keep, cs["drop_p"], t["gu"],
                           cs["gu_mode"], t["gres"], cs["gres_mode"], **kw)


def case_reference(cs, t):
    """(float64 results, {quantity: (fp32-arithmetic error, tolerance)}) of a case; GroupNorm: also "r", the largest group
    offset ratio"""
    ref, cond = {}, {}
    if cs["kind"] == "chan_stats":
        ref["sums"] = ref_chan_sums(t["x"])
        x = t["x"]
        f32 = torch.stack([x.sum(1), (x * x).sum(1)], -1)
        for k, nm in enumerate(("sum", "sumsq")):
            cond[nm] = (max_rel(f32[..., k], ref["sums"][..., k]), TOL["sums"])
    elif cs["kind"] == "parts":
        c0, hw = cs["c0"], cs["hw"]
        srcs = [ref_fold(t["p0"])]
        f32 = [t["p0"].sum(1).transpose(1, 2)]
        if cs["c1"] > 0:
            srcs.append(ref_fold(t["p1"]) if cs["parts1"] else ref_chan_sums(t["x1"]))
            x1 = t["x1"]
            f32.append(t["p1"].sum(1).transpose(1, 2) if cs["parts1"] else torch.stack([x1.sum(1), (x1 * x1).sum(1)], -1))
        ref["sums"] = torch.cat(srcs, 1)
        ref["a"], ref["b"] = ref_gn_coef(*ref_stats_from_sums(ref["sums"], cs["groups"], hw), t["gamma"], t["beta"], t["film"])
        s32 = torch.cat(f32, 1)
        cond["sums"] = (max_rel(s32, ref["sums"]), TOL["fold"])
        # the coefficient formula in fp32 on the fp32 sums (no torch operator takes a partial table)
        n, c = s32.shape[:2]
        sg = s32.reshape(n, cs["groups"], c // cs["groups"], 2).sum(2)
        cnt = torch.tensor(float(c // cs["groups"] * hw))
        mean = sg[..., 0] / cnt
        rstd = 1.0 / torch.sqrt((sg[..., 1] / cnt - mean * mean).clamp_min(0) + EPS)
        rep = lambda u: u[:, :, None].expand(n, cs["groups"], c // cs["groups"]).reshape(n, c)
        a32 = t["gamma"][None] * rep(rstd)
        b32 = t["beta"][None] - rep(mean) * a32
        if cs["film"]:
            a32, b32 = a32 * (1 + t["film"][:, :c]), b32 * (1 + t["film"][:, :c]) + t["film"][:, c:2 * c]
        cond["a"], cond["b"] = (max_rel(a32, ref["a"]), TOL["affine"]), (max_rel(b32, ref["b"]), TOL["affine"])
    elif cs["kind"] == "gn":
        n, h, w, ct = cs["n"], cs["h"], cs["w"], sum(cs["srcs"])
        x3 = t["x"].reshape(n, h * w, ct)
        film = t["film"][:, :2 * ct] if t["film"] is not None else None
        ref["sums"] = ref_chan_sums(x3)
        ref["a"], ref["b"] = ref_gn_coef(*ref_group_stats(x3, cs["groups"]), t["gamma"], t["beta"], film)
        ref["y"] = x3.double() * ref["a"][:, None] + ref["b"][:, None]
        y32 = F.group_norm(x3.transpose(1, 2), cs["groups"], t["gamma"], t["beta"], EPS)
        if film is not None:
            y32 = y32 * (1 + film[:, :ct, None]) + film[:, ct:, None]
        cond["y"] = (max_rel(y32.transpose(1, 2), ref["y"]), TOL["affine"])
        skip = cs["degenerate"][1] if cs.get("degenerate") else None
        ref["r"] = group_offset_ratio(x3, cs["groups"], skip)
        if "gu_mode" in cs:
            keep = case_keep_mask(cs)
            ref.update(_gn_backward_of(cs, t, keep))
            f32 = _gn_backward_of(cs, t, keep, dtype=torch.float32, torch_norm=True)
            for nm in ("dx", "dgamma", "dbeta", "dfilm"):
                if ref[nm] is not None:
                    cond[nm] = (max_rel(f32[nm], ref[nm]), TOL["gn_bwd"])
    elif cs["kind"] == "ln":
        x, c = t["x"], cs["c"]
        ref["mean"], ref["rstd"] = ref_ln_stats(x)
        ref["out"] = ref_ln_apply(x, t["gamma"], t["beta"], t["res"])
        ref.update(ref_ln_backward(x, t["g"], t["gamma"], t["gres"], t["base"]))
        xx = x.clone().requires_grad_(True)
        y32 = F.layer_norm(xx, (c,), t["gamma"], t["beta"], EPS)
        y32.backward(t["g"])
        dst32 = xx.grad + (t["gres"] if t["gres"] is not None else 0) + (t["base"] if t["base"] is not None else 0)
        out32 = y32.detach() + (t["res"] if t["res"] is not None else 0)
        gx32 = t["g"] * F.layer_norm(x, (c,), None, None, EPS)
        cond["out"] = (max_rel(out32, ref["out"]), TOL["ln_fwd"])
        cond["mean"] = (max_rel(x.mean(1), ref["mean"]), TOL["ln_fwd"])
        cond["rstd"] = (max_rel(1.0 / torch.sqrt(x.var(1, unbiased=False) + EPS), ref["rstd"]), TOL["ln_fwd"])
        cond["dst"] = (max_rel(dst32, ref["dst"]), TOL["ln_bwd"])
        cond["gxhat"] = (max_rel(gx32, ref["gxhat"]), TOL["ln_bwd"])
        cond["dgamma"] = (max_rel(gx32.sum(0), ref["gxhat"].sum(0)), TOL["ln_bwd"])
    return ref, cond


def rule_misses(cs, ref, cond):
    """what of the conditioning rule (module docstring) a case misses ([] = admitted).  The offset family is the one exception:
    it has its own bound (offset_bound) and is measured, not admitted."""
    if "r" in cs:
        return []
    bad = [(nm, err, tol) for nm, (err, tol) in cond.items() if not err <= tol / 4]
    if cs["kind"] == "gn" and not ref["r"] <= R_MAX:
        bad.append(("group offset ratio", ref["r"], R_MAX))
    return bad


@functools.lru_cache(maxsize=None)
def sweep_reference(name):
    """[(case, inputs, float64 results, conditioning figures)] of a sweep, computed once and shared by the tests that use it
    (never modified).  The geometry comes from random.Random(seed of the sweep); each case carries its own tensor seed, redrawn
    until the case meets the conditioning rule."""
    make, seed = SWEEPS[name]
    rnd = random.Random(seed)
    out = []
    for cs in make(rnd):
        for _ in range(MAX_DRAWS):
            cs["seed"] = rnd.randrange(1 << 30)
            t = case_tensors(cs)
            ref, cond = case_reference(cs, t)
            missed = rule_misses(cs, ref, cond)
            if not missed:
                break
            for m in missed:                 # how often each part of the rule asked for a new draw
                key = (name, "offset ratio" if m[0] == "group offset ratio" else "fp32 arithmetic")
                REDRAWS[key] = REDRAWS.get(key, 0) + 1
        else:
            raise RuntimeError(f"sweep {name}: no draw of {cs} meets the conditioning rule")
        out.append((cs, t, ref, cond))
    return out


def sweep_cases(name):
    """the case dicts of a sweep (plain dicts; copies)"""
    return [dict(cs) for cs, _, _, _ in sweep_reference(name)]


# ---------------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ---------------------------------------------------------------------------------------------------------------------
GUARD_BITS = 0x7FC5A5A5          # a quiet NaN no arithmetic produces


class Guarded:
    """A device output of `rows` rows with row stride `ld` floats of which the kernel owns columns [col0, col0 + cols),
    allocated with one guard row in front and BEHIND = 3 behind (the spare waves of a last block of four rows each have a row to
    be caught in) and prefilled, guards, padding and owned region alike, with GUARD_BITS (a NaN).  fill() puts the base of an accumulating launch into the owned region.  After the launch owned() is
    the owned region (CPU, [rows, cols]), untouched() says whether every word outside it still holds the pattern (compared as
    int32: NaN != NaN as floats) and written() whether none inside it does."""

    BEHIND = 3

    def __init__(self, rows, ld, cols=None, col0=0, device="cuda"):
        self.rows, self.ld, self.col0 = rows, ld, col0
        self.cols = ld - col0 if cols is None else cols
        assert self.cols > 0 and col0 + self.cols <= ld
        self.bits = torch.full(((rows + 1 + self.BEHIND) * ld,), GUARD_BITS, dtype=torch.int32, device=device)

    @property
    def ptr(self):
        """address of row 0, column 0 (the guard row in front ends here)"""
        return self.bits.data_ptr() + 4 * self.ld

    def tensor(self):
        return self.bits.view(torch.float32)[self.ld:(self.rows + 1) * self.ld].view(self.rows, self.ld)

    def fill(self, base):
        self.tensor()[:, self.col0:self.col0 + self.cols] = base.reshape(self.rows, self.cols).to(self.bits.device)

    def owned(self):
        return self.tensor()[:, self.col0:self.col0 + self.cols].cpu()

    def _mask(self):
        own = torch.zeros(self.rows + 1 + self.BEHIND, self.ld, dtype=torch.bool)
        own[1:self.rows + 1, self.col0:self.col0 + self.cols] = True
        return own

    def untouched(self):
        bits = self.bits.cpu().view(self.rows + 1 + self.BEHIND, self.ld)
        return bool((bits[~self._mask()] == GUARD_BITS).all())

    def written(self):
        bits = self.bits.cpu().view(self.rows + 1 + self.BEHIND, self.ld)
        return not bool((bits[self._mask()] == GUARD_BITS).any())


def padded(t, ld):
    """[..., c] -> [..., ld] with NaN in the padding columns (an input's padding must never be read)"""
    out = torch.full((*t.shape[:-1], ld), float("nan"), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out
