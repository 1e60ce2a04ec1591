"""Learned variance on the HIP path (hparam learn_sigma; Nichol & Dhariwal 2021): the hybrid-loss kernels (csrc/lvloss.hip:
sgd_lv_loss_fwd / sgd_lv_loss_bwd), the 2C-wide output head forward and backward, the ancestral update (csrc/lvstep.hip:
sgd_ddpm_lv_step), strided 'native' trajectories (sampling kwarg native_steps), the other samplers on a C-row head, and
calc_bpd.  The reference has none of this; the expected values are the formulas restated here -- float64 over the same fp32
inputs, torch fp32 in the kernels' documented operation order where the gate is bit-equality or an error budget -- and the
project's own kernels (sgd_loss_fwd / sgd_loss_bwd on the mean half).  GPU only; every test prints the figures it asserts on
(run with -s).

Bounds.  Per-sample values 1e-6 relative and gradients 1e-5 rel-L2 against float64, as tests/test_hip_loss_weighting.py; the
t > 0 term of the bound is an fp32 expression that cancels where lv ~ lq, so its error is held to the larger of those bounds and
4x the error of the torch-fp32 restatement (same operation order, on the device) against float64 on the same inputs; the
t == 0 term runs in double and meets the plain bounds alone.  Forward against the oracle 1e-4 (the parity contract), parameter
gradients 1e-4 max-rel, teacher-forced trajectories 1e-5 rel-L2 (tests/test_hip_ztsnr.py).

Measured on the MI355X: simple term bit-equal to sgd_loss_fwd / sgd_loss_bwd; t == 0: per_vlb 4.5e-8, gradient 3.2e-8 rel-L2 from
float64; t > 0, worst case kernel / restatement / bound: per_vlb 7.3e-4 / 7.3e-4 / 2.9e-3 (plain), 3.7e-2 / 3.7e-2 / 1.5e-1
(zero-terminal), gradient 5.3e-3 / 5.3e-3 / 2.1e-2 and 1.6e-1 / 1.6e-1 / 6.2e-1 -- all of it at T-1, where max_log - min_log is
1.5e-5 / 8e-8 and the variance part of the bound is below one fp32 rounding of its terms; step kernel bit-equal to torch fp32
(the device's expf is torch's); 6-wide head forward 3.0e-6 from the oracle; training loss 1.1e-7, gradients 1.6e-6 (both parameterizations
in f32 and f16x3); strided native trajectories at most 5.4e-7 worst step, pred_x0 4.7e-6 ('v' on the eps form at T-1) (DESIGN.md
section 7)."""
import math

import numpy as np
import pytest
import torch

from conftest import max_rel, rel_l2

pytestmark = pytest.mark.gpu

T, S, B, W = 1000, 16, 2, 2.0
LN2 = math.log(2.0)
PARS, KINDS = ("eps", "x0", "v"), ("l2", "l1", "huber")
TS = (0, 1, 241, T - 1)


class _AD(dict):
    __getattr__ = dict.__getitem__


def _diffusion(**kw):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, **kw))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _count(monkeypatch, *names):
    """call counters on entries of the loaded library"""
    from sgdm_amd import _lib as L
    lib, calls = L.load(), {n: 0 for n in names}
    for n in names:
        def wrapped(*a, _n=n, _fn=getattr(lib, n)):
            calls[_n] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, n, wrapped)
    return calls


# ------------------------------------------------------------------------------------------------------------ loss kernels

@pytest.fixture(scope="module")
def scheds():
    """the schedule objects whose buffers are the kernels' tables: plain and zero-terminal, both with min_snr weights"""
    return dict(plain=_diffusion(learn_sigma=True, parameterization="v", loss_weighting="min_snr").sampler,
                zt=_diffusion(learn_sigma=True, parameterization="v", loss_weighting="min_snr", zero_terminal_snr=True).sampler)


def _tabs(s, dtype=torch.float32):
    names = dict(sa="sqrt_alphas_cumprod", s1="sqrt_one_minus_alphas_cumprod", r0="sqrt_recip_alphas_cumprod",
                 r1="sqrt_recipm1_alphas_cumprod", c1="posterior_mean_coef1", c2="posterior_mean_coef2", mx="lv_max_log",
                 mn="lv_min_log", wt="loss_weights")
    return {k: getattr(s, v).to(dtype) for k, v in names.items()}


def _dev(x, offset):
    buf = torch.empty(x.numel() + 4, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + x.numel()].view(x.shape)
    v.copy_(x)
    return v


def _case(s, b, Cc, hw, par, shift, seed, offset):
    """x0 on the 8-bit grid with exact -1 and +1, v uniform in [-1.5, 1.5], t from TS; a t == 0 sample's mean is drawn so that
    |x0 - mu_th| is at most 3 standard deviations (even elements) or 20.5 .. 30 (odd elements: the clamp)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor([TS[(i + shift) % len(TS)] for i in range(b)], dtype=torch.long)
    x0 = torch.randint(0, 256, (b, Cc, hw), generator=g).float() / 127.5 - 1.0
    x0[:, 0, 0], x0[:, -1, -1] = -1.0, 1.0
    noise, v = torch.randn(b, Cc, hw, generator=g), torch.rand(b, Cc, hw, generator=g) * 3.0 - 1.5
    m = torch.randn(b, Cc, hw, generator=g) * 1.2
    tb = {k: a.cpu().double() for k, a in _tabs(s).items()}
    for n in range(b):
        if int(t[n]) != 0:
            continue
        frac = (v[n].double() + 1) / 2
        lv = frac * tb["mx"][0] + (1 - frac) * tb["mn"][0]
        k = (torch.rand(Cc, hw, generator=g, dtype=torch.float64) * 2 - 1) * 3.0
        far = torch.sign(k) * (20.5 + k.abs() / 3.0 * 9.5)
        k.view(-1)[1::2] = far.view(-1)[1::2]
        x0p = x0[n].double() - k * torch.exp(0.5 * lv)              # mean_coef1[0] == 1, mean_coef2[0] == 0: mu_th = x0p
        xt = tb["sa"][0] * x0[n].double() + tb["s1"][0] * noise[n].double()
        m[n] = (x0p if par == 1 else (tb["r0"][0] * xt - x0p) / tb["r1"][0] if par == 0 else (tb["sa"][0] * xt - x0p) / tb["s1"][0]).float()
    out = torch.cat([m, v], 1)
    return dict(out=_dev(out, offset), x0=_dev(x0, offset), noise=_dev(noise, offset), t=t.cuda(), m=_dev(m, offset))


def _restate(c, tb, par, kind, weighted, gw, gv, dtype):
    """(per_raw, per_w, per_vlb, gout, share of t == 0 elements within a factor 2 of the clamp) in `dtype` on the device from
    the fp32 inputs, in the kernels' operation order; the decoder term always in double; means as double sums of the elements.
    The variance-half gradient is the kernel's closed form for t > 0 and autograd through the decoder term for t == 0"""
    out, x0, noise, t = c["out"].to(dtype), c["x0"].to(dtype), c["noise"].to(dtype), c["t"]
    b, Cc, hw = x0.shape
    f = lambda k: tb[k].to(dtype)[t].view(b, 1, 1)
    m, v = out[:, :Cc], out[:, Cc:]
    sa, s1, c1, c2, mx, mn = (f(k) for k in ("sa", "s1", "c1", "c2", "mx", "mn"))
    target = noise if par == 0 else x0 if par == 1 else sa * noise - s1 * x0
    d = m - target
    el = d * d if kind == 0 else d.abs() if kind == 1 else torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    w = tb["wt"].to(dtype)[t] if weighted else torch.ones(b, dtype=dtype, device="cuda")
    raw = el.double().reshape(b, -1).mean(1)
    chw = torch.tensor(float(Cc * hw), dtype=dtype, device="cuda")
    k = ((gw.to(dtype) * w) / chw).view(b, 1, 1)
    gm = (2 * k) * d if kind == 0 else k * torch.sign(d) if kind == 1 else k * d.clamp(-1, 1)
    xt = sa * x0 + s1 * noise
    x0p = f("r0") * xt - f("r1") * m if par == 0 else m if par == 1 else sa * xt - s1 * m
    mu_th, mu_q = c1 * x0p + c2 * xt, c1 * x0 + c2 * xt
    frac = (v + 1) * 0.5
    lv = frac * mx + (1 - frac) * mn
    dm = mu_q - mu_th
    e1, e2 = torch.exp(mn - lv), (dm * dm) * torch.exp(-lv)
    kl = (0.5 * ((((-1 + lv) - mn) + e1) + e2)) / LN2
    dkl = (0.5 * ((1 - e1) - e2)) / LN2
    gvar = ((gv.to(dtype) / chw).view(b, 1, 1) * (0.5 * (mx - mn))) * dkl
    # t == 0 in double, whatever `dtype`
    o64, x64, n64 = c["out"].double(), c["x0"].double(), c["noise"].double()
    f64 = lambda k: tb[k].double()[t].view(b, 1, 1)
    v64 = o64[:, Cc:].clone().requires_grad_(True)
    m64 = o64[:, :Cc]
    xt64 = f64("sa") * x64 + f64("s1") * n64
    x0p64 = f64("r0") * xt64 - f64("r1") * m64 if par == 0 else m64 if par == 1 else f64("sa") * xt64 - f64("s1") * m64
    mu64 = f64("c1") * x0p64 + f64("c2") * xt64
    fr64 = (v64 + 1) / 2
    lv64 = fr64 * f64("mx") + (1 - fr64) * f64("mn")
    inv, dd = torch.exp(-0.5 * lv64), x64 - mu64
    phi = lambda u: 0.5 * (1 + torch.tanh(math.sqrt(2 / math.pi) * (u + 0.044715 * u ** 3)))
    cp, cm = phi(inv * (dd + 1 / 255)), phi(inv * (dd - 1 / 255))
    p = torch.where(x64 < -0.999, cp, torch.where(x64 > 0.999, 1 - cm, cp - cm))
    dec = -torch.log(p.clamp(min=1e-12)) / LN2
    first = (t == 0).view(b, 1, 1)
    L = torch.where(first, dec, kl.double())
    vlb = L.reshape(b, -1).mean(1)
    (gdec,) = torch.autograd.grad((dec.reshape(b, -1).mean(1) * gv.double() * first.view(b)).sum(), v64)
    gvar = torch.where(first, gdec.to(dtype), gvar)
    near = (first & (p > 0.5e-12) & (p < 2e-12)).sum().item() / max(1, int(first.sum()) * Cc * hw)
    return raw, w.double() * raw, vlb.detach(), torch.cat([gm, gvar], 1), near


def _launch(lib, s, c, par, kind, weighted, gw, gv, offset):
    from sgdm_amd import _lib as L
    from sgdm_amd.losses import _lv_tables
    from sgdm_amd.unet import _ptr
    import ctypes as C
    b, Cc, hw = c["x0"].shape
    tabs = _lv_tables(s)
    wt = s.loss_weights if weighted else None
    res = [torch.full((b,), float("nan"), device="cuda") for _ in range(3)]
    L.check(lib.sgd_lv_loss_fwd(_ptr(c["out"]), _ptr(c["x0"]), _ptr(c["noise"]), _ptr(c["t"]), C.byref(tabs), _ptr(wt), par, kind,
                                b, Cc, hw, *(_ptr(r) for r in res), _st()), "sgd_lv_loss_fwd")
    n = b * 2 * Cc * hw
    buf = torch.full((n + 4,), float("nan"), device="cuda")
    gout = buf[offset:offset + n].view(b, 2 * Cc, hw)
    L.check(lib.sgd_lv_loss_bwd(_ptr(c["out"]), _ptr(c["x0"]), _ptr(c["noise"]), _ptr(c["t"]), C.byref(tabs), _ptr(wt),
                                gw.data_ptr(), gv.data_ptr(), par, kind, b, Cc, hw, _ptr(gout), _st()), "sgd_lv_loss_bwd")
    torch.cuda.synchronize()
    guard = torch.cat([buf[:offset], buf[offset + n:]])
    assert bool(torch.isnan(guard).all())                           # nothing written outside [b, 2C, hw]
    return res, gout


def _simple(lib, s, c, par, kind, weighted, gw, offset):
    """sgd_loss_fwd / sgd_loss_bwd on the mean half (a contiguous copy at the same offset from a 16-byte boundary)"""
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    b, Cc, hw = c["x0"].shape
    wt = s.loss_weights if weighted else None
    raw, pw = (torch.empty(b, device="cuda") for _ in range(2))
    a = (_ptr(c["m"]), _ptr(c["x0"]), _ptr(c["noise"]), _ptr(c["t"]), _ptr(s.sqrt_alphas_cumprod), _ptr(s.sqrt_one_minus_alphas_cumprod),
         _ptr(wt))
    L.check(lib.sgd_loss_fwd(*a, par, kind, b, Cc * hw, _ptr(raw), _ptr(pw), _st()), "sgd_loss_fwd")
    g = _dev(torch.zeros(b, Cc, hw), offset)
    L.check(lib.sgd_loss_bwd(*a, gw.data_ptr(), 1.0, par, kind, b, Cc * hw, _ptr(g), _st()), "sgd_loss_bwd")
    return raw, pw, g


def _relv(got, want):
    got, want = got.double(), want.double()
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()) if got.numel() else 0.0


# (b, C, hw, offset in floats): the scalar path (hw % 4 != 0), the 16-byte path on one and on several blocks per sample, a
# sample of three quads per channel, and two shapes once more from pointers one float past a 16-byte boundary
SHAPES = [(3, 3, 35, 0), (2, 4, 256, 0), (1, 3, 16, 0), (2, 3, 4096, 0), (2, 3, 4096, 1), (3, 3, 35, 1)]


@pytest.mark.parametrize("sched", ["plain", "zt"])
@pytest.mark.parametrize("b,Cc,hw,offset", SHAPES)
def test_loss_kernels(b, Cc, hw, offset, sched, scheds):
    from sgdm_amd import _lib as L
    lib = L.load()
    s = scheds[sched]
    if sched == "zt":
        assert float(s.lv_max_log[T - 1]) == 0.0 and float(s.sqrt_alphas_cumprod[T - 1]) == 0.0
    tb32 = _tabs(s)
    worst = dict(raw=0.0, vlb0=0.0, vlb=0.0, vlb_budget=0.0, g0=0.0, g=0.0, g_budget=0.0)
    for par in range(3):
        if sched == "zt" and par == 0:
            continue                                                # no 'eps' model on a zero-terminal-SNR schedule
        for kind in range(3):
            shift = par + kind + hw
            c = _case(s, b, Cc, hw, par, shift, seed=31 * par + 7 * kind + hw % 5, offset=offset)
            g = torch.Generator().manual_seed(hw + par)
            gw, gv = (torch.rand(b, generator=g) + 0.5).cuda(), (torch.rand(b, generator=g) + 0.5).cuda()
            for weighted in (True, False):
                (raw, pw, vlb), gout = _launch(lib, s, c, par, kind, weighted, gw, gv, offset)
                (raw2, pw2, vlb2), _ = _launch(lib, s, c, par, kind, weighted, gw, gv, offset)
                assert torch.equal(raw, raw2) and torch.equal(pw, pw2) and torch.equal(vlb, vlb2)       # no atomics
                s_raw, s_pw, s_g = _simple(lib, s, c, par, kind, weighted, gw, offset)
                assert torch.equal(raw, s_raw) and torch.equal(pw, s_pw)                                # sgd_loss_fwd's bits
                assert torch.equal(gout[:, :Cc], s_g), float((gout[:, :Cc] - s_g).abs().max())          # sgd_loss_bwd's bits
                _, gout0 = _launch(lib, s, c, par, kind, weighted, gw, torch.zeros_like(gv), offset)
                assert not gout0[:, Cc:].any() and torch.equal(gout0[:, :Cc], gout[:, :Cc])
                raw64, pw64, vlb64, g64, near = _restate(c, tb32, par, kind, weighted, gw, gv, torch.float64)
                _, _, vlb32, g32, _ = _restate(c, tb32, par, kind, weighted, gw, gv, torch.float32)
                assert near <= 1e-3                                  # (0 with these inputs: nothing is left out below)
                first = c["t"] == 0
                worst["raw"] = max(worst["raw"], _relv(raw, raw64), _relv(pw, pw64))
                worst["vlb0"] = max(worst["vlb0"], _relv(vlb[first], vlb64[first]))
                e, budget = _relv(vlb[~first], vlb64[~first]), max(1e-6, 4 * _relv(vlb32[~first], vlb64[~first]))
                assert e <= budget, (par, kind, e, budget)
                worst["vlb"], worst["vlb_budget"] = max(worst["vlb"], e), max(worst["vlb_budget"], budget)
                gvar, gvar64, gvar32 = gout[:, Cc:], g64[:, Cc:], g32[:, Cc:]
                if bool(first.any()):
                    worst["g0"] = max(worst["g0"], rel_l2(gvar[first].cpu(), gvar64[first].cpu()))
                if bool((~first).any()):
                    e = rel_l2(gvar[~first].cpu(), gvar64[~first].cpu())
                    budget = max(1e-5, 4 * rel_l2(gvar32[~first].cpu(), gvar64[~first].cpu()))
                    assert e <= budget, (par, kind, e, budget)
                    worst["g"], worst["g_budget"] = max(worst["g"], e), max(worst["g_budget"], budget)
    print(f"lv loss kernels b={b} C={Cc} hw={hw} offset={offset} [{sched}]: simple term bit-equal to sgd_loss_fwd/bwd, max rel "
          f"vs float64 {worst['raw']:.2e}; per_vlb t == 0 {worst['vlb0']:.2e}, t > 0 {worst['vlb']:.2e} (budget "
          f"{worst['vlb_budget']:.2e}); variance-half gradient rel-L2 t == 0 {worst['g0']:.2e}, t > 0 {worst['g']:.2e} (budget "
          f"{worst['g_budget']:.2e})")
    assert worst["raw"] <= 1e-6 and worst["vlb0"] <= 1e-6 and worst["g0"] <= 1e-5


def test_loss_entries_refuse_bad_arguments(scheds):
    import ctypes as C
    from sgdm_amd import _lib as L
    from sgdm_amd.losses import _lv_tables
    from sgdm_amd.unet import _ptr
    lib = L.load()
    s = scheds["plain"]
    f, t = torch.zeros(256, device="cuda"), torch.zeros(2, dtype=torch.long, device="cuda")
    good = C.byref(_lv_tables(s))
    no_mx, no_r0 = _lv_tables(s), _lv_tables(s)
    no_mx.max_log, no_r0.sqrt_recip_ac = None, None
    fwd = dict(out=_ptr(f), x0=_ptr(f), noise=_ptr(f), t=_ptr(t), tabs=good, wt=_ptr(s.loss_weights), par=2, kind=0, b=1, c=3, hw=8,
               raw=_ptr(f), pw=_ptr(f), vlb=_ptr(f), st=_st())
    bwd = dict(out=_ptr(f), x0=_ptr(f), noise=_ptr(f), t=_ptr(t), tabs=good, wt=_ptr(s.loss_weights), gw=f.data_ptr(),
               gv=f.data_ptr(), par=2, kind=0, b=1, c=3, hw=8, gout=_ptr(f), st=_st())
    common = (dict(out=None), dict(x0=None), dict(noise=None), dict(t=None), dict(tabs=None), dict(tabs=C.byref(no_mx)),
              dict(par=0, tabs=C.byref(no_r0)), dict(b=0), dict(b=-1), dict(c=0), dict(hw=0), dict(hw=-4), dict(par=3), dict(par=-1),
              dict(kind=3), dict(kind=-1))
    for args, fn, own in ((fwd, lib.sgd_lv_loss_fwd, (dict(raw=None), dict(pw=None), dict(vlb=None))),
                          (bwd, lib.sgd_lv_loss_bwd, (dict(gw=None), dict(gv=None), dict(gout=None)))):
        for bad in common + own:                                    # (keyword order is the C argument order)
            assert fn(*dict(args, **bad).values()) == 1, (fn.__name__, bad)     # SGD_ERR_ARG: refused before any launch
        for ok in (dict(wt=None), dict(par=2, tabs=C.byref(no_r0))):
            assert fn(*dict(args, **ok).values()) == 0, (fn.__name__, ok)
    step = dict(x=_ptr(f), out=_ptr(f), z=_ptr(f), mode=0, w=0.0, row=f.data_ptr(), clip=1, b=1, c=3, hw=8, x_out=_ptr(f), x0_out=None,
                st=_st())
    for bad in (dict(x=None), dict(out=None), dict(row=None), dict(x_out=None), dict(b=0), dict(c=0), dict(hw=0), dict(mode=3),
                dict(mode=-1)):
        assert lib.sgd_ddpm_lv_step(*dict(step, **bad).values()) == 1, bad
    assert lib.sgd_ddpm_lv_step(*dict(step, z=None).values()) == 0              # the all-zero row has kz == 0: z is not read
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ step kernel

def _ulps(a, b):
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("b,Cc,hw", [s[:3] for s in SHAPES[:4]])
def test_step_kernel_against_its_torch_fp32_restatement(b, Cc, hw):
    from sgdm_amd import _lib as L
    from sgdm_amd.diffusion import native_rows, native_times
    from sgdm_amd.unet import _ptr
    lib = L.load()
    rows = []
    for par, extra in (("eps", {}), ("x0", {}), ("v", {}), ("v", dict(zero_terminal_snr=True))):
        a = _diffusion(learn_sigma=True, parameterization=par, **extra).sampler.alphas_cumprod.double().cpu().numpy()
        tab, _ = native_rows(a[native_times(10, T)], "lv_native", par, [0.9] * 10)
        rows += [(f"{par}{'/zt' if extra else ''} row {i}", tab[i]) for i in (9, 4, 0)]
    assert float(rows[-3][1][0]) == 0.0 and float(rows[-1][1][6]) == 0.0        # the zero-terminal 'v' row (k0 = 0); a kz = 0 row
    g = torch.Generator().manual_seed(b * hw + Cc)
    x, z = torch.randn(b, Cc, hw, generator=g).cuda(), torch.randn(b, Cc, hw, generator=g).cuda()
    out = torch.randn(2 * b, hw, 2 * Cc, generator=g).cuda()
    out[..., Cc:] = out[..., Cc:].clamp(-1.5, 1.5)
    perm = out.clone()
    perm[b:, :, Cc:] = perm[b:, :, Cc:].flip(-1) + 1.0               # the unconditional half's variance channels: never read
    worst, total = 0, 0
    for name, row in rows:
        r = row.cuda()
        k0, k1, k2, k3, mx, mn, kz = (r[i] for i in range(7))
        for mode in (0, 1, 2):
            w32, one = torch.tensor(W, device="cuda"), torch.tensor(1.0, device="cuda")
            oc, ou = out[:b, :, :Cc].permute(0, 2, 1), out[b:, :, :Cc].permute(0, 2, 1)
            m = oc if mode == 0 else (one - w32) * ou + w32 * oc if mode == 1 else (one + w32) * oc - w32 * ou
            v = out[:b, :, Cc:].permute(0, 2, 1)
            for clip in (0, 1):
                x0 = k0 * x - k1 * m
                x0 = x0.clamp(-1, 1) if clip else x0
                want = k2 * x0 + k3 * x
                if float(kz) != 0.0:
                    frac = (v + 1) * 0.5
                    want = want + (torch.exp(0.5 * (frac * mx + (1 - frac) * mn)) * kz) * z
                got, got0 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
                zp = None if float(kz) == 0.0 else z
                L.check(lib.sgd_ddpm_lv_step(_ptr(x), _ptr(out), _ptr(zp), mode, W, r.data_ptr(), clip, b, Cc, hw, _ptr(got),
                                             _ptr(got0), _st()), "sgd_ddpm_lv_step")
                assert torch.equal(got0, x0.contiguous()), (name, mode, clip)
                u = _ulps(got, want.contiguous())
                worst, total = max(worst, u), total + 1
                # in place, no x0 output, and the permuted unconditional variance channels: the same bits
                xi = x.clone()
                L.check(lib.sgd_ddpm_lv_step(_ptr(xi), _ptr(perm if mode else out), _ptr(zp), mode, W, r.data_ptr(), clip, b, Cc, hw,
                                             _ptr(xi), None, _st()), "sgd_ddpm_lv_step")
                assert torch.equal(xi, got), (name, mode, clip)
    which = "bit-equal: the device's expf is torch's" if worst == 0 else "exp differs in the last place"
    print(f"sgd_ddpm_lv_step b={b} C={Cc} hw={hw}: {total} launches, worst distance from the torch-fp32 restatement {worst} ulp "
          f"({which})")
    assert worst <= 2


# ------------------------------------------------------------------------------------------------------- the 2C-wide head

KW = dict(image_size=S, in_channels=3, model_channels=32, num_res_blocks=2, channel_mult=[1, 2, 4], attention_resolutions=[4],
          num_heads=8, use_scale_shift_norm=True, use_ca_block=True, legacy=False, dropout=0.0, cond_token_num=1, cond_dim=27,
          context_dim=32, use_cls_token_as_pooled=True, condition_method="stegoclusterlayout")


def _build(out_channels, sd=None):
    from sgdm_amd.synth import weights_from_seed
    from sgdm_amd.unet import UNetModelCA
    m = UNetModelCA(condition=_AD(scale_type="imagen", stegoclusterlayout=_AD(layout_dim=27)), out_channels=out_channels, **KW)
    if sd is None:
        sd = weights_from_seed([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 23)
    m.load_state_dict(sd)
    return m.cuda().eval(), sd


@pytest.fixture(scope="module")
def wide():
    """(the c32 / 16x16 model with a 6-wide head, its weights, a batch of 4)"""
    from sgdm_amd.synth import synth_batch
    m, sd = _build(6)
    return m, sd, synth_batch("stegoclusterlayout", 4, S, 27, 27, seed=5)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_wide_head_forward_against_the_oracle(prec, wide):
    from oracle import unet_ref as U
    m, sd, batch = wide
    m.eval()
    m.hip_precision = prec
    cfg = U.make_cfg("unetca_fast", S, model_channels=32, cond_dim=27, condition_method="stegoclusterlayout", layout_dim=27,
                     cond_token_num=1, context_dim=32, out_channels=6)
    g = torch.Generator().manual_seed(9)
    x, t = torch.randn(B, 3, S, S, generator=g), torch.tensor([999, 3])
    cond, layout = batch["cond"][:B], batch["layout"][:B]
    errs = {}
    with torch.no_grad():
        for name, w in (("B", 1), ("2B", W)):                        # the int 1 is the single evaluation at B, 2.0 the doubled one
            ref = U.forward_with_cond_scale(cfg, sd, x, t, w, cond, layout)
            got = m.forward_with_cond_scale(x.cuda(), t.cuda(), cond_scale=w, cond=cond.cuda(), layout=layout.cuda())
            assert tuple(got.shape) == (B, 6, S, S)
            errs[name] = float((got.cpu() - ref).abs().max() / ref.abs().max())
    print(f"6-wide head forward [{prec}] max-rel-err vs oracle: {errs}")
    assert max(errs.values()) < 1e-4


def _attach(d, m):
    seen = {}

    def denoise_fn(x, t, **kw):
        out = m.forward(x, t, **kw)
        seen["x_noisy"], seen["out"] = x.detach().clone(), out[0].detach().clone()
        return out
    d.set_denoise_fn(denoise_fn, m.forward_with_cond_scale)
    return seen


NAMES = ("first", "last", "out.2.weight", "out.2.bias")


def _grads(m):
    named = dict(m.named_parameters())
    params = [p for p in m.parameters() if p.requires_grad and p.grad is not None]     # (on the path of this model kind)
    return dict(zip(NAMES, (params[0].grad.clone(), params[-1].grad.clone(), named["out.2.weight"].grad.clone(),
                            named["out.2.bias"].grad.clone())))


def _loss64(d, par, kind, x0, noise, x_noisy, out, t, weights):
    """float64 restatement of mean(per_w + vlb_weight * per_vlb) on the observed x_noisy and model output"""
    s = d.sampler
    n = len(t)
    f = lambda name: getattr(s, name).double()[t].view(n, 1, 1, 1)
    o, x, nz, xt = out.double(), x0.double(), noise.double(), x_noisy.double()
    m, v = o[:, :3], o[:, 3:]
    sa, s1 = f("sqrt_alphas_cumprod"), f("sqrt_one_minus_alphas_cumprod")
    target = dict(eps=nz, x0=x, v=sa * nz - s1 * x)[par]
    dd = m - target
    el = dict(l2=dd * dd, l1=dd.abs(), huber=torch.where(dd.abs() < 1, 0.5 * dd * dd, dd.abs() - 0.5))[kind]
    raw = el.reshape(n, -1).mean(1)
    x0p = f("sqrt_recip_alphas_cumprod") * xt - f("sqrt_recipm1_alphas_cumprod") * m if par == "eps" else sa * xt - s1 * m
    c1, c2 = f("posterior_mean_coef1"), f("posterior_mean_coef2")
    mu_th, mu_q = c1 * x0p + c2 * xt, c1 * x + c2 * xt
    frac = (v + 1) / 2
    lq = f("lv_min_log")
    lv = frac * f("lv_max_log") + (1 - frac) * lq
    kl = 0.5 * (-1 + lv - lq + torch.exp(lq - lv) + (mu_q - mu_th) ** 2 * torch.exp(-lv)) / LN2
    inv, dx = torch.exp(-0.5 * lv), x - mu_th
    phi = lambda u: 0.5 * (1 + torch.tanh(math.sqrt(2 / math.pi) * (u + 0.044715 * u ** 3)))
    cp, cm = phi(inv * (dx + 1 / 255)), phi(inv * (dx - 1 / 255))
    p = torch.where(x < -0.999, cp, torch.where(x > 0.999, 1 - cm, cp - cm))
    dec = -torch.log(p.clamp(min=1e-12)) / LN2
    vlb = torch.where((t == 0).view(n, 1, 1, 1), dec, kl).reshape(n, -1).mean(1)
    w = 1.0 if weights is None else weights.double()[t]
    return (w * raw + s.vlb_weight * vlb).mean(), raw, vlb


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("par,extra", [("eps", {}), ("v", dict(loss_weighting="min_snr"))])
def test_training_step_with_learned_variance(par, extra, prec, wide, monkeypatch):
    from sgdm_amd.losses import lv_vlb_torch, simple_loss_torch as _simple_torch
    m, sd, batch = wide
    m.train()
    m.hip_precision = prec
    N = 4
    d = _diffusion(parameterization=par, learn_sigma=True, **extra).train()
    seen = _attach(d, m)
    s = d.sampler
    g = torch.Generator().manual_seed(3)
    x0 = (torch.randint(0, 256, (N, 3, S, S), generator=g).float() / 127.5 - 1.0).cuda()
    noise = torch.randn(N, 3, S, S, generator=g).cuda()
    t = torch.tensor([0, 1, 241, T - 1]).cuda()
    ukw = dict(cond=batch["cond"].cuda(), layout=batch["layout"].cuda(), cond_drop_prob=0.5,
               cond_drop_mask=torch.tensor([True, False, False, True]).cuda())
    calls = _count(monkeypatch, "sgd_q_sample_v", "sgd_q_sample", "sgd_lv_loss_fwd", "sgd_lv_loss_bwd", "sgd_loss_fwd", "sgd_loss_bwd")
    m.zero_grad(set_to_none=True)
    loss, ld = d.p_losses(x0, t, noise, **ukw)
    loss.backward()
    assert calls == dict(sgd_q_sample_v=0, sgd_q_sample=1, sgd_lv_loss_fwd=1, sgd_lv_loss_bwd=1, sgd_loss_fwd=0, sgd_loss_bwd=0)
    got = _grads(m)
    assert tuple(seen["out"].shape) == (N, 6, S, S)
    weights = s.loss_weights if extra else None
    want, raw64, vlb64 = _loss64(d, par, "l2", x0, noise, seen["x_noisy"], seen["out"], t, weights)
    err_l = abs(float(loss.detach()) - float(want)) / abs(float(want))
    keys =["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss", "train/vlb"] + (["train/ddpm_loss_raw"] if extra else [])
    assert sorted(ld) == sorted(keys)
    assert float(ld["train/vlb"]) == pytest.approx(float(vlb64.mean()), rel=1e-5)
    assert max_rel(ld["train/epoch_stats_y"].cpu(), raw64.cpu()) < 1e-6
    # the same step through the torch chain of the CPU branch, under autograd on the device
    m.zero_grad(set_to_none=True)
    out = m.forward(seen["x_noisy"], t, **ukw)[0]
    assert torch.equal(out.detach(), seen["out"])
    sa, s1 = (s._ext(a, t, x0.shape) for a in (s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod))
    target = noise if par == "eps" else sa * noise - s1 * x0
    per = _simple_torch("l2", target, out[:, :3])
    per = per if weights is None else per * weights[t]
    (per + s.vlb_weight * lv_vlb_torch(s, out, x0, noise, t, par)).mean().backward()
    ref = _grads(m)
    errs = {k: max_rel(got[k], ref[k]) for k in NAMES}
    print(f"learn_sigma training step {par} {extra} [{prec}], t {t.tolist()}: loss rel err vs float64 {err_l:.2e}; gradients vs the "
          f"torch chain {({k: f'{v:.2e}' for k, v in errs.items()})}")
    for k in NAMES:
        assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) > 0, k
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    assert err_l < 1e-6
    assert max(errs.values()) < 1e-4
    # validation: the forward kernel only
    with torch.no_grad():
        d.eval().p_losses(x0, t, noise, **ukw)
    assert calls["sgd_lv_loss_fwd"] == 2 and calls["sgd_lv_loss_bwd"] == 1


def test_without_the_hparam_the_step_is_untouched(wide, monkeypatch):
    """an ordinary model's step before and after a learn_sigma step on a second model: bit-equal, no new entry called"""
    from sgdm_amd.synth import synth_batch
    m6, _, batch = wide
    m3, _ = _build(3)
    m3.train(), m6.train()
    m3.hip_precision = m6.hip_precision = "f16x3"
    N = 4
    g = torch.Generator().manual_seed(4)
    x0, noise = torch.randn(N, 3, S, S, generator=g).cuda(), torch.randn(N, 3, S, S, generator=g).cuda()
    t = torch.tensor([0, 999, 250, 731]).cuda()
    ukw = dict(cond=batch["cond"].cuda(), layout=batch["layout"].cuda(), cond_drop_prob=0.5,
               cond_drop_mask=torch.tensor([True, False, False, True]).cuda())
    plain, lv = _diffusion().train(), _diffusion(learn_sigma=True).train()
    plain.set_denoise_fn(m3.forward, m3.forward_with_cond_scale)
    lv.set_denoise_fn(m6.forward, m6.forward_with_cond_scale)
    assert not hasattr(plain.sampler, "lv_max_log")
    calls = _count(monkeypatch, "sgd_lv_loss_fwd", "sgd_lv_loss_bwd", "sgd_ddpm_lv_step")

    def step(d, m):
        m.zero_grad(set_to_none=True)
        loss, ld = d.p_losses(x0, t, noise, **ukw)
        loss.backward()
        return loss.detach().clone(), ld, _grads(m)

    before = step(plain, m3)
    assert calls == dict(sgd_lv_loss_fwd=0, sgd_lv_loss_bwd=0, sgd_ddpm_lv_step=0)
    step(lv, m6)
    assert calls["sgd_lv_loss_fwd"] == calls["sgd_lv_loss_bwd"] == 1
    after = step(plain, m3)
    assert calls["sgd_lv_loss_fwd"] == calls["sgd_lv_loss_bwd"] == 1
    assert sorted(before[1]) == sorted(after[1]) == ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    assert torch.equal(before[0], after[0]) and all(torch.equal(before[2][k], after[2][k]) for k in NAMES)


# ------------------------------------------------------------------------------------------------------------ trajectories

SHAPE = (B, 3, S, S)


@pytest.fixture(scope="module")
def pair(wide):
    """(the 6-wide model, an out_channels=3 model with the same weights whose out.2 holds rows [0, 3), cond, layout), f16x3"""
    m6, sd, batch = wide
    sd3 = {k: (v[:3].clone() if k.startswith("out.2.") else v.clone()) for k, v in sd.items()}
    m3, _ = _build(3, sd3)
    return m6, m3, batch["cond"][:B].cuda(), batch["layout"][:B].cuda()


def _sk(d, method, steps, **kw):
    sk = dict(sampling_method=method, vis=None, num_timesteps=steps, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True, dtp=1,
              temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True, disable_tqdm=True,
              alphas_cumprod=d.sampler.alphas_cumprod, parameterization=d.hparams.parameterization)
    if d.hparams.parameterization == "v":
        sk.update(sqrt_alphas_cumprod=d.sampler.sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod=d.sampler.sqrt_one_minus_alphas_cumprod)
    return dict(sk, **kw)                                           # (nothing about learn_sigma: the step reads the model's width)


def _run(d, method, sk, cond, layout, x_T, graph, **kwx):
    final, inter = d.sampler_list[method].sample(
        shape=SHAPE, sampling_kwargs=dict(sk, hip_graph=graph), denoise_sample_fn=d.denoise_sample_fn,
        denoise_sample_fn_kwargs=dict(cond=cond, layout=layout, cond_scale=W), x_T=x_T.clone(), **kwx)
    return final.cpu(), inter["x_inter"].cpu(), inter["pred_x0"].cpu()


def _x_T(seed):
    return torch.randn(*SHAPE, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("par,learn,form", [("eps", True, "eps"), ("v", True, "eps"), ("eps", False, "eps"), ("v", False, "eps"),
                                            ("v", False, "data")])
def test_strided_native_trajectory(par, learn, form, pair, monkeypatch):
    """native_steps=10: captured == eager bit for bit, every step teacher-forced against the method restated in float64 from
    alphas_cumprod alone, and the times the UNet is given are s_i.  The three native update kinds: learned variance, fixed
    variance on the eps form (for 'v': sgd_v_to_eps, then sgd_ddpm_step on the chain's eps rows) and fixed variance on the
    data form of 'v'"""
    from sgdm_amd import _lib as L
    from sgdm_amd import diffusion as Dm
    m6, m3, cond, layout = pair
    m = m6 if learn else m3
    m.eval()
    m.hip_precision = "f16x3"
    K = 10
    d = _diffusion(parameterization=par, **(dict(learn_sigma=True) if learn else {}))
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    times = [int(round(i * (T - 1) / (K - 1))) for i in range(K)]
    g = torch.Generator().manual_seed(17)
    zs = {i: torch.randn(*SHAPE, generator=g) for i in range(K)}
    data = form == "data"
    sk = _sk(d, "native", T, native_steps=K, temperature=0.9, log_num_per_prog=K + 1, **(dict(v_form="data") if data else {}))
    x_T = _x_T(61)
    calls = _count(monkeypatch, "sgd_ddpm_lv_step", "sgd_ddpm_step", "sgd_v_step")
    # the time the UNet is actually given: the argument of every eager evaluation, and the static buffer the captured
    # launches read at every replay
    given = {False: [], True: []}
    run0, step0 = m._run, Dm._GraphedStep.step

    def spy_run(x, t, *a, **k):
        given[False].append(t.tolist())
        return run0(x, t, *a, **k)

    def spy_step(self, i, *a, **k):
        step0(self, i, *a, **k)
        given[True].append(self.t.tolist())
    out = {}
    for graph in (False, True):
        torch.manual_seed(5)
        with monkeypatch.context() as mp:
            if graph:
                mp.setattr(Dm._GraphedStep, "step", spy_step)
            else:
                mp.setattr(m, "_run", spy_run)
            out[graph] = _run(d, "native", sk, cond, layout, x_T, graph, noise_fn=lambda i: zs[i])
    for graph in (False, True):
        assert given[graph] == [[s] * B for s in reversed(times)], (graph, given[graph])
    used = "sgd_ddpm_lv_step" if learn else "sgd_v_step" if data else "sgd_ddpm_step"
    assert calls[used] > 0 and all(v == 0 for k, v in calls.items() if k != used), calls
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)
    final, x_inter, pred_x0 = out[True]
    assert tuple(x_inter.shape) == (K,) + SHAPE and torch.equal(x_inter[-1], final) and bool(torch.isfinite(x_inter).all())
    # the method in float64 from the fp32 alphas_cumprod of the visited times
    ac = d.sampler.alphas_cumprod.double().cpu().numpy()[times]
    ap = np.concatenate([[1.0], ac[:-1]])
    beta = 1 - ac / ap
    c1, c2, pv = beta * np.sqrt(ap) / (1 - ac), (1 - ap) * np.sqrt(1 - beta) / (1 - ac), beta * (1 - ap) / (1 - ac)
    mx, mn = np.log(beta), np.log(np.maximum(pv, 1e-300))
    mn[0] = mn[1]
    prec = L.PREC_BY_NAME[m.hip_precision]
    ins = [x_T.cpu()] + list(x_inter[:-1])
    errs, errs0 = [], []
    for k, i in enumerate(reversed(range(K))):
        x = ins[k].cuda()
        tt = torch.full((B,), times[i], dtype=torch.long, device="cuda")
        guided = m.forward_with_cond_scale(x, tt, cond=cond, layout=layout, cond_scale=W).double()
        mean = guided[:, :3]
        if par == "eps":
            x0 = math.sqrt(1 / ac[i]) * x.double() - math.sqrt(1 / ac[i] - 1) * mean
        else:
            x0 = math.sqrt(ac[i]) * x.double() - math.sqrt(1 - ac[i]) * mean
        x0 = x0.clamp(-1, 1)
        if learn:
            # the halves of the doubled evaluation: the variance channels of the CONDITIONAL half
            raw = m._engine(2 * B, S, S, prec).eps_nhwc.double().reshape(2 * B, S * S, 6)
            v = raw[:B, :, 3:].permute(0, 2, 1).reshape(B, 3, S, S)
            frac = (v + 1) / 2
            sig = torch.exp(0.5 * (frac * mx[i] + (1 - frac) * mn[i]))
        else:
            sig = math.sqrt(pv[i]) if i > 0 else 0.0
        nxt = c1[i] * x0 + c2[i] * x.double() + (0.0 if i == 0 else 0.9) * sig * zs[i].cuda().double()
        errs.append(rel_l2(x_inter[k], nxt.cpu()))
        errs0.append(rel_l2(pred_x0[k], x0.cpu()))
    print(f"native_steps={K} {par} learn_sigma={learn} form={form}, fused CFG w {W}: captured == eager, UNet times s_i; vs float64, "
          f"teacher-forced: max rel_l2 "
          f"{max(errs):.3e}, pred_x0 {max(errs0):.3e}")
    assert max(errs) <= 1e-5, errs
    assert max(errs0) <= 1e-5, errs0


def test_generic_denoiser_on_the_learned_variance_update(pair):
    """a generic ``denoise_sample_fn`` (guided NCHW [B, 2C, H, W]) is re-laid as [B, hw, 2C] and stepped eagerly with mode 0:
    every step against the method in float64 on the function's own output; 'ddim' slices the mean half in torch"""
    m6, m3, cond, layout = pair
    m6.eval()
    m6.hip_precision = "f16x3"
    K = 4
    d = _diffusion(learn_sigma=True)
    fn = lambda x, t, **kw: m6.forward_with_cond_scale(x, t, **kw)          # not the bound method: the generic path
    d.set_denoise_fn(m6.forward, fn)
    times = [int(round(i * (T - 1) / (K - 1))) for i in range(K)]
    g = torch.Generator().manual_seed(19)
    zs = {i: torch.randn(*SHAPE, generator=g) for i in range(K)}
    sk = _sk(d, "native", T, native_steps=K, log_num_per_prog=K + 1)
    x_T = _x_T(3)
    final, x_inter, pred_x0 = _run(d, "native", sk, cond, layout, x_T, True, noise_fn=lambda i: zs[i])
    ac = d.sampler.alphas_cumprod.double().cpu().numpy()[times]
    ap = np.concatenate([[1.0], ac[:-1]])
    beta = 1 - ac / ap
    c1, c2, pv = beta * np.sqrt(ap) / (1 - ac), (1 - ap) * np.sqrt(1 - beta) / (1 - ac), beta * (1 - ap) / (1 - ac)
    mx, mn = np.log(beta), np.log(np.maximum(pv, 1e-300))
    mn[0] = mn[1]
    ins = [x_T.cpu()] + list(x_inter[:-1])
    errs = []
    for k, i in enumerate(reversed(range(K))):
        x = ins[k].cuda()
        out = fn(x, torch.full((B,), times[i], dtype=torch.long, device="cuda"), cond=cond, layout=layout, cond_scale=W).double()
        x0 = (math.sqrt(1 / ac[i]) * x.double() - math.sqrt(1 / ac[i] - 1) * out[:, :3]).clamp(-1, 1)
        frac = (out[:, 3:] + 1) / 2
        sig = torch.exp(0.5 * (frac * mx[i] + (1 - frac) * mn[i]))
        nxt = c1[i] * x0 + c2[i] * x.double() + (0.0 if i == 0 else 1.0) * sig * zs[i].cuda().double()
        errs.append(max(rel_l2(x_inter[k], nxt.cpu()), rel_l2(pred_x0[k], x0.cpu())))
    torch.manual_seed(5)
    dd = _run(d, "ddim", _sk(d, "ddim", 4, log_num_per_prog=5), cond, layout, x_T, True)
    print(f"generic denoiser, native_steps={K}, learned variance: worst step rel_l2 vs float64 {max(errs):.3e}; ddim-4 finite")
    assert max(errs) <= 1e-5, errs
    assert bool(torch.isfinite(dd[0]).all()) and tuple(dd[0].shape) == SHAPE


def test_other_samplers_ignore_the_variance_half(pair):
    """ddim-10 and dpmsolver-10 of the learn_sigma model: bit-equal to the out_channels=3 twin, on an engine whose eps_nhwc is
    C wide; the twin's default captured ddim trajectory is bit-equal before and after"""
    from sgdm_amd import _lib as L
    m6, m3, cond, layout = pair
    for m in (m6, m3):
        m.eval()
        m.hip_precision = "f16x3"
    d6, d3 = _diffusion(learn_sigma=True), _diffusion()
    d6.set_denoise_fn(m6.forward, m6.forward_with_cond_scale)
    d3.set_denoise_fn(m3.forward, m3.forward_with_cond_scale)
    x_T = _x_T(7)

    def both(d, method):
        torch.manual_seed(5)
        return _run(d, method, _sk(d, method, 10, log_num_per_prog=11), cond, layout, x_T, True)

    before = both(d3, "ddim")
    for method in ("ddim", "dpmsolver"):
        got, want = both(d6, method), both(d3, method)
        for a, b in zip(got, want):
            assert torch.equal(a, b), method
        torch.manual_seed(5)
        eager = _run(d6, method, _sk(d6, method, 10, log_num_per_prog=11), cond, layout, x_T, False)
        assert torch.equal(eager[0], got[0]), method
    prec = L.PREC_BY_NAME["f16x3"]
    assert (2 * B, S, S, prec, 3) in m6._engines and tuple(m6._engines[(2 * B, S, S, prec, 3)].eps_nhwc.shape) == (2 * B, S, S, 3)
    after = both(d3, "ddim")
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    # the samples of p_sample_loop: the same route
    skp = dict(num_timesteps=10, ddim_eta=0.0, log_num_per_prog=2, clip_denoised=True, temperature=1.0)
    kw = dict(denoise_sample_fn_kwargs=dict(cond=cond, layout=layout, cond_scale=W), x_T=x_T.clone())
    a, _ = d6.p_sample_loop("ddim", SHAPE, skp, **kw)
    b, _ = d3.p_sample_loop("ddim", SHAPE, skp, **dict(kw, x_T=x_T.clone()))
    assert torch.equal(a, b)


def test_refusals_before_any_launch(pair, monkeypatch):
    m6, m3, cond, layout = pair
    m6.eval()
    d = _diffusion(learn_sigma=True)
    d.set_denoise_fn(m6.forward, m6.forward_with_cond_scale)
    calls = _count(monkeypatch, "sgd_igemm", "sgd_ddpm_lv_step", "sgd_timestep_embedding")
    base = _sk(d, "native", T, native_steps=10)
    for bad in (dict(dtp=0.9), dict(noise_dropout=0.1), dict(cfg_interval=(0, 500)), dict(cfg_rescale=0.5), dict(v_form="data"),
                dict(native_steps=1), dict(native_steps=T + 1)):
        with pytest.raises(ValueError):
            _run(d, "native", dict(base, **bad), cond, layout, _x_T(1), True)
    for method in ("ddim", "plms", "pndm", "dpmsolver"):
        with pytest.raises(ValueError, match="native_steps"):
            _run(d, method, _sk(d, method, 10, native_steps=5), cond, layout, _x_T(1), True)
    with pytest.raises(ValueError, match="out_channels"):
        d.set_denoise_fn(m3.forward, m3.forward_with_cond_scale)
    # a network output that is neither C nor 2C wide, and a C-wide one under the learned-variance update
    odd = _diffusion()
    odd.set_denoise_fn(m3.forward, lambda x, t, **k: torch.zeros(B, 5, S, S, device="cuda"))
    with pytest.raises(ValueError, match="channels"):
        _run(odd, "ddim", _sk(odd, "ddim", 4), cond, layout, _x_T(1), True)
    thin = _diffusion(learn_sigma=True)
    thin.set_denoise_fn(m6.forward, lambda x, t, **k: torch.zeros(B, 3, S, S, device="cuda"))
    with pytest.raises(ValueError, match="channels"):
        _run(thin, "native", _sk(thin, "native", T, native_steps=4), cond, layout, _x_T(1), True)
    assert calls ==dict(sgd_igemm=0, sgd_ddpm_lv_step=0, sgd_timestep_embedding=0)


# ---------------------------------------------------------------------------------------------------------------- calc_bpd

def test_calc_bpd_is_the_sum_of_the_per_timestep_terms(wide, monkeypatch):
    m, sd, batch = wide
    m.eval()
    m.hip_precision = "f16x3"
    TT = 12                                                 # a short schedule: calc_bpd evaluates the UNet once per timestep
    d = _diffusion(learn_sigma=True, num_timesteps=TT).eval()
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    g = torch.Generator().manual_seed(8)
    x0 = (torch.randint(0, 256, (B, 3, S, S), generator=g).float() / 127.5 - 1.0).cuda()
    noises = {t: torch.randn(B, 3, S, S, generator=g).cuda() for t in range(TT)}
    ckw = dict(cond=batch["cond"][:B].cuda(), layout=batch["layout"][:B].cuda())
    calls = _count(monkeypatch, "sgd_lv_loss_fwd", "sgd_lv_loss_bwd")
    out = d.calc_bpd(x0, noise_fn=lambda t: noises[t], **ckw)
    assert calls == dict(sgd_lv_loss_fwd=TT, sgd_lv_loss_bwd=0)
    vb = out["vb"]
    assert tuple(vb.shape) == (B, TT) and bool(torch.isfinite(out["total_bpd"]).all()) and bool((out["prior_bpd"] > 0).all())
    for t in range(TT):                                     # explicit p_losses calls fed the same noise
        tt = torch.full((B,), t, dtype=torch.long, device="cuda")
        with torch.no_grad():
            loss, ld = d.p_losses(x0, tt, noises[t], **ckw)
        assert float(ld["val/vlb"]) == float(vb[:, t].mean()), t
        assert float(loss) == pytest.approx(float(ld["val/ddpm_loss"] + d.sampler.vlb_weight * vb[:, t].mean()), rel=1e-6)
    assert torch.allclose(out["total_bpd"], vb.sum(1) + out["prior_bpd"])
    print(f"calc_bpd on the c32 model, T = {TT}: total {out['total_bpd'].tolist()} bits/dim, prior {out['prior_bpd'].tolist()}")
