"""Learned variance (hparam learn_sigma; Nichol & Dhariwal 2021, "Improved DDPM") where it needs no GPU: the two log-variance
tables, the strided ancestral chain of the sampling kwarg native_steps, the CPU branch of the hybrid loss against a float64
restatement written here, calc_bpd on a stub denoiser, the refusals, the unchanged path without the hparam and the binding of
the new entry points.  The reference has no learned variance; the expected values are the published formulas restated."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

T = 1000
LN2 = math.log(2.0)
SCHEDULES = {"linear": dict(beta_schedule="linear"), "cosine": dict(beta_schedule="cosine"),
             "zt": dict(beta_schedule="linear", zero_terminal_snr=True, parameterization="v")}
PARS, KINDS = ("eps", "x0", "v"), ("l2", "l1", "huber")


def _diffusion(**kw):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cpu", **dict(bench.MODEL_PARAMS, **kw))


class _AD(dict):
    __getattr__ = dict.__getitem__


def _unet(out_channels):
    """the tiny conditional UNet of the smoke run (constructed on the CPU, never evaluated here)"""
    from sgdm_amd.unet import UNetModelCA
    return UNetModelCA(condition=_AD(scale_type="imagen", stegoclusterlayout=_AD(layout_dim=27)), image_size=16, in_channels=3,
                       out_channels=out_channels, model_channels=32, num_res_blocks=2, channel_mult=[1, 2, 4],
                       attention_resolutions=[4], num_heads=8, use_scale_shift_norm=True, use_ca_block=True, legacy=False,
                       dropout=0.0, cond_token_num=1, cond_dim=27, context_dim=32, use_cls_token_as_pooled=True,
                       condition_method="stegoclusterlayout")


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())


# ----------------------------------------------------------------------------------------------------------------- tables

@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_log_variance_tables(sched):
    d = _diffusion(learn_sigma=True, **SCHEDULES[sched])
    s = d.sampler
    mx, mn = s.lv_max_log, s.lv_min_log
    for tab in (mx, mn):
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (T,) and bool(torch.isfinite(tab).all())
    assert float(mn[0]) == float(mn[1])
    assert bool((mn <= mx).all())
    assert "lv_max_log" not in d.state_dict() and "lv_min_log" not in d.state_dict()         # non-persistent
    # float64 from the fp32 buffers, rounded once
    b, a = s.betas.double().numpy(), s.alphas_cumprod.double().numpy()
    ap = np.append(1.0, a[:-1])
    assert np.array_equal(mx.numpy(), np.log(b).astype(np.float32))
    assert np.array_equal(mn.numpy()[1:], np.log(b * (1 - ap) / (1 - a)).astype(np.float32)[1:])
    if sched == "zt":
        assert float(mx[T - 1]) == 0.0
    assert d.sampler.vlb_weight == T / 1000.0
    assert _diffusion(learn_sigma=True, vlb_weight=0.25).sampler.vlb_weight == 0.25


# ----------------------------------------------------------------------------------------------------------- native_steps

@pytest.mark.parametrize("K", [2, 10, 100, 250, 999, 1000])
def test_native_times(K):
    from sgdm_amd.diffusion import native_times
    s = native_times(K, T)
    assert len(s) == K and s[0] == 0 and s[-1] == T - 1 and bool((np.diff(s) > 0).all())
    assert [int(v) for v in s] == [int(round(i * (T - 1) / (K - 1))) for i in range(K)]


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("kind", ["ddpm", "v_native", "lv_native"])
def test_strided_chain_reproduces_alphas_cumprod(sched, kind):
    from sgdm_amd.diffusion import native_rows, native_times
    d = _diffusion(learn_sigma=True, **SCHEDULES[sched])
    par = d.hparams.parameterization
    a = d.sampler.alphas_cumprod.double().numpy()
    for K in (10, 100):
        s = native_times(K, T)
        tab, beta = native_rows(a[s], kind, par, [1.0] * K)
        assert np.abs(np.cumprod(1.0 - beta) - a[s]).max() <= 1e-12
        assert tab.dtype == torch.float32 and tab.shape == (K, 5 if kind == "ddpm" else 8)
        if kind == "lv_native":
            assert bool(torch.isfinite(tab[:, 2:]).all()) and float(tab[0, 6]) == 0.0 and float(tab[0, 5]) == float(tab[1, 5])
            assert bool((tab[:, 5] <= tab[:, 4]).all())
            if par == "v":
                assert bool(torch.isfinite(tab).all())                  # the 'v' row never divides by sqrt(ac)
                if sched == "zt":
                    assert float(tab[-1, 0]) == 0.0 and float(tab[-1, 4]) == 0.0


@pytest.mark.parametrize("par", PARS)
def test_full_chain_is_the_unstrided_table_to_fp32_rounding(par, capsys):
    """K = T: float64 from the fp32 alphas_cumprod against the tables built from the float64 betas -- not bit-equal (1 - ac_t /
    ac_{t-1} of two fp32 numbers resolves a beta of 1e-4 to ~1e-3 relative), and not promised to be.  For every
    parameterization: the 'ddpm' rows of a 'v' model carry the eps pair (sqrt(1/ac), sqrt(1/ac - 1)) like ``step_table``,
    because the step runner has changed v to eps before sgd_ddpm_step reads it"""
    from sgdm_amd.diffusion import native_rows
    d = _diffusion(parameterization=par)
    s = d.sampler
    a = s.alphas_cumprod.double().numpy()
    tab, _ = native_rows(a, "ddpm", par, [1.0] * T)
    want = s.step_table([1.0] * T)
    if par == "x0":
        assert torch.equal(tab[:, :2], want[:, :2]) and float(tab[5, 0]) == 0.0 and float(tab[5, 1]) == -1.0
        tab, want = tab.clone(), want.clone()
        tab[:, :2], want[:, :2] = 1.0, 1.0                  # (exact above; the relative distance of a 0 is not defined)
    dist = [_rel(tab[:, j], want[:, j]) for j in range(5)]
    with capsys.disabled():
        print(f"\nnative_steps=T vs unstrided table [{par}]: worst relative distance per column {dist}")
    # sqrt(1 / ac) only rounds; every other column holds 1 - ac or beta' = 1 - ac_t / ac_{t-1}, a difference of fp32-rounded
    # numbers near 1: each ac is off by up to 2^-24 relative, so the difference by up to 2 * 2^-24 absolute -- relative to the
    # smallest beta of the schedule, with a factor 2 for the quotients and the final rounding
    assert dist[0] <= 2.0 ** -22
    assert max(dist[1:]) <= 4 * 2.0 ** -24 / float(s.betas.min())
    assert float(tab[0, 4]) == 0.0 == float(want[0, 4]) and float(tab[0, 3]) == 0.0 == float(want[0, 3])


def test_native_steps_refusals():
    from sgdm_amd.diffusion import lv_native_option, native_steps_option
    for method in ("ddim", "plms", "pndm", "dpmsolver"):
        with pytest.raises(ValueError, match="native_steps"):
            native_steps_option(dict(native_steps=10), method, T)
    for K in (1, 0, -3, T + 1, 2.5, True):
        with pytest.raises(ValueError, match="native_steps"):
            native_steps_option(dict(native_steps=K), "native", T)
    assert native_steps_option({}, "ddim", T) is None and native_steps_option(dict(native_steps=T), "native", T) == T
    # through the samplers and p_sample_loop: before anything is loaded or launched (device='cpu': nothing could be)
    d = _diffusion()
    d.set_denoise_fn(None, lambda *a, **k: None)
    sk = dict(num_timesteps=10, ddim_eta=0.0, temperature=1.0, clip_denoised=True, log_num_per_prog=2, native_steps=5)
    for method in ("ddim", "plms", "pndm", "dpmsolver"):
        with pytest.raises(ValueError, match="native_steps"):
            d.p_sample_loop(method, (1, 3, 8, 8), sk)
        with pytest.raises(ValueError, match="native_steps"):
            d.sampler_list[method].sample(shape=(1, 3, 8, 8), sampling_kwargs=dict(sk, alphas_cumprod=d.sampler.alphas_cumprod))
    with pytest.raises(ValueError, match="native_steps"):
        d.p_sample_loop("native", (1, 3, 8, 8), dict(sk, num_timesteps=T, native_steps=1))
    # an eps-form strided trajectory that visits alphas_cumprod == 0: the v_form_option rule
    z = _diffusion(zero_terminal_snr=True, parameterization="v")
    z.set_denoise_fn(None, lambda *a, **k: None)
    with pytest.raises(ValueError, match="alphas_cumprod is 0"):
        z.sampler.sample((1, 3, 8, 8), sampling_kwargs=dict(sk, num_timesteps=T, v_form="eps"), denoise_sample_fn=None)
    # the learned-variance native update refuses what its one launch does not implement
    for bad in (dict(dtp=0.9), dict(noise_dropout=0.1), dict(cfg_interval=(0, 500)), dict(cfg_rescale=0.5), dict(v_form="data")):
        with pytest.raises(ValueError, match="learn_sigma"):
            lv_native_option(bad)
        lvd = _diffusion(learn_sigma=True, parameterization="v")
        lvd.set_denoise_fn(None, lambda *a, **k: None)
        with pytest.raises(ValueError, match="learn_sigma"):
            lvd.p_sample_loop("native", (1, 3, 8, 8), dict(sk, num_timesteps=T, **bad))
    lv_native_option(dict(dtp=1, noise_dropout=0, cfg_rescale=0))


# ------------------------------------------------------------------------------------------------- the loss's CPU branch

def _inputs(s, par, seed=0, B=4, Cc=3, hw=(4, 5), decoder="near"):
    """x0 on the 8-bit grid (with exact -1 and +1), v uniform in [-1.5, 1.5], t = (0, 1, T-1, middle); at t == 0 the mean is
    drawn so that |x0 - mu_th| is at most 3 standard deviations ('near') or between 20.5 and 30 ('far': the clamp)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor([0, 1, T - 1, 241][:B])
    x0 = torch.randint(0, 256, (B, Cc) + hw, generator=g).float() / 127.5 - 1.0
    x0.view(B, -1)[:, 0], x0.view(B, -1)[:, 1] = -1.0, 1.0
    noise = torch.randn((B, Cc) + hw, generator=g)
    v = torch.rand((B, Cc) + hw, generator=g) * 3.0 - 1.5
    m = torch.randn((B, Cc) + hw, generator=g)
    # t == 0: m from the wanted d = x0 - mu_th (posterior_mean_coef1[0] == 1, coef2[0] == 0: mu_th = x0p), in float64
    sa, s1 = float(s.sqrt_alphas_cumprod[0]), float(s.sqrt_one_minus_alphas_cumprod[0])
    lv = ((v[0].double() + 1) / 2) * float(s.lv_max_log[0]) + (1 - (v[0].double() + 1) / 2) * float(s.lv_min_log[0])
    k = (torch.rand(v[0].shape, generator=g, dtype=torch.float64) * 2 - 1) * 3.0
    if decoder == "far":
        k = torch.sign(k) * (20.5 + k.abs() / 3.0 * 9.5)
    x0p = x0[0].double() - k * torch.exp(0.5 * lv)
    xt = sa * x0[0].double() + s1 * noise[0].double()
    if par == "x0":
        m0 = x0p
    elif par == "eps":
        m0 = (float(s.sqrt_recip_alphas_cumprod[0]) * xt - x0p) / float(s.sqrt_recipm1_alphas_cumprod[0])
    else:
        m0 = (sa * xt - x0p) / s1
    m[0] = m0.float()
    return torch.cat([m, v], 1), x0, noise, t


def _restate(s, out, x0, noise, t, par, kind, wt=None):
    """float64 restatement of the issue's formulas from the fp32 inputs and buffers: (per_w, per_raw, per_vlb)"""
    f = lambda name: getattr(s, name).double()[t].reshape(-1, 1, 1, 1)
    Cc = x0.shape[1]
    o, x, n = out.double(), x0.double(), noise.double()
    m, v = o[:, :Cc], o[:, Cc:]
    sa, s1 = f("sqrt_alphas_cumprod"), f("sqrt_one_minus_alphas_cumprod")
    target = dict(eps=n, x0=x, v=sa * n - s1 * x)[par]
    dd = m - target
    el = dict(l2=dd * dd, l1=dd.abs(), huber=torch.where(dd.abs() < 1, 0.5 * dd * dd, dd.abs() - 0.5))[kind]
    raw = el.reshape(len(x), -1).mean(1)
    xt = sa * x + s1 * n
    if par == "eps":
        x0p = f("sqrt_recip_alphas_cumprod") * xt - f("sqrt_recipm1_alphas_cumprod") * m
    else:
        x0p = m if par == "x0" else sa * xt - s1 * m
    c1, c2 = f("posterior_mean_coef1"), f("posterior_mean_coef2")
    mu_th, mu_q = c1 * x0p + c2 * xt, c1 * x + c2 * xt
    frac = (v + 1) / 2
    mx, lq = f("lv_max_log"), f("lv_min_log")
    lv = frac * mx + (1 - frac) * lq
    kl = 0.5 * (-1 + lv - lq + torch.exp(lq - lv) + (mu_q - mu_th) ** 2 * torch.exp(-lv)) / LN2
    inv, d = torch.exp(-0.5 * lv), x - mu_th
    phi = lambda u: 0.5 * (1 + torch.tanh(math.sqrt(2 / math.pi) * (u + 0.044715 * u ** 3)))
    cp, cm = phi(inv * (d + 1 / 255)), phi(inv * (d - 1 / 255))
    p = torch.where(x < -0.999, cp, torch.where(x > 0.999, 1 - cm, cp - cm))
    dec = -torch.log(p.clamp(min=1e-12)) / LN2
    L = torch.where((t == 0).reshape(-1, 1, 1, 1), dec, kl)
    near_clamp = ((t == 0).reshape(-1, 1, 1, 1) & (p > 0.5e-12) & (p < 2e-12)).sum()
    w = 1.0 if wt is None else wt.double()[t]
    return raw * w, raw, L.reshape(len(x), -1).mean(1), int(near_clamp)


@pytest.mark.parametrize("decoder", ["near", "far"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("par", PARS)
def test_cpu_branch_against_float64_restatement(par, kind, decoder):
    from sgdm_amd.losses import lv_loss
    d = _diffusion(learn_sigma=True, parameterization=par, loss_type=kind, loss_weighting="min_snr")
    s, h = d.sampler, d.hparams
    out, x0, noise, t = _inputs(s, par, seed=3, decoder=decoder)
    per_w, raw, vlb = lv_loss(s, h, out, x0, noise, t, s.loss_weights)
    w_w, w_raw, w_vlb, near = _restate(s, out, x0, noise, t, par, kind, s.loss_weights)
    assert near == 0                                        # no element within a factor 2 of the clamp with these inputs
    assert _rel(raw, w_raw) < 1e-6 and _rel(per_w, w_w) < 1e-6
    # t > 0 in fp32: the expression cancels where lv ~ lq; its absolute error is a few ulp of the largest term
    assert np.abs(vlb.double().numpy() - w_vlb.numpy()).max() <= 2e-5 * max(1.0, float(w_vlb.abs().max())), (vlb, w_vlb)
    assert _rel(vlb[0], w_vlb[0]) < 1e-6                    # t == 0 runs in double
    if decoder == "far":
        # every interior element clamps at 39.86 bits; the two edge pixels (x0 = -1 / +1) are one-sided and may cost 0 bits
        n = x0[0].numel()
        assert (n - 2) / n * 39.86 < float(w_vlb[0]) <= -math.log(1e-12) / LN2 + 1e-9


@pytest.mark.parametrize("par", PARS)
def test_exact_target_and_min_variance_give_zero_bound(par):
    from sgdm_amd.losses import lv_loss
    d = _diffusion(learn_sigma=True, parameterization=par)
    s, h = d.sampler, d.hparams
    _, x0, noise, t = _inputs(s, par, seed=5)
    sa, s1 = (s._ext(a, t, x0.shape) for a in (s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod))
    target = dict(eps=noise, x0=x0, v=sa * noise - s1 * x0)[par]
    out = torch.cat([target, -torch.ones_like(x0)], 1)
    _, _, vlb = lv_loss(s, h, out, x0, noise, t, None)
    assert float(vlb[1:].abs().max()) <= 1e-6, vlb


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("par", PARS)
def test_gradient_stops_at_the_mean(par, kind):
    d = _diffusion(learn_sigma=True, parameterization=par, loss_type=kind)
    plain = _diffusion(parameterization=par, loss_type=kind)
    out, x0, noise, t = _inputs(d.sampler, par, seed=7)
    out = out.requires_grad_(True)
    d.set_denoise_fn(lambda x, tt: (out, 0.0, {}), None)
    loss, ld = d.train().p_losses(x0, t, noise)
    loss.backward()
    m = out.detach()[:, :3].clone().requires_grad_(True)
    plain.set_denoise_fn(lambda x, tt: (m, 0.0, {}), None)
    l2, ld2 = plain.train().p_losses(x0, t, noise)
    l2.backward()
    assert torch.equal(out.grad[:, :3], m.grad)
    assert float(out.grad[:, 3:].abs().max()) > 0
    assert torch.equal(ld["train/ddpm_loss"], ld2["train/ddpm_loss"]) and torch.equal(ld["train/epoch_stats_y"], ld2["train/epoch_stats_y"])
    assert float(loss.detach()) == pytest.approx(float(ld["train/ddpm_loss"] + d.sampler.vlb_weight * ld["train/vlb"]), rel=1e-6)


def test_gradcheck_of_both_terms():
    from sgdm_amd.losses import lv_decoder_bits, lv_kl_bits
    g = torch.Generator().manual_seed(11)
    r = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)
    mu_th, mu_q = r(12).requires_grad_(True), r(12)
    lq = -3.0 + r(12) * 0.1
    lv = (lq + r(12).abs()).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: lv_kl_bits(a, mu_q, b, lq), (mu_th, lv))
    # the decoder term at the t = 0 scale: sd ~ 0.01, |x0 - mu| at most 3 sd, and the clamped group (gradient 0 on both sides)
    x0 = torch.tensor([-1.0, 1.0] + [(i * 19 % 256) / 127.5 - 1.0 for i in range(10)], dtype=torch.float64)
    lv0 = (-9.5 + r(12) * 0.3).requires_grad_(True)
    for k in ((torch.rand(12, generator=g, dtype=torch.float64) * 2 - 1) * 3.0, torch.full((12,), 25.0, dtype=torch.float64)):
        mu = (x0 - k * torch.exp(0.5 * lv0.detach())).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda a, b: lv_decoder_bits(x0, a, b), (mu, lv0), eps=1e-7, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- calc_bpd

@pytest.mark.parametrize("sched", ["linear", "cosine"])
def test_calc_bpd_on_the_exact_denoiser(sched):
    TT = 50                                                 # a short schedule: calc_bpd evaluates the denoiser T times
    d = _diffusion(learn_sigma=True, num_timesteps=TT, **SCHEDULES[sched])
    g = torch.Generator().manual_seed(2)
    x0 = torch.randint(0, 256, (2, 3, 4, 4), generator=g).float() / 127.5 - 1.0
    noises = {t: torch.randn(2, 3, 4, 4, generator=g) for t in range(TT)}
    seen = []

    def stub(x_t, t):
        seen.append(int(t[0]))
        return torch.cat([noises[int(t[0])], -torch.ones_like(x_t)], 1), 0.0, {}

    d.set_denoise_fn(stub, None)
    out = d.calc_bpd(x0, noise_fn=lambda t: noises[t])
    assert seen == list(reversed(range(TT)))
    vb, prior, total = out["vb"], out["prior_bpd"], out["total_bpd"]
    assert tuple(vb.shape) == (2, TT) and tuple(prior.shape) == (2,) and bool(torch.isfinite(total).all())
    assert float(vb[:, 1:].abs().max()) <= 1e-6
    assert torch.allclose(total, vb[:, 0] + prior, rtol=0, atol=1e-5)
    a = float(d.sampler.alphas_cumprod[TT - 1])
    want = (0.5 * (-1 - math.log(1 - a) + (1 - a) + a * x0.double() ** 2)).reshape(2, -1).mean(1) / LN2
    assert _rel(prior, want) < 1e-6
    with pytest.raises(ValueError, match="learn_sigma"):
        _diffusion().calc_bpd(x0)


# --------------------------------------------------------------------------------------------------------------- hparams

def test_hparam_validation_and_the_unchanged_default():
    with pytest.raises(ValueError, match="v_posterior"):
        _diffusion(learn_sigma=True, v_posterior=0.5)
    with pytest.raises(ValueError, match="out_channels"):
        _diffusion(learn_sigma=True, out_channels=3, channels=3)
    with pytest.raises(ValueError, match="vlb_weight"):
        _diffusion(learn_sigma=True, vlb_weight=-1.0)
    narrow, wide = _unet(3), _unet(6)
    with pytest.raises(ValueError, match="out_channels"):
        _diffusion(learn_sigma=True).set_denoise_fn(narrow.forward, narrow.forward_with_cond_scale)
    _diffusion(learn_sigma=True).set_denoise_fn(wide.forward, wide.forward_with_cond_scale)
    # a 3-channel output under learn_sigma is refused by p_losses too (a generic denoiser)
    d = _diffusion(learn_sigma=True)
    d.set_denoise_fn(lambda x, t: (x, 0.0, {}), None)
    with pytest.raises(ValueError, match="channels"):
        d.p_losses(torch.zeros(1, 3, 4, 4), torch.tensor([3]), torch.zeros(1, 3, 4, 4))
    # hparam absent (or False): no buffers, no 'vlb' entry, the loss of the chain as it always was
    for extra in ({}, dict(learn_sigma=False)):
        for par in PARS:
            for kind in KINDS:
                p = _diffusion(parameterization=par, loss_type=kind, **extra).train()
                assert not hasattr(p.sampler, "lv_max_log") and not hasattr(p.sampler, "lv_min_log") and not p.sampler.learn_sigma
                g = torch.Generator().manual_seed(1)
                x0, noise, m = (torch.randn(3, 3, 4, 4, generator=g) for _ in range(3))
                t = torch.tensor([0, 500, 999])
                p.set_denoise_fn(lambda x, tt: (m, 0.0, {}), None)
                loss, ld = p.p_losses(x0, t, noise)
                s = p.sampler
                sa, s1 = (s._ext(a, t, x0.shape) for a in (s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod))
                target = dict(eps=noise, x0=x0, v=sa * noise - s1 * x0)[par]
                if kind == "l2":
                    want = ((target - m) ** 2).reshape(3, -1).mean(1)
                elif kind == "l1":
                    want = (target - m).abs().reshape(3, -1).mean(1)
                else:
                    want = torch.nn.functional.smooth_l1_loss(target, m, reduction="none").reshape(3, -1).mean(1)
                assert torch.equal(loss, want.mean()) and "train/vlb" not in ld
                assert torch.equal(ld["train/epoch_stats_y"], want)


def test_new_entries_are_declared_and_bound():
    from sgdm_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()
    for name in ("sgd_lv_loss_fwd", "sgd_lv_loss_bwd", "sgd_ddpm_lv_step"):
        assert re.search(rf"\bint {name}\(", header) and name in L.SIGNATURES
    assert L.ABI_VERSION == 25 and "#define SGD_ABI_VERSION 25" in header         # additive entries: the ABI number stays
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgdm_build_lv", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for f in ("lvloss.hip", "lvstep.hip"):
        assert mod.FILE_FLAGS[f] == ["-ffp-contract=off"] and os.path.exists(os.path.join(PKG, "csrc", f))
