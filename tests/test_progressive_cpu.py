"""Progressive distillation (hparam progressive_steps = K; Salimans & Ho 2022, Algorithm 2 = stage 2 of Meng et al. 2023) where it
needs no GPU: the row table against a float64 restatement that literally takes two DDIM steps of the 2K-step trailing grid
(make_ddim_sampling_parameters, eta 0, no clip) and one step of the K-step grid with the target the rows give; the grid snapping;
the option's refusals; progressive_next_stage; p_losses on the generic path with stub callables against float64; the sampling
defaults; the binding of the three new entry points.  The reference has no counterpart; the expected values are the formulas
restated here.

Bounds: 1e-12 relative on z_e for the rows (float64 on both sides; measured at most 3.4e-16); 1e-6 relative on the loss -- the
torch chain forms the target in fp32 from rows rounded once (every |d| <= 1, so ~1e-7 of the target) and the loss is an fp32 mean of
O(1) terms; the float64 restatement starts from the float64 rows and the same fp32 inputs."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, load_json

T, W = 1000, 2.0
KS = (1, 2, 4, 8, 50)


def _diffusion(**kw):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cpu", **dict(bench.MODEL_PARAMS, **kw))


def _ac(zero_terminal, par, steps=T):
    """the schedule's own fp32 alphas_cumprod buffer, in float64"""
    d = _diffusion(parameterization=par, zero_terminal_snr=zero_terminal, num_timesteps=steps)
    return d.sampler.alphas_cumprod.double().numpy()


# ------------------------------------------------------------------------------------------------------------------ rows

def _ddim_step(par, z, y, a_t, a_prev):
    """one deterministic DDIM step (eta 0, no clip) in float64 from the cumulative alphas of the step, as the sampler does it:
    the x0 and eps the network output stands for, then sqrt(a_prev) x0 + sqrt(1 - a_prev) eps"""
    al, sg = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    if par == "eps":
        x0, eps = (z - sg * y) / al, y
    elif par == "x0":
        x0, eps = y, (z - al * y) / sg
    else:
        x0, eps = al * z - sg * y, sg * z + al * y
    return np.sqrt(a_prev) * x0 + np.sqrt(1.0 - a_prev) * eps


CASES = [(par, False) for par in ("eps", "x0", "v")] + [(par, True) for par in ("x0", "v")]
# every K of KS needs num_timesteps % (2 K) == 0: 1000 = 2^3 5^3 has no multiple of 16, so K = 8 runs on a schedule of 800
# timesteps (where every K of KS divides), the others on both
GRIDS = [(1000, k) for k in KS if 1000 % (2 * k) == 0] + [(800, k) for k in KS]
assert sorted({k for _, k in GRIDS}) == sorted(KS) and all(n % (2 * k) == 0 for n, k in GRIDS)


@pytest.mark.parametrize("T,K", GRIDS)
@pytest.mark.parametrize("par,zero_terminal", CASES)
def test_rows_reproduce_two_teacher_steps_in_float64(par, zero_terminal, T, K):
    from sgdm_amd.diffusion import make_ddim_sampling_parameters, make_ddim_timesteps, progressive_rows
    ac = _ac(zero_terminal, par, T)
    assert ac.shape == (T,)
    if zero_terminal:
        assert ac[-1] == 0.0
    rows = progressive_rows(torch.tensor(ac), K, par)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (K, 5) and bool(torch.isfinite(rows).all())
    rows = rows.numpy()
    # the teacher's grid and the student's, with the sampler's own a / a_prev
    g2 = make_ddim_timesteps("uniform", 2 * K, T, timestep_spacing="trailing")
    g1 = make_ddim_timesteps("uniform", K, T, timestep_spacing="trailing")
    _, a2, p2 = make_ddim_sampling_parameters(ac, g2, 0.0)
    _, a1, p1 = make_ddim_sampling_parameters(ac, g1, 0.0)
    assert np.array_equal(g2[1::2], g1) and np.array_equal(a2[1::2], a1) and np.array_equal(p2[0::2], p1)
    assert p1[0] == ac[0]                                                # e = -1 reads alphas_cumprod[0]
    rng = np.random.default_rng(K)
    worst_e = worst_m = 0.0
    for i in range(K):
        z, y1, y2 = rng.standard_normal((3, 257))
        z_m = _ddim_step(par, z, y1, a2[2 * i + 1], p2[2 * i + 1])      # t -> m
        assert p2[2 * i + 1] == a2[2 * i]
        z_e = _ddim_step(par, z_m, y2, a2[2 * i], p2[2 * i])             # m -> e
        a_1, b_1, d0, d1, d2 = rows[i]
        got_m = a_1 * z + b_1 * y1
        got_e = _ddim_step(par, z, d0 * z + d1 * y1 + d2 * y2, a1[i], p1[i])     # ONE step t -> e with the rows' target
        worst_m = max(worst_m, float(np.linalg.norm(got_m - z_m) / np.linalg.norm(z_m)))
        worst_e = max(worst_e, float(np.linalg.norm(got_e - z_e) / np.linalg.norm(z_e)))
    print(f"progressive rows {par} zero-terminal {zero_terminal} T {T} K {K}: rel-L2 z_m {worst_m:.2e}, z_e {worst_e:.2e}")
    assert worst_m <= 1e-12 and worst_e <= 1e-12


@pytest.mark.parametrize("par,zero_terminal", CASES)
def test_coefficients_are_bounded_and_d0_is_zero_off_v(par, zero_terminal):
    from sgdm_amd.diffusion import progressive_rows
    ac = torch.tensor(_ac(zero_terminal, par))
    for K in [k for k in range(1, 501) if T % (2 * k) == 0]:
        d = progressive_rows(ac, K, par)[:, 2:]
        assert float(d.abs().max()) <= 1.0, (K, float(d.abs().max()))
        if par != "v":
            assert bool((d[:, 0] == 0).all())
            assert float((d[:, 1] + d[:, 2] - 1.0).abs().max()) <= 1e-14
        else:
            assert bool((d[:, 0] <= 0).all()) and bool((d[:, 0] < 0).any())    # (0 where m == e: K = T / 2, i = 0)


def test_rows_refuse_what_they_cannot_form():
    from sgdm_amd.diffusion import progressive_rows
    ac = torch.tensor(_ac(False, "v"))
    with pytest.raises(ValueError, match="progressive_rows"):
        progressive_rows(ac, 3, "v")
    with pytest.raises(ValueError, match="progressive_rows"):
        progressive_rows(ac, 0, "v")
    with pytest.raises(NotImplementedError):
        progressive_rows(ac, 4, "mu")
    with pytest.raises(ValueError, match="divides by"):
        progressive_rows(torch.tensor(_ac(True, "v")), 4, "eps")


# ------------------------------------------------------------------------------------------------------------------ grid

def test_snapped_grid_is_the_trailing_grid_and_stays_uniform():
    from sgdm_amd.diffusion import make_ddim_timesteps, progressive_grid
    t = torch.arange(T)
    seen = 0
    for K in range(1, T + 1):
        if T % (2 * K):
            continue
        idx, snapped = progressive_grid(t, K, T)
        grid, counts = torch.unique(snapped, return_counts=True)
        assert np.array_equal(grid.numpy(), make_ddim_timesteps("uniform", K, T, timestep_spacing="trailing")), K
        assert bool((counts == T // K).all()) and int(idx.min()) == 0 and int(idx.max()) == K - 1
        assert torch.equal(snapped, (idx + 1) * (T // K) - 1) and bool((snapped >= t).all())
        seen += 1
    assert seen == 12                                   # the divisors of 500


# ---------------------------------------------------------------------------------------------------------------- option

class _H:
    def __init__(self, **kw):
        self.num_timesteps, self.parameterization = T, "eps"
        self.__dict__.update(kw)


@pytest.mark.parametrize("K", [0, -4, 3, 7, 8, 1000, 4.0, "4", True])
def test_option_refuses_a_step_count_that_is_no_positive_divisor(K):
    from sgdm_amd.diffusion import progressive_option
    with pytest.raises(ValueError, match=r"progressive_steps=.*positive int K with num_timesteps % \(2 K\) == 0"):
        progressive_option(_H(progressive_steps=K))
    with pytest.raises(ValueError, match="progressive_steps="):
        _diffusion(progressive_steps=K)


def test_option_refuses_learned_variance():
    from sgdm_amd.diffusion import progressive_option
    with pytest.raises(ValueError, match="progressive_steps with learn_sigma"):
        progressive_option(_H(progressive_steps=4, learn_sigma=True))
    with pytest.raises(ValueError, match="progressive_steps with learn_sigma"):
        _diffusion(progressive_steps=4, learn_sigma=True, out_channels=6, channels=3)


def test_option_refuses_eps_on_a_zero_terminal_snr_schedule():
    from sgdm_amd.diffusion import progressive_option
    with pytest.raises(ValueError, match="progressive_steps with parameterization='eps' on a zero_terminal_snr"):
        progressive_option(_H(progressive_steps=4, zero_terminal_snr=True))
    assert progressive_option(_H(progressive_steps=4, zero_terminal_snr=True, parameterization="v")) == 4
    assert progressive_option(_H(progressive_steps=4, zero_terminal_snr=True, parameterization="x0")) == 4


def test_option_values():
    from sgdm_amd.diffusion import progressive_option
    assert progressive_option(_H()) is None and progressive_option(_H(progressive_steps=None)) is None
    for K in (1, 2, 4, 5, 10, 50, 250, 500, np.int64(4)):
        got = progressive_option(_H(progressive_steps=K))
        assert got == K and type(got) is int
    assert _diffusion().progressive is None and _diffusion(progressive_steps=None).progressive is None
    assert _diffusion(progressive_steps=4).progressive == 4
    assert _diffusion(progressive_steps=8, num_timesteps=800).progressive == 8
    d = _diffusion(progressive_steps=4, distill_guidance=W, distill_rescale=0.5)
    assert d.progressive == 4 and d.distill == (W, 0.5)


# ------------------------------------------------------------------------------------------------------------ next stage

def _cpu_unet():
    """the small drop-in UNet, on the CPU (it is copied and looked at, never evaluated)"""
    from sgdm_amd.unet import UNetModel

    class AD(dict):
        __getattr__ = dict.__getitem__
    entry = load_json("unet_index.json")["uf_clusterlayout_c32_s16"]
    kw = dict(entry["ctor"])
    cond = AD(scale_type="imagen")
    if entry["layout_dim"]:
        cond[kw["condition_method"]] = AD(layout_dim=entry["layout_dim"])
    return UNetModel(condition=cond, **kw).train()


def test_next_stage_freezes_the_student_and_halves_the_steps():
    from sgdm_amd.train import progressive_next_stage
    from sgdm_amd.unet import UNetModelBase
    m = _cpu_unet()
    d = _diffusion(progressive_steps=4, distill_guidance=W, distill_rescale=0.5, parameterization="v")
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    first = object()
    d.set_distill_teacher(first)
    d.__dict__["_pd_rows"], d.__dict__["_distill_runner"] = {"stale": 1}, "stale"
    names = sorted(d.state_dict())
    assert progressive_next_stage(d) == 2
    h = d.hparams
    assert (d.progressive, h.progressive_steps) == (2, 2)
    assert d.distill is None and h.distill_guidance is None and h.distill_rescale is None and h.guidance_distilled is True
    assert "_pd_rows" not in d.__dict__ and "_distill_runner" not in d.__dict__
    teacher = d._distill_teacher
    assert isinstance(teacher, UNetModelBase) and teacher is not m and teacher is not first
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters()) and m.training
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(teacher.parameters(), m.parameters()))
    assert sorted(d.state_dict()) == names                                  # the teacher reaches no state_dict
    # the student moves on; the next stage freezes it as it then is, in the arithmetic mode asked for
    with torch.no_grad():
        next(iter(m.parameters())).add_(1.0)
    assert progressive_next_stage(d, hip_precision="f16") == 1 and d.progressive == 1
    t2 = d._distill_teacher
    assert t2 is not teacher and t2.hip_precision == "f16" and torch.equal(next(iter(t2.parameters())), next(iter(m.parameters())))
    assert not torch.equal(next(iter(teacher.parameters())), next(iter(m.parameters())))
    with pytest.raises(ValueError, match="progressive_steps is 1"):
        progressive_next_stage(d)
    assert d.progressive == 1 and d.hparams.progressive_steps == 1


def test_next_stage_refusals_change_nothing():
    from sgdm_amd.train import progressive_next_stage
    m = _cpu_unet()
    d = _diffusion(progressive_steps=5, distill_guidance=W)                 # 1000 % 10 == 0, but 5 has no half
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    with pytest.raises(ValueError, match="cannot be halved"):
        progressive_next_stage(d)
    assert d.progressive == 5 and d.distill == (W, 0.0) and getattr(d, "_distill_teacher", None) is None
    off = _diffusion()
    off.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    with pytest.raises(ValueError, match="progressive_steps is not set"):
        progressive_next_stage(off)
    generic = _diffusion(progressive_steps=4, distill_guidance=W)
    generic.set_denoise_fn(lambda x, t, **kw: (x, 0.0, {}), None)
    with pytest.raises(TypeError, match="drop-in UNet"):
        progressive_next_stage(generic)
    assert generic.progressive == 4 and generic.distill == (W, 0.0) and generic.hparams.progressive_steps == 4


# ------------------------------------------------------------------------------------------------------ p_losses on the CPU

def _inputs(B=6):
    g = torch.Generator().manual_seed(29)
    x0, noise = torch.randn(B, 3, 8, 8, generator=g), torch.randn(B, 3, 8, 8, generator=g)
    out = 1.5 * torch.randn(B, 3, 8, 8, generator=g)            # |d| on both sides of huber's 1
    return x0, noise, out, torch.tensor([0, 999, 500, 37, 640, 250])


class _Student:
    def __init__(self, out):
        self.out, self.out_channels, self.calls = out, out.shape[1], []

    def __call__(self, x, t, *a, **kw):
        self.calls.append(dict(x=x.clone(), t=t.clone(), kw=kw))
        return self.out, 0.0, dict()


def _net(x, t, w, cond):
    """a smooth function of everything a teacher sees, in the dtype of ``x``"""
    tt = (t.to(x.dtype) / T).reshape(-1, 1, 1, 1)
    return torch.tanh(0.7 * x + tt) * (1.0 + 0.25 * w) + 0.1 * cond.to(x.dtype).reshape(-1, 1, 1, 1) * x.flip(1)


class _Teacher:
    """a plain callable: guided=True takes (x, t, cond_scale, cond=...), else (x, t, cond=...)"""

    def __init__(self, guided):
        self.guided, self.calls = guided, []

    def __call__(self, x, t, *a, cond=None, **kw):
        w = a[0] if self.guided else 0.0
        assert len(a) == int(self.guided)
        self.calls.append(dict(x=x.clone(), t=t.clone(), w=w, cond=cond, grad=torch.is_grad_enabled()))
        return _net(x, t, w, cond)


def _per64(loss_type, out, target):
    diff = out.double() - target.double()
    if loss_type == "l2":
        el = diff ** 2
    elif loss_type == "l1":
        el = diff.abs()
    else:
        el = torch.where(diff.abs() < 1, 0.5 * diff ** 2, diff.abs() - 0.5)
    return el.reshape(len(out), -1).mean(1)


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("weighting", [None, "trunc_snr"])
@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
@pytest.mark.parametrize("par,K", [("eps", 4), ("x0", 10), ("v", 4)])
def test_loss_is_against_the_two_step_target(par, K, loss_type, weighting, guided):
    from sgdm_amd.diffusion import progressive_rows
    x0, noise, out, t = _inputs()
    hp = dict(distill_guidance=W) if guided else {}
    d = _diffusion(parameterization=par, loss_type=loss_type, loss_weighting=weighting, progressive_steps=K, **hp).train()
    student, teacher = _Student(out), _Teacher(guided)
    d.set_denoise_fn(student, None)
    d.set_distill_teacher(teacher)
    cond = torch.arange(6.0).view(6, 1)
    loss, ld = d.p_losses(x0, t, noise, cond=cond, cond_drop_prob=0.5)
    # float64 restatement from the same fp32 inputs and the float64 rows
    st = T // K
    idx = t // st
    ts, tm = (idx + 1) * st - 1, (idx + 1) * st - 1 - st // 2
    assert int(idx.min()) == 0 and int(idx.max()) == K - 1                 # both ends of the grid in one batch
    s = d.sampler
    x = s.q_sample(x0, noise, ts)
    r = progressive_rows(s.alphas_cumprod, K, par)[idx]
    a1, b1, d0, d1, d2 = (r[:, k].reshape(-1, 1, 1, 1) for k in range(5))
    w = W if guided else 0.0
    y1 = _net(x.double(), ts, w, cond)
    z_m = a1 * x.double() + b1 * y1
    y2 = _net(z_m, tm, w, cond)
    target = d0 * x.double() + d1 * y1 + d2 * y2
    per = _per64(loss_type, out, target)
    wt = s.loss_weights.double()[ts] if weighting else torch.ones(6, dtype=torch.float64)
    want = (wt * per).mean()
    err = abs(float(loss) - float(want)) / float(want)
    print(f"progressive p_losses {par} K {K} {loss_type} {weighting} guided {guided}: loss {float(loss):.6e}, rel err {err:.2e}")
    assert err <= 1e-6
    keys = ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    assert sorted(ld) == sorted(keys + (["train/ddpm_loss_raw"] if weighting else []))
    assert torch.allclose(ld["train/epoch_stats_y"].double(), per, rtol=1e-6, atol=0)
    assert torch.equal(ld["train/epoch_stats_x"], ts)                       # the SNAPPED timestep is what is logged
    # it is neither the trained target nor the teacher's one-step output
    assert float((target - y1).abs().max()) > 1e-2 and abs(float(loss) - float((wt * _per64(loss_type, out, y1)).mean())) > 1e-4 * float(want)
    # teacher at (z_t, t), then at (z_m, m), under no_grad with the caller's cond; the student once, at the snapped t, with
    # cond_drop_prob forced to 0.0
    assert len(teacher.calls) == 2 and len(student.calls) == 1
    c1, c2, sc = teacher.calls[0], teacher.calls[1], student.calls[0]
    assert torch.equal(c1["x"], x) and torch.equal(c1["t"], ts) and torch.equal(sc["x"], x) and torch.equal(sc["t"], ts)
    assert torch.equal(c2["t"], tm) and float((c2["x"].double() - z_m).abs().max()) <= 1e-5 * float(z_m.abs().max())
    assert all(c["grad"] is False and torch.equal(c["cond"], cond) and c["w"] == w for c in (c1, c2))
    assert sc["kw"]["cond_drop_prob"] == 0.0 and torch.equal(sc["kw"]["cond"], cond)
    # validation: forward only, the val/ keys
    d.eval()
    with torch.no_grad():
        vloss, vd = d.p_losses(x0, t, noise, cond=cond)
    assert sorted(vd) == sorted(["val/ddpm_loss", "val/loss"] + (["val/ddpm_loss_raw"] if weighting else []))
    assert float(vloss) == float(loss)


def test_gradient_reaches_the_student_output_only():
    x0, noise, out, t = _inputs()
    out = out.clone().requires_grad_(True)
    d = _diffusion(parameterization="v", progressive_steps=4).train()
    seen = {}

    def teacher(x, tt, cond=None):
        seen.setdefault("y", []).append(_net(x, tt, 0.0, cond))
        return seen["y"][-1], 0.0, dict()                                   # a model's triple is accepted
    d.set_denoise_fn(_Student(out), None)
    d.set_distill_teacher(teacher)
    loss, _ = d.p_losses(x0, t, noise, cond=torch.zeros(6, 1))
    loss.backward()
    assert len(seen["y"]) == 2 and out.grad is not None and float(out.grad.abs().max()) > 0
    assert not any(y.requires_grad for y in seen["y"])


def test_refusals_come_before_either_model_is_called():
    x0, noise, out, t = _inputs()

    def refused(match, teacher, **ukw):
        d = _diffusion(progressive_steps=4).train()
        student = _Student(out)
        d.set_denoise_fn(student, None)
        if teacher is not None:
            d.set_distill_teacher(teacher)
        with pytest.raises(ValueError, match=match):
            d.p_losses(x0, t, noise, cond=torch.zeros(6, 1), **ukw)
        assert not student.calls and not getattr(teacher, "calls", None)

    refused("progressive_steps is set but there is no teacher", None)
    refused("cond_drop_mask", _Teacher(False), cond_drop_mask=torch.zeros(6, dtype=torch.bool))
    lv = _Teacher(False)
    lv.learn_sigma = True
    refused("learn_sigma", lv)
    wide = _Teacher(False)
    wide.out_channels = 6
    refused("output channels", wide)
    frozen = torch.nn.Linear(2, 2)                                           # a module teacher: the checks of stage 1
    refused("train mode", frozen)
    refused("require grad", frozen.eval())


def test_without_the_hparam_nothing_changes():
    import bench
    assert "progressive_steps" not in bench.MODEL_PARAMS
    x0, noise, out, t = _inputs()
    runs = []
    for kw in ({}, dict(progressive_steps=None)):
        d = _diffusion(parameterization="v", **kw).train()
        assert d.progressive is None
        student = _Student(out)
        d.set_denoise_fn(student, None)
        d.set_distill_teacher(_Teacher(False))                              # never called without the hparam
        runs.append(d.p_losses(x0, t, noise, cond_drop_prob=0.5) + (student, d._distill_teacher))
    (loss, ld, st, tch), (loss_n, ld_n, _, tch_n) = runs
    assert torch.equal(loss, loss_n) and all(torch.equal(ld[k], ld_n[k]) for k in ld) and not tch.calls and not tch_n.calls
    assert torch.equal(ld["train/epoch_stats_x"], t) and torch.equal(st.calls[0]["t"], t)      # t as given: nothing snapped
    assert st.calls[0]["kw"] == dict(cond_drop_prob=0.5)
    s = _diffusion(parameterization="v").sampler
    sa, s1 = s.sqrt_alphas_cumprod[t].view(6, 1, 1, 1).double(), s.sqrt_one_minus_alphas_cumprod[t].view(6, 1, 1, 1).double()
    assert float(loss) == pytest.approx(float(_per64("l2", out, sa * noise.double() - s1 * x0.double()).mean()), rel=1e-6)


def test_loss_path_of_a_progressive_step():
    from sgdm_amd.losses import _loss_path
    unet, w = object(), object()
    for distilling in (False, True):
        for weights in (None, w):
            assert _loss_path(False, distilling, unet, weights, True, True) == "progressive_fused"
            assert _loss_path(False, distilling, None, weights, True, True) == "torch"
            assert _loss_path(False, distilling, None, weights, False, progressive=True) == "torch"
    assert _loss_path(False, True, unet, None, True) == "distill_fused"     # the default: not progressive
    assert _loss_path(False, True, unet, None, True, False) == "distill_fused"


# ---------------------------------------------------------------------------------------------------------------- sampling

def test_sampling_defaults_walk_the_students_grid(monkeypatch):
    seen = {}

    def sample(shape, sampling_kwargs=None, **kw):
        seen.clear()
        seen.update(sampling_kwargs)
        z = torch.zeros(shape)
        return z, dict(pred_x0=z)
    keys = ("num_timesteps", "ddim_eta", "timestep_spacing", "cfg_distilled")
    want = dict(num_timesteps=4, ddim_eta=0, timestep_spacing="trailing", cfg_distilled=True)
    d = _diffusion(progressive_steps=4)
    d.set_denoise_fn(None, lambda *a, **k: None)
    for method in ("ddim", "dpmsolver", "pndm", "plms"):
        monkeypatch.setattr(d.sampler_list[method], "sample", sample)
    for method in ("ddim", "dpmsolver"):
        d.p_sample_loop(method, (1, 3, 4, 4), {})
        assert {k: seen.get(k) for k in keys} == want, method
        # an explicit kwarg still wins, each on its own
        for k, v in dict(num_timesteps=8, ddim_eta=0.5, timestep_spacing="leading", cfg_distilled=False).items():
            d.p_sample_loop(method, (1, 3, 4, 4), {k: v})
            assert {j: seen.get(j) for j in keys} == dict(want, **{k: v}), (method, k)
    for method in ("pndm", "plms"):                                          # no defaults for the other samplers
        d.p_sample_loop(method, (1, 3, 4, 4), dict(num_timesteps=6))
        assert seen["num_timesteps"] == 6 and not any(k in seen for k in keys[1:]), method
    plain = _diffusion()
    plain.set_denoise_fn(None, lambda *a, **k: None)
    monkeypatch.setattr(plain.sampler_list["ddim"], "sample", sample)
    plain.p_sample_loop("ddim", (1, 3, 4, 4), dict(num_timesteps=6))
    assert seen["num_timesteps"] == 6 and not any(k in seen for k in keys[1:])


# ----------------------------------------------------------------------------------------------------------------- binding

def test_binding_declares_the_three_entries_and_the_abi_stays():
    import ctypes as C
    from sgdm_amd import _lib as L
    txt = open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()
    assert int(re.search(r"#define SGD_ABI_VERSION (\d+)", txt).group(1)) == L.ABI_VERSION == 25
    assert re.search(r"typedef struct sgd_pd_row \{ float a1, b1, d0, d1, d2, pad0, pad1, pad2; \} sgd_pd_row;", txt)
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    for name, nargs in (("sgd_pd_half_step", 12), ("sgd_pd_loss_fwd", 16), ("sgd_pd_loss_bwd", 17)):
        res, args = L.SIGNATURES[name]
        proto = re.search(r"^int %s\(([^;]*)\);" % name, txt, flags=re.M).group(1)
        decl = [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]
        assert res is C.c_int32 and len(args) == len(decl) == nargs
        for a, d in zip(args, decl):                                        # pointers where the header has pointers, else the scalar
            if "*" in d:
                assert a in (C.c_void_p, L.dvp), (name, d)
            else:
                assert a is ctype[d.split()[0]], (name, d)
        names = [d.split()[-1].lstrip("*") for d in decl]
        for dev_only in ("w_dev", "idx", "rows", "gper"):                   # what the kernels dereference: never host memory
            if dev_only in names:
                assert args[names.index(dev_only)] is L.dvp, (name, dev_only)
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgdm_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "progressive.hip" in b._sources() and b.FILE_FLAGS["progressive.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(PKG, "csrc", "progressive.hip")).read()
    assert '#include "loss_common.h"' in src and '#include "sampler_common.h"' in src
