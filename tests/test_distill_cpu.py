"""Guidance distillation (hparams distill_guidance / distill_rescale, LatentDiffusion.set_distill_teacher, sampling kwarg
cfg_distilled; Meng et al. 2023, stage 1) where it needs no GPU: p_losses on the generic path with stub callables against a
float64 restatement of loss(student_out, guided(teacher halves, w)), the refusals -- raised before either stub is called --,
the unchanged path without the hparam, the teacher's isolation from parameters() / state_dict(), the sampling kwarg's checks
and the binding of the two new entry points.  The reference has no counterpart; the expected values are the formulas restated
here.

Bound: 1e-6 relative on the per-sample loss -- the stub teacher forms the guided target in fp32 (two rounded products and a
sum, ~1e-7 of the target) and the loss is an fp32 mean of O(1) terms; the float64 restatement starts from the same fp32
halves."""
import os
import re

import pytest
import torch

from conftest import PKG, ROOT

T, W = 1000, 2.0


def _diffusion(**kw):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cpu", **dict(bench.MODEL_PARAMS, **kw))


def _inputs(B=5):
    g = torch.Generator().manual_seed(23)
    x0, noise = torch.randn(B, 3, 8, 8, generator=g), torch.randn(B, 3, 8, 8, generator=g)
    out = 1.5 * torch.randn(B, 3, 8, 8, generator=g)            # |d| on both sides of huber's 1
    tc, tu = torch.randn(B, 3, 8, 8, generator=g), torch.randn(B, 3, 8, 8, generator=g)
    return x0, noise, out, tc, tu, torch.tensor([0, 999, 500, 37, 640])


def _guided(scale_type, tc, tu, w):
    return (1 - w) * tu + w * tc if scale_type == "imagen" else (1 + w) * tc - w * tu


class _Student:
    """a callable denoiser that records what reaches it"""

    def __init__(self, out, out_channels=3):
        self.out, self.out_channels, self.calls = out, out_channels, []

    def __call__(self, x, t, *a, **kw):
        self.calls.append(dict(x=x.clone(), kw=kw))
        return self.out, 0.0, dict()


class _Teacher(torch.nn.Module):
    """forward_with_cond_scale semantics over two fixed halves; a real module with a parameter, frozen and in eval mode"""

    def __init__(self, scale_type, tc, tu, out_channels=3):
        super().__init__()
        self.scale_type, self.tc, self.tu, self.out_channels, self.calls = scale_type, tc, tu, out_channels, []
        self.weight = torch.nn.Parameter(torch.full((7,), 3.25))
        self.eval().requires_grad_(False)

    def forward_with_cond_scale(self, x, t, cond_scale, cond=None, **kw):
        self.calls.append(dict(x=x.clone(), w=cond_scale, cond=cond, grad=torch.is_grad_enabled()))
        return _guided(self.scale_type, self.tc, self.tu, cond_scale)


def _per64(loss_type, out, target):
    diff = out.double() - target.double()
    if loss_type == "l2":
        el = diff ** 2
    elif loss_type == "l1":
        el = diff.abs()
    else:
        el = torch.where(diff.abs() < 1, 0.5 * diff ** 2, diff.abs() - 0.5)
    return el.reshape(len(out), -1).mean(1)


# ------------------------------------------------------------------------------------------------------ p_losses on the CPU

@pytest.mark.parametrize("weighting", [None, "min_snr"])
@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
@pytest.mark.parametrize("par", ["eps", "x0", "v"])
@pytest.mark.parametrize("scale_type", ["imagen", "cfg"])
def test_loss_is_against_the_guided_teacher_output(scale_type, par, loss_type, weighting):
    x0, noise, out, tc, tu, t = _inputs()
    d = _diffusion(parameterization=par, loss_type=loss_type, loss_weighting=weighting, distill_guidance=W).train()
    student, teacher = _Student(out), _Teacher(scale_type, tc, tu)
    d.set_denoise_fn(student, None)
    d.set_distill_teacher(teacher)
    cond = torch.arange(5.0).view(5, 1)
    loss, ld = d.p_losses(x0, t, noise, cond=cond, cond_drop_prob=0.5)
    per = _per64(loss_type, out, _guided(scale_type, tc.double(), tu.double(), W))
    w = d.sampler.loss_weights.double()[t] if weighting else torch.ones(5, dtype=torch.float64)
    want = (w * per).mean()
    assert abs(float(loss) - float(want)) <= 1e-6 * float(want)
    keys = ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    assert sorted(ld) == sorted(keys + (["train/ddpm_loss_raw"] if weighting else []))          # today's keys
    assert torch.allclose(ld["train/epoch_stats_y"].double(), per, rtol=1e-6, atol=0)          # the UNWEIGHTED per-sample loss
    # not the trained target of the parameterization, and not the conditional half alone
    s = d.sampler
    sa, s1 = s.sqrt_alphas_cumprod[t].view(5, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod[t].view(5, 1, 1, 1)
    plain = _per64(loss_type, out, dict(eps=noise, x0=x0, v=sa * noise - s1 * x0)[par])
    assert abs(float(loss) - float((w * plain).mean())) > 1e-3 * float(want)
    assert abs(float(loss) - float((w * _per64(loss_type, out, tc)).mean())) > 1e-3 * float(want)
    # one call each on the same x_noisy; the teacher under no_grad at weight w with the caller's cond; the student with the
    # caller's cond and cond_drop_prob forced to 0.0
    assert len(teacher.calls) == len(student.calls) == 1
    tcall, scall = teacher.calls[0], student.calls[0]
    assert torch.equal(tcall["x"], scall["x"]) and torch.equal(tcall["x"], s.q_sample(x0, noise, t))
    assert tcall["w"] == W and tcall["grad"] is False and torch.equal(tcall["cond"], cond)
    assert scall["kw"]["cond_drop_prob"] == 0.0 and isinstance(scall["kw"]["cond_drop_prob"], float)
    assert torch.equal(scall["kw"]["cond"], cond)
    # validation: the val/ keys
    d.eval()
    with torch.no_grad():
        vloss, vd = d.p_losses(x0, t, noise, cond=cond)
    assert sorted(vd) == sorted(["val/ddpm_loss", "val/loss"] + (["val/ddpm_loss_raw"] if weighting else []))
    assert float(vloss) == float(loss)


def test_gradient_reaches_the_student_output_only():
    x0, noise, out, tc, tu, t = _inputs()
    out = out.clone().requires_grad_(True)
    d = _diffusion(distill_guidance=W).train()
    teacher = _Teacher("cfg", tc, tu)
    d.set_denoise_fn(_Student(out), None)
    d.set_distill_teacher(teacher)
    loss, _ = d.p_losses(x0, t, noise)
    loss.backward()
    want = 2.0 * (out.detach().double() - _guided("cfg", tc.double(), tu.double(), W)) / (out[0].numel() * len(out))
    assert torch.allclose(out.grad.double(), want, rtol=1e-5, atol=1e-9)
    assert teacher.weight.grad is None


@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
@pytest.mark.parametrize("par", ["eps", "x0", "v"])
def test_without_the_hparam_nothing_changes(par, loss_type):
    import bench
    assert not any(k.startswith("distill") or k == "guidance_distilled" for k in bench.MODEL_PARAMS)
    x0, noise, out, tc, tu, t = _inputs()
    runs = []
    for kw in ({}, dict(distill_guidance=None)):
        d = _diffusion(parameterization=par, loss_type=loss_type, **kw).train()
        assert d.distill is None
        student = _Student(out)
        d.set_denoise_fn(student, None)
        runs.append(d.p_losses(x0, t, noise, cond_drop_prob=0.5) + (student,))
    (loss, ld, st), (loss_n, ld_n, _) = runs
    assert sorted(ld) == sorted(ld_n) == ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    assert torch.equal(loss, loss_n) and all(torch.equal(ld[k], ld_n[k]) for k in ld)
    assert st.calls[0]["kw"] == dict(cond_drop_prob=0.5)                     # the caller's kwargs, untouched
    # the restated plain loss, as before the feature
    s = _diffusion(parameterization=par).sampler
    sa, s1 = s.sqrt_alphas_cumprod[t].view(5, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod[t].view(5, 1, 1, 1)
    per = _per64(loss_type, out, dict(eps=noise.double(), x0=x0.double(), v=sa.double() * noise.double() - s1.double() * x0.double())[par])
    assert float(loss) == pytest.approx(float(per.mean()), rel=1e-6)
    # a teacher without the hparam is never called
    d = _diffusion(parameterization=par, loss_type=loss_type).train()
    teacher = _Teacher("cfg", tc, tu)
    d.set_denoise_fn(_Student(out), None)
    d.set_distill_teacher(teacher)
    loss_t, _ = d.p_losses(x0, t, noise, cond_drop_prob=0.5)
    assert torch.equal(loss_t, loss) and not teacher.calls


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_hparams_are_validated_at_construction():
    from sgdm_amd.diffusion import distill_option
    bad = [(dict(distill_guidance=float("nan")), "distill_guidance"), (dict(distill_guidance=float("inf")), "distill_guidance"),
           (dict(distill_guidance="2"), "distill_guidance"), (dict(distill_guidance=True), "distill_guidance"),
           (dict(distill_guidance=2.0, distill_rescale=1.5), "distill_rescale"),
           (dict(distill_guidance=2.0, distill_rescale=-0.1), "distill_rescale"),
           (dict(distill_guidance=2.0, distill_rescale=float("nan")), "distill_rescale"),
           (dict(distill_guidance=2.0, distill_rescale="0.7"), "distill_rescale"),
           (dict(distill_rescale=0.7), "distill_guidance is not")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            _diffusion(**kw)
    assert _diffusion().distill is None and _diffusion(distill_guidance=None).distill is None
    assert _diffusion(distill_guidance=3).distill == (3.0, 0.0)
    assert _diffusion(distill_guidance=-1.5, distill_rescale=0.7).distill == (-1.5, 0.7)
    assert _diffusion(distill_guidance=0.0, distill_rescale=1).distill == (0.0, 1.0)
    assert distill_option(type("H", (), {})()) is None


def test_every_refusal_comes_before_either_model_is_called():
    x0, noise, out, tc, tu, t = _inputs()

    def refused(match, teacher, student=None, hp=None, **ukw):
        d = _diffusion(**dict(dict(distill_guidance=W), **(hp or {}))).train()
        student = _Student(out) if student is None else student
        d.set_denoise_fn(student, None)
        if teacher is not None:
            d.set_distill_teacher(teacher)
        with pytest.raises(ValueError, match=match):
            d.p_losses(x0, t, noise, **ukw)
        assert not student.calls
        for m in (teacher, getattr(teacher, "__self__", None)):
            assert not getattr(m, "calls", None)

    refused("no teacher", None)
    refused("learn_sigma", _Teacher("cfg", tc, tu), student=_Student(torch.cat([out, out], 1), 6),
            hp=dict(learn_sigma=True, out_channels=6, channels=3))
    lv_teacher = _Teacher("cfg", tc, tu)
    lv_teacher.learn_sigma = True
    refused("learn_sigma", lv_teacher)
    refused("output channels", _Teacher("cfg", tc, tu, out_channels=6))
    refused("output channels", _Teacher("cfg", tc, tu).forward_with_cond_scale, student=_Student(out, 4))
    class Both(_Teacher):
        def forward(self, x, tt, *a, **kw):
            self.calls.append(dict(x=x.clone(), kw=kw))
            return out, 0.0, dict()

    both = Both("cfg", tc, tu)
    refused("same object", both, student=both)
    refused("same object", both.forward_with_cond_scale, student=both)
    refused("train mode", _Teacher("cfg", tc, tu).train())
    refused("require grad", _Teacher("cfg", tc, tu).requires_grad_(True))
    refused("require grad", _Teacher("cfg", tc, tu).requires_grad_(True).forward_with_cond_scale)
    refused("cond_drop_mask", _Teacher("cfg", tc, tu), cond_drop_mask=torch.tensor([True, False, False, True, False]))
    # CFG rescale of the target reads both halves of the drop-in teacher's doubled evaluation: the fused path only
    refused("distill_rescale", _Teacher("cfg", tc, tu), hp=dict(distill_rescale=0.7))
    # and a teacher whose output has another shape is refused when it is seen
    d = _diffusion(distill_guidance=W).train()
    d.set_denoise_fn(_Student(out), None)
    d.set_distill_teacher(lambda x, tt, w, **kw: torch.cat([tc, tc], 1))
    with pytest.raises(ValueError, match="teacher's output"):
        d.p_losses(x0, t, noise)


def test_a_plain_callable_teacher_is_called_with_the_weight():
    x0, noise, out, tc, tu, t = _inputs()
    seen = []

    def teacher(x, tt, w, **kw):
        seen.append((w, sorted(kw)))
        return _guided("imagen", tc, tu, w)
    d = _diffusion(distill_guidance=W).train()
    d.set_denoise_fn(_Student(out), None)
    d.set_distill_teacher(teacher)
    loss, _ = d.p_losses(x0, t, noise, layout=torch.zeros(5, 1))
    assert seen == [(W, ["cond", "layout"])]
    per = _per64("l2", out, _guided("imagen", tc.double(), tu.double(), W))
    assert float(loss) == pytest.approx(float(per.mean()), rel=1e-6)
    d.set_distill_teacher(None)
    with pytest.raises(ValueError, match="no teacher"):
        d.p_losses(x0, t, noise)


# --------------------------------------------------------------------------------------------------------------- isolation

def test_the_teacher_reaches_no_parameters_and_no_state_dict():
    x0, noise, out, tc, tu, t = _inputs()
    plain = _diffusion(distill_guidance=W)
    names_p, names_s = [n for n, _ in plain.named_parameters()], sorted(plain.state_dict())
    d = _diffusion(distill_guidance=W)
    teacher = _Teacher("cfg", tc, tu)
    d.set_distill_teacher(teacher)
    assert [n for n, _ in d.named_parameters()] == names_p and sorted(d.state_dict()) == names_s
    mine = {id(v) for v in list(teacher.parameters()) + list(teacher.buffers()) + [tc, tu]}
    assert mine and not mine & {id(v) for v in list(d.parameters()) + list(d.buffers()) + list(d.state_dict().values())}
    assert teacher not in list(d.modules()) and "_distill_teacher" not in d._modules
    # train() / double() of the diffusion object do not reach it
    d.train().double()
    assert not teacher.training and teacher.weight.dtype == torch.float32
    # a bound method is kept as it is
    d.set_distill_teacher(teacher.forward_with_cond_scale)
    assert [n for n, _ in d.named_parameters()] == names_p and sorted(d.state_dict()) == names_s


# ---------------------------------------------------------------------------------------------------------------- sampling

def test_cfg_distilled_is_refused_with_a_guidance_schedule_before_the_library_is_loaded(monkeypatch):
    from sgdm_amd import _lib as L
    from sgdm_amd.diffusion import _StepRunner, cfg_distilled_option, cfg_options

    def no_load():
        raise AssertionError("the library must not be loaded before the arguments are checked")
    monkeypatch.setattr(L, "load", no_load)
    assert cfg_options(dict(cfg_distilled=True)) == (0.0, None)
    assert cfg_options(dict(cfg_distilled=False, cfg_rescale=0.5, cfg_interval=(1, 5))) == (0.5, (1, 5))
    assert cfg_distilled_option(None) is False and cfg_distilled_option({}) is False
    for bad, match in ((dict(cfg_interval=(100, 900)), "cfg_interval"), (dict(cfg_rescale=0.7), "cfg_rescale"),
                       (dict(cfg_interval=(0, 999), cfg_rescale=1.0), "cfg_interval"),
                       (dict(lv_native=True), "learned-variance")):
        with pytest.raises(ValueError, match=match):
            cfg_options(dict(bad, cfg_distilled=True))
        with pytest.raises(ValueError, match=match):
            _StepRunner(lambda x, t, **kw: x, dict(cond_scale=2.0), dict(bad, cfg_distilled=True))
    # a generic denoise_sample_fn guides inside the call: there is no conditional evaluation to take alone
    with pytest.raises(ValueError, match="drop-in UNet"):
        cfg_options(dict(cfg_distilled=True), fused=False)
    with pytest.raises(ValueError, match="drop-in UNet"):
        _StepRunner(lambda x, t, **kw: x, dict(cond_scale=2.0), dict(cfg_distilled=True))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="cfg_distilled"):
            cfg_options(dict(cfg_distilled=bad))


def test_the_hparam_guidance_distilled_sets_the_kwarg(monkeypatch):
    seen = {}

    def sample(shape, sampling_kwargs=None, **kw):
        seen.update(sampling_kwargs)
        z = torch.zeros(shape)
        return z, dict(pred_x0=z)
    for hp, given, want in ((dict(guidance_distilled=True), {}, True), ({}, {}, None), (dict(guidance_distilled=False), {}, None),
                            (dict(guidance_distilled=True), dict(cfg_distilled=False), False), ({}, dict(cfg_distilled=True), True)):
        d = _diffusion(**hp)
        d.set_denoise_fn(None, lambda *a, **k: None)
        monkeypatch.setattr(d.sampler_list["ddim"], "sample", sample)
        seen.clear()
        d.p_sample_loop("ddim", (1, 3, 4, 4), dict(given, num_timesteps=4))
        assert seen.get("cfg_distilled") is want, (hp, given)


# --------------------------------------------------------------------------------------------------------------- loss path

def test_loss_path_of_every_combination():
    """the one decision p_losses_hip takes: a distillation step never runs the weighted kernels (they form the trained
    target, not the teacher's); without a drop-in UNet teacher on the device it is the torch chain on the teacher's tensor"""
    from sgdm_amd.losses import _loss_path
    unet, w = object(), object()
    for lv, distilling, d_unet, weights, on_dev, want in (
            (False, False, None, None, True, "torch"), (False, False, None, None, False, "torch"),
            (False, False, None, w, True, "weighted_fused"), (False, False, None, w, False, "torch"),
            (False, True, unet, None, True, "distill_fused"), (False, True, unet, w, True, "distill_fused"),
            (False, True, None, None, True, "torch"), (False, True, None, w, True, "torch"),
            (False, True, None, None, False, "torch"), (False, True, None, w, False, "torch"),
            (True, False, None, None, True, "lv"), (True, False, None, w, True, "lv"), (True, False, None, w, False, "lv")):
        assert _loss_path(lv, distilling, d_unet, weights, on_dev) == want, (lv, distilling, d_unet, weights, on_dev)


# ----------------------------------------------------------------------------------------------------------------- binding

def test_binding_declares_both_entries_and_the_abi_stays():
    import ctypes as C
    from sgdm_amd import _lib as L
    txt = open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()
    assert int(re.search(r"#define SGD_ABI_VERSION (\d+)", txt).group(1)) == L.ABI_VERSION == 25
    for name, nargs in (("sgd_distill_loss_fwd", 13), ("sgd_distill_loss_bwd", 14)):
        res, args = L.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == nargs and args[2] is C.c_int32 and args[3] is L.dvp
        proto = re.search(r"int %s\(([^;]*)\);" % name, txt).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == nargs
    bwd = L.SIGNATURES["sgd_distill_loss_bwd"][1]
    assert bwd[10] is L.dvp and bwd[11] is C.c_float            # gper from the device, gscale a constant of the caller
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgdm_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "distill.hip" in b._sources() and b.FILE_FLAGS["distill.hip"] == ["-ffp-contract=off"]
