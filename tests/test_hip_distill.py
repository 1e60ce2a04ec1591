"""Guidance distillation on the HIP path (Meng et al. 2023, stage 1): csrc/distill.hip: sgd_distill_loss_fwd / sgd_distill_loss_bwd;
sgdm_amd/train.py: _DistillLossFn, distill_teacher_from, p_losses_hip with the hparam distill_guidance; sgdm_amd/diffusion.py: the
sampling kwarg cfg_distilled (_StepRunner, _GraphedStep).  The reference has no counterpart; the expected values are the formulas
restated here -- the gradient in torch fp32, product by product in the kernel's documented order (bit-exact gate), the loss in
float64 over the same fp32 inputs -- and the project's own paths: the explicit-target step through forward_with_cond_scale and
_MSEFn, and the cond-only evaluations of an empty cfg_interval.  GPU only.

Bounds (those of tests/test_hip_loss_weighting.py for sgd_loss_fwd / sgd_loss_bwd): per-sample loss 1e-6 relative against float64,
gradient bit-equal to torch fp32 and 1e-5 rel-L2 against float64; training step: loss 1e-6 relative, first / last parameter
gradient 1e-4 max-rel against the explicit-target step.  Every test prints the figure it asserts on (run with -s).
Measured on the MI355X: per-sample loss at most 1.4e-7 from float64, gradient bit-equal to torch fp32 and at most 5.0e-7 rel-L2
from float64; training step loss 9.9e-8 (1.4e-7 with distill_rescale), parameter gradients bit-equal (at most 2.1e-6 with
distill_rescale) to the explicit-target step; fixed point at most 1.2e-12 x mean(target^2), 0.08 .. 1.2 x at w = 2; fixed batch,
8 steps: last / first loss 0.133."""
import pytest
import torch

from conftest import max_rel, rel_l2
from test_hip_unet import build_model
from test_hip_vpred import _guided32, _sk, _st

pytestmark = pytest.mark.gpu

T, S, N, W, PHI = 1000, 16, 4, 2.0, 0.7
KINDS = ("l2", "l1", "huber")


def _diffusion(**kw):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, **kw))


# ---------------------------------------------------------------------------------------------------------------- kernels

def _dev(x, offset):
    """`x` on the device, `offset` floats past a 16-byte boundary"""
    buf = torch.empty(x.numel() + 4, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + x.numel()].view(x.shape)
    v.copy_(x)
    return v


def _case(b, c, hw, mode, w, seed, offset):
    """student output NCHW [b, c, hw] and teacher output NHWC [2b | b, hw, c]; `out` drawn so that |d| lies on both sides of 1
    and a few elements have d == 0 exactly (there both teacher halves are 0: a target that is exact in fp32 AND in float64)"""
    g = torch.Generator().manual_seed(seed)
    teach = torch.randn(2 * b if mode else b, hw, c, generator=g)
    zero = torch.zeros(b, c, hw, dtype=torch.bool)
    zero.view(-1)[::7] = True
    z = zero.permute(0, 2, 1)
    teach[:b][z] = 0.0
    if mode:
        teach[b:][z] = 0.0
    target = _guided32(teach, mode, w, b).permute(0, 2, 1).contiguous()
    out = target + 1.2 * torch.randn(b, c, hw, generator=g)
    out[zero] = target[zero]
    d = out - target
    assert bool((d == 0).any()) and not target[zero].any()
    if c * hw >= 64:
        assert bool((d.abs() > 1).any()) and bool(((d.abs() < 1) & (d != 0)).any())
    t = torch.randint(0, T, (b,), generator=g)
    return dict(out=_dev(out, offset), teach=_dev(teach, offset), t=t.cuda(), host=(out, teach, t))


def _fwd(lib, cs, mode, w_dev, wt, kind, b, c, hw):
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    bufs = [torch.full((b + 2,), float("nan"), device="cuda") for _ in range(2)]
    raw, pw = (v[1:1 + b] for v in bufs)
    L.check(lib.sgd_distill_loss_fwd(_ptr(cs["out"]), _ptr(cs["teach"]), mode, _ptr(w_dev), _ptr(cs["t"]), _ptr(wt), kind, b, c, hw,
                                     _ptr(raw), _ptr(pw), _st()), "sgd_distill_loss_fwd")
    torch.cuda.synchronize()
    for v in bufs:                                                  # nothing written outside [b]
        assert bool(torch.isnan(v[0])) and bool(torch.isnan(v[-1]))
    return raw.clone(), pw.clone()


def _bwd(lib, cs, mode, w_dev, wt, kind, b, c, hw, gper, gscale, offset):
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    n = b * c * hw
    buf = torch.full((n + 4,), float("nan"), device="cuda")
    gout = buf[offset:offset + n].view(b, c, hw)
    L.check(lib.sgd_distill_loss_bwd(_ptr(cs["out"]), _ptr(cs["teach"]), mode, _ptr(w_dev), _ptr(cs["t"]), _ptr(wt), kind, b, c, hw,
                                     gper.data_ptr(), gscale, _ptr(gout), _st()), "sgd_distill_loss_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(torch.cat([buf[:offset], buf[offset + n:]])).all())     # nothing written outside [b, c, hw]
    return gout


def _restate(host, mode, w, wt, kind, gper, gscale, dtype):
    """(per_raw, per_w, gout) in `dtype` from the fp32 inputs; in fp32 every product is rounded before it is added (1 - w and
    1 + w formed in fp32) and the gradient follows the kernel's order: k = (gper * wt[t]) / chw, k = k * gscale,
    g = (2 k) d | k sign(d) | k clamp(d, -1, 1)"""
    out, teach, t = host
    b, c, hw = out.shape
    o, tc = out.to(dtype), teach.to(dtype)
    if dtype == torch.float32:
        target = _guided32(tc, mode, w, b)
    else:
        target = tc if mode == 0 else (1.0 - w) * tc[b:] + w * tc[:b] if mode == 1 else (1.0 + w) * tc[:b] - w * tc[b:]
    d = o - target.permute(0, 2, 1)
    el = d * d if kind == 0 else d.abs() if kind == 1 else torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    wts = wt.cpu().to(dtype)[t] if wt is not None else torch.ones(b, dtype=dtype)
    raw = el.reshape(b, -1).mean(1)
    k = (gper.to(dtype) * wts) / torch.tensor(float(c * hw), dtype=dtype)
    k = (k * torch.tensor(gscale, dtype=dtype)).view(b, 1, 1)
    g = (2 * k) * d if kind == 0 else k * torch.sign(d) if kind == 1 else k * d.clamp(-1, 1)
    return raw, wts * raw, g


def _rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float(((got - want).abs() / want.abs()).max())


# (b, c, hw, offset in floats): the 16-byte path on several waves; an odd chw on the scalar path from buffers 4 bytes past a
# 16-byte boundary; one sample of one wave; 1026 quads per plane: the forward workgroup (1024 threads) strides its loop a second
# time, the backward takes 5 blocks per sample, the last with 2 live threads; the same past 1024 threads on the scalar path with
# an odd hw; hw % 4 == 0 but 4 bytes off a 16-byte boundary, which must take the scalar path
SHAPES = [(3, 3, 256, 0), (2, 3, 25, 1), (1, 4, 64, 0), (2, 3, 4104, 0), (2, 3, 1029, 1), (1, 4, 64, 1)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("b,c,hw,offset", SHAPES)
def test_kernels_every_guided_form_and_loss(b, c, hw, offset, mode):
    from sgdm_amd import _lib as L
    lib = L.load()
    table = torch.rand(T, generator=torch.Generator().manual_seed(5)).cuda() + 0.25
    worst_f, worst_g = 0.0, 0.0
    for kind in range(3):
        w = (W, -0.3, 7.5)[kind]
        w_dev = torch.tensor([w], dtype=torch.float32, device="cuda")
        cs = _case(b, c, hw, mode, w, seed=31 * mode + 7 * kind + hw % 5, offset=offset)
        gper = torch.rand(b, generator=torch.Generator().manual_seed(hw + mode)) + 0.5
        for wt, gscale in ((table, 1.0), (None, 3.0)):
            raw, pw = _fwd(lib, cs, mode, w_dev, wt, kind, b, c, hw)
            raw2, pw2 = _fwd(lib, cs, mode, w_dev, wt, kind, b, c, hw)
            gout = _bwd(lib, cs, mode, w_dev, wt, kind, b, c, hw, gper.cuda(), gscale, offset)
            assert torch.equal(raw, raw2) and torch.equal(pw, pw2)                  # fixed fold order: run-to-run identical
            assert torch.equal(gout, _bwd(lib, cs, mode, w_dev, wt, kind, b, c, hw, gper.cuda(), gscale, offset))
            _, _, g32 = _restate(cs["host"], mode, w, wt, kind, gper, gscale, torch.float32)
            raw64, pw64, g64 = _restate(cs["host"], mode, w, wt, kind, gper, gscale, torch.float64)
            assert torch.equal(gout.cpu(), g32), (mode, kind, wt is not None, float((gout.cpu() - g32).abs().max()))
            worst_f = max(worst_f, _rel(raw, raw64), _rel(pw, pw64))
            worst_g = max(worst_g, rel_l2(gout.cpu(), g64))
            if wt is None:
                assert torch.equal(raw, pw)
    print(f"distill kernels (b, c, hw) = {(b, c, hw)} offset {offset} mode {mode}: per-sample loss max rel {worst_f:.2e}; gradient "
          f"bit-equal to torch fp32, max rel-L2 vs float64 {worst_g:.2e}")
    assert worst_f <= 1e-6
    assert worst_g <= 1e-5


@pytest.mark.parametrize("mode,w", [(1, 1.0), (2, 0.0)])
@pytest.mark.parametrize("b,c,hw,offset", SHAPES)
def test_identity_weight_is_the_conditional_half(b, c, hw, offset, mode, w):
    """the target is the conditional half bit for bit: sgd_loss_fwd / sgd_loss_bwd with par = 1 fed that half as x0 agree"""
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    w_dev = torch.tensor([w], dtype=torch.float32, device="cuda")
    cs = _case(b, c, hw, mode, w, seed=hw + mode, offset=offset)
    out, teach, t = cs["host"]
    x0 = _dev(teach[:b].permute(0, 2, 1).contiguous(), offset)
    gper = (torch.rand(b, generator=torch.Generator().manual_seed(3)) + 0.5).cuda()
    for kind in range(3):
        raw, pw = _fwd(lib, cs, mode, w_dev, None, kind, b, c, hw)
        gout = _bwd(lib, cs, mode, w_dev, None, kind, b, c, hw, gper, 1.0, offset)
        raw_l, pw_l, g_l = torch.empty(b, device="cuda"), torch.empty(b, device="cuda"), torch.empty(b, c, hw, device="cuda")
        L.check(lib.sgd_loss_fwd(_ptr(cs["out"]), _ptr(x0), None, _ptr(cs["t"]), None, None, None, 1, kind, b, c * hw, _ptr(raw_l),
                                 _ptr(pw_l), _st()), "sgd_loss_fwd")
        L.check(lib.sgd_loss_bwd(_ptr(cs["out"]), _ptr(x0), None, _ptr(cs["t"]), None, None, None, gper.data_ptr(), 1.0, 1, kind, b,
                                 c * hw, _ptr(g_l), _st()), "sgd_loss_bwd")
        torch.cuda.synchronize()
        assert torch.equal(raw, raw_l) and torch.equal(pw, pw_l), (kind, raw.tolist(), raw_l.tolist())
        assert torch.equal(gout, g_l)
        # and mode 0 on the conditional half alone
        c0 = dict(cs, teach=_dev(teach[:b].contiguous(), offset))
        assert torch.equal(_fwd(lib, c0, 0, None, None, kind, b, c, hw)[0], raw)


def test_entry_points_refuse_bad_arguments():
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    f, t = torch.zeros(128, device="cuda"), torch.zeros(2, dtype=torch.long, device="cuda")
    o1, o2 = torch.full((64,), -7.0, device="cuda"), torch.full((64,), -7.0, device="cuda")
    fwd = dict(out=_ptr(f), teach=_ptr(f), mode=2, w=_ptr(f), t=_ptr(t), wt=_ptr(f), kind=0, b=1, c=4, hw=8, raw=_ptr(o1), pw=_ptr(o2),
               st=_st())
    bwd = dict(out=_ptr(f), teach=_ptr(f), mode=2, w=_ptr(f), t=_ptr(t), wt=_ptr(f), kind=0, b=1, c=4, hw=8, gper=f.data_ptr(),
               gscale=1.0, gout=_ptr(o1), st=_st())
    common = (dict(out=None), dict(teach=None), dict(t=None), dict(b=0), dict(b=-1), dict(c=0), dict(c=-3), dict(hw=0), dict(hw=-4),
              dict(mode=3), dict(mode=-1), dict(kind=3), dict(kind=-1), dict(w=None), dict(mode=1, w=None),
              dict(c=2 ** 20, hw=2 ** 20), dict(b=2 ** 30))
    for args, fn, own in ((fwd, lib.sgd_distill_loss_fwd, (dict(raw=None), dict(pw=None))),
                          (bwd, lib.sgd_distill_loss_bwd, (dict(gper=None), dict(gout=None)))):
        for bad in common + own:                                    # (keyword order is the C argument order)
            assert fn(*dict(args, **bad).values()) == 1, (fn.__name__, bad)     # SGD_ERR_ARG: refused before any launch
    torch.cuda.synchronize()
    assert bool((o1 == -7.0).all()) and bool((o2 == -7.0).all())               # nothing written
    for args, fn in ((fwd, lib.sgd_distill_loss_fwd), (bwd, lib.sgd_distill_loss_bwd)):
        for ok in (dict(mode=0, w=None), dict(wt=None), {}):                    # what a call does not read may be missing
            assert fn(*dict(args, **ok).values()) == 0, (fn.__name__, ok)
    torch.cuda.synchronize()
    assert not bool((o1 == -7.0).all())


# --------------------------------------------------------------------------------------------------------------- training

def _batch(entry, seed=26):
    from sgdm_amd.synth import synth_batch
    kw = entry["ctor"]
    batch = synth_batch(kw["condition_method"], N, S, kw["cond_dim"], entry["layout_dim"], seed=seed)
    g = torch.Generator().manual_seed(3)
    x0, noise = batch["image"].cuda(), torch.randn(N, 3, S, S, generator=g).cuda()
    ukw = dict(cond=batch["cond"].float().cuda())
    if "layout" in batch:
        ukw["layout"] = batch["layout"].cuda()
    return x0, noise, ukw


def _student(name, prec, scale_type="imagen"):
    m, entry = build_model(name, prec, scale_type)
    m.dropout = 0.0
    return m.train(), entry


def _other_teacher(m, **kw):
    """a teacher whose output is not the student's: the copy with its head conv scaled by 1.5"""
    from sgdm_amd.train import distill_teacher_from
    teacher = distill_teacher_from(m, **kw)
    with torch.no_grad():
        teacher.P("out.2.weight").mul_(1.5)
        teacher.P("out.2.bias").mul_(1.5)
    return teacher


@pytest.fixture(scope="module")
def pairs():
    """per precision: the c32 student in training mode, a frozen teacher that differs from it, one fixed batch"""
    cache = {}

    def get(prec):
        if prec not in cache:
            m, entry = _student("uf_clusterlayout_c32_s16", prec)
            cache[prec] = (m, _other_teacher(m)) + _batch(entry)
        return cache[prec]
    return get


def _attach(d, m):
    seen = {}

    def denoise_fn(x, t, **kw):
        out = m.forward(x, t, **kw)
        seen["x_noisy"], seen["kw"] = x.detach().clone(), kw
        seen["out"] = out[0].detach().clone()
        return out
    d.set_denoise_fn(denoise_fn, m.forward_with_cond_scale)
    return seen


def _step(d, m, x0, t, noise, ukw):
    """p_losses + backward: (loss, loss_dict, first gradient, last gradient), gradients cloned"""
    m.zero_grad(set_to_none=True)
    loss, ld = d.p_losses(x0, t, noise, **ukw)
    loss.backward()
    params = [p for p in m.parameters() if p.requires_grad]
    return loss.detach().clone(), ld, params[0].grad.clone(), params[-1].grad.clone()


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


ENTRIES = ("sgd_distill_loss_fwd", "sgd_distill_loss_bwd", "sgd_cfg_combine", "sgd_cfg_guide", "sgd_nhwc_to_nchw", "sgd_q_sample",
           "sgd_q_sample_v", "sgd_loss_fwd", "sgd_loss_bwd")


def _explicit_target(teacher, x, t, ukw, phi):
    """what a user would write today: forward_with_cond_scale (and, for the rescale, the conditional evaluation: Lin et al.
    2023, eq. 15-16 in float64 from the two fp32 outputs)"""
    with torch.no_grad():
        g = teacher.forward_with_cond_scale(x, t, W, **ukw)
        if phi == 0:
            return g
        pos = teacher.forward(x, t, cond_drop_prob=0.0, **ukw)[0].double()
        g = g.double()
        f = pos.reshape(N, -1).std(1) / g.reshape(N, -1).std(1)
        return ((phi * f + (1.0 - phi)).view(N, 1, 1, 1) * g).float()


@pytest.mark.parametrize("phi", [0.0, PHI])
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("par", ["eps", "v"])
def test_training_step_against_the_explicit_target(par, prec, phi, pairs, monkeypatch):
    """one distillation p_losses + backward on the c32 model against the same student step with the explicit target fed to
    _MSEFn; the launches counted: one loss kernel each way, no combine, no re-layout of the teacher's output"""
    from sgdm_amd.losses import _MSEFn
    m, teacher, x0, noise, ukw = pairs(prec)
    hp = dict(distill_rescale=phi) if phi else {}
    d = _diffusion(parameterization=par, distill_guidance=W, **hp).train()
    seen = _attach(d, m)
    d.set_distill_teacher(teacher)
    t = torch.tensor([0, 999, 250, 731]).cuda()
    calls = _count(monkeypatch, *ENTRIES)
    loss, ld, first, last = _step(d, m, x0, t, noise, dict(ukw, cond_drop_prob=0.5))
    # (the one sgd_nhwc_to_nchw is the student's own output)
    assert calls == dict(sgd_distill_loss_fwd=1, sgd_distill_loss_bwd=1, sgd_cfg_combine=0, sgd_cfg_guide=int(phi > 0),
                         sgd_nhwc_to_nchw=1, sgd_q_sample=1, sgd_q_sample_v=0, sgd_loss_fwd=0, sgd_loss_bwd=0)
    assert seen["kw"]["cond_drop_prob"] == 0.0
    assert sorted(ld) == ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    s = d.sampler
    sa, s1 = s.sqrt_alphas_cumprod[t].view(N, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod[t].view(N, 1, 1, 1)
    assert torch.equal(seen["x_noisy"], sa * x0 + s1 * noise)       # the bits of the plain path's x_noisy
    # the same student step with an explicit target
    m.zero_grad(set_to_none=True)
    target = _explicit_target(teacher, seen["x_noisy"], t, ukw, phi)
    out = m.forward(seen["x_noisy"], t, cond_drop_prob=0.0, **ukw)[0]
    assert torch.equal(out.detach(), seen["out"])
    per = _MSEFn.apply(out, target)
    want = per.mean()
    want.backward()
    params = [p for p in m.parameters() if p.requires_grad]
    want = float(want.detach())
    err_l = abs(float(loss) - want) / want
    err_y = max_rel(ld["train/epoch_stats_y"].cpu(), per.detach().cpu())
    err_f, err_b = max_rel(first, params[0].grad), max_rel(last, params[-1].grad)
    print(f"distillation step {par} {prec} rescale {phi}: loss {float(loss):.4e}, rel err {err_l:.2e}, per-sample {err_y:.2e}; grad "
          f"first / last parameter vs explicit target {err_f:.2e} / {err_b:.2e}")
    assert float(first.abs().max()) > 0 and float(last.abs().max()) > 0
    assert all(p.grad is None for p in teacher.parameters())
    assert err_l <= 1e-6
    assert err_f < 1e-4 and err_b < 1e-4


def test_loss_weighting_applies_and_validation_launches_the_forward_kernel_only(pairs, monkeypatch):
    m, teacher, x0, noise, ukw = pairs("f32")
    d = _diffusion(parameterization="v", loss_type="huber", loss_weighting="min_snr", distill_guidance=W).train()
    seen = _attach(d, m)
    d.set_distill_teacher(teacher)
    t = torch.tensor([3, 999, 250, 731]).cuda()
    loss, ld, first, _ = _step(d, m, x0, t, noise, ukw)
    target = _explicit_target(teacher, seen["x_noisy"], t, ukw, 0.0).double()
    diff = seen["out"].double() - target
    per = torch.where(diff.abs() < 1, 0.5 * diff ** 2, diff.abs() - 0.5).reshape(N, -1).mean(1)
    w = s_w = d.sampler.loss_weights[t].double()
    assert len(set(s_w.tolist())) == N
    want = (w * per).mean()
    err = abs(float(loss) - float(want)) / float(want)
    assert sorted(ld) == ["train/ddpm_loss", "train/ddpm_loss_raw", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    err_y = max_rel(ld["train/epoch_stats_y"].cpu(), per.cpu())
    print(f"weighted huber distillation step: loss rel err {err:.2e}, unweighted per-sample {err_y:.2e}")
    assert err <= 1e-6 and err_y <= 1e-6 and float(first.abs().max()) > 0
    # validation
    d.eval()
    calls = _count(monkeypatch, *ENTRIES)
    with torch.no_grad():
        vloss, vd = d.p_losses(x0, t, noise, **ukw)
    assert calls["sgd_distill_loss_fwd"] == 1 and calls["sgd_distill_loss_bwd"] == 0 and calls["sgd_loss_fwd"] == 0
    assert sorted(vd) == ["val/ddpm_loss", "val/ddpm_loss_raw", "val/loss"] and not vloss.requires_grad
    # (the student's inference forward is not its training forward bit for bit: the 1e-4 parity contract)
    assert float(vloss) == pytest.approx(float(loss), rel=1e-3)


@pytest.mark.parametrize("loss_type", ["l2", "huber"])
def test_callable_teacher_with_loss_weighting_trains_against_the_teacher(loss_type, pairs, monkeypatch):
    """a teacher that is not a drop-in UNet (a plain callable) on the device, loss_weighting on: the torch chain on the teacher's
    guided output times the weights -- NOT the weighted kernels, which form the trained target (here v) themselves.  Bound: the
    1e-6 relative of the weighted step above (an fp32 mean of 768 terms against float64)."""
    m, teacher, x0, noise, ukw = pairs("f32")
    d = _diffusion(parameterization="v", loss_type=loss_type, loss_weighting="min_snr", distill_guidance=W).train()
    seen = _attach(d, m)
    asked = []

    def teach(x, t, w, cond=None, **kw):
        asked.append(w)
        return teacher.forward_with_cond_scale(x, t, w, cond=cond, **kw)
    d.set_distill_teacher(teach)
    t = torch.tensor([3, 999, 250, 731]).cuda()
    calls = _count(monkeypatch, *ENTRIES)
    loss, ld, first, _ = _step(d, m, x0, t, noise, ukw)
    assert asked == [W]
    assert calls["sgd_loss_fwd"] == 0 and calls["sgd_loss_bwd"] == 0
    assert calls["sgd_distill_loss_fwd"] == 0 and calls["sgd_distill_loss_bwd"] == 0
    assert calls["sgd_q_sample"] == 1 and calls["sgd_q_sample_v"] == 0
    diff = seen["out"].double() - _explicit_target(teacher, seen["x_noisy"], t, ukw, 0.0).double()
    el = diff ** 2 if loss_type == "l2" else torch.where(diff.abs() < 1, 0.5 * diff ** 2, diff.abs() - 0.5)
    per = el.reshape(N, -1).mean(1)
    want = (d.sampler.loss_weights[t].double() * per).mean()
    err = abs(float(loss) - float(want)) / float(want)
    err_y = max_rel(ld["train/epoch_stats_y"].cpu(), per.cpu())
    # the trained target would give another loss altogether
    sa, s1 = (v[t].view(N, 1, 1, 1).double() for v in (d.sampler.sqrt_alphas_cumprod, d.sampler.sqrt_one_minus_alphas_cumprod))
    dv = seen["out"].double() - (sa * noise.double() - s1 * x0.double())
    elv = dv ** 2 if loss_type == "l2" else torch.where(dv.abs() < 1, 0.5 * dv ** 2, dv.abs() - 0.5)
    other = (d.sampler.loss_weights[t].double() * elv.reshape(N, -1).mean(1)).mean()
    print(f"weighted {loss_type} distillation step, callable teacher: loss rel err {err:.2e}, unweighted per-sample {err_y:.2e}; "
          f"against the v target it would be {float(other):.4e}, not {float(want):.4e}")
    assert sorted(ld) == ["train/ddpm_loss", "train/ddpm_loss_raw", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    assert err <= 1e-6 and err_y <= 1e-6 and float(first.abs().max()) > 0
    assert abs(float(other) - float(want)) > 1e-3 * float(want)


def test_refusals_come_before_any_launch(pairs, monkeypatch):
    from sgdm_amd.train import distill_teacher_from
    m, teacher, x0, noise, ukw = pairs("f32")
    t = torch.tensor([0, 999, 250, 731]).cuda()
    calls = _count(monkeypatch, "sgd_q_sample", "sgd_q_sample_v", "sgd_distill_loss_fwd")

    def refused(match, teach, hp=None, **extra):
        d = _diffusion(**dict(dict(distill_guidance=W), **(hp or {}))).train()
        if hp:                                                      # (set_denoise_fn itself refuses a C-wide UNet for learn_sigma)
            d.set_denoise_fn(lambda *a, **k: m.forward(*a, **k), None)
        else:
            d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
        if teach is not None:
            d.set_distill_teacher(teach)
        with pytest.raises(ValueError, match=match):
            d.p_losses(x0, t, noise, **dict(ukw, **extra))

    refused("no teacher", None)
    refused("same object", m)
    refused("same object", m.forward_with_cond_scale)
    refused("train mode", distill_teacher_from(m).train())
    refused("require grad", distill_teacher_from(m).requires_grad_(True))
    refused("cond_drop_mask", teacher, cond_drop_mask=torch.tensor([True, False, False, True]).cuda())
    refused("learn_sigma", teacher, hp=dict(learn_sigma=True))
    wide, _ = build_model("uf_clusterlayout_c32_s16", "f32")
    wide.out_channels = 6                                           # (only looked at: refused before anything is built)
    refused("output channels", wide)
    assert calls == dict(sgd_q_sample=0, sgd_q_sample_v=0, sgd_distill_loss_fwd=0)
    with pytest.raises(TypeError):
        distill_teacher_from(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="hip_precision"):
        distill_teacher_from(m, hip_precision="fp8")


def test_teacher_isolation_over_optimizer_steps():
    """two FusedAdamWEma steps: every teacher tensor keeps its bits, the teacher has no .grad, it reaches neither the
    student's parameters nor the EMA, and an 'f16' teacher runs while the student trains in f16x3"""
    from sgdm_amd.ema import LitEma
    from sgdm_amd.optim import FusedAdamWEma
    from sgdm_amd.train import distill_teacher_from
    m, entry = _student("uf_clusterlayout_c32_s16", "f16x3")
    x0, noise, ukw = _batch(entry)
    ema = LitEma(m)
    with torch.no_grad():                                           # shadows that are not the parameters
        for b in ema.buffers():
            if b.dtype == torch.float32 and b.dim() > 0:
                b.mul_(0.5)
    teacher = distill_teacher_from(m, ema=ema, hip_precision="f16")
    assert teacher.hip_precision == "f16" and m.hip_precision == "f16x3" and not teacher.training
    assert not teacher._engines and "_hip_graph_steps" not in teacher.__dict__
    shadow = dict(ema.named_buffers())
    for name, p in teacher.named_parameters():
        assert not p.requires_grad
        if name in ema.m_name2s_name:
            assert torch.equal(p, shadow[ema.m_name2s_name[name]]) and p.data_ptr() != shadow[ema.m_name2s_name[name]].data_ptr()
    mine = {p.data_ptr() for p in m.parameters()}
    assert not mine & {p.data_ptr() for p in teacher.parameters()}
    start = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    d = _diffusion(distill_guidance=W).train()
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    d.set_distill_teacher(teacher)
    assert not {id(p) for p in teacher.parameters()} & {id(p) for p in d.parameters()}
    opt = FusedAdamWEma([p for p in m.parameters() if p.requires_grad], lr=1e-3, ema=ema, ema_model=m)
    t = torch.tensor([10, 999, 250, 731]).cuda()
    before = [p.detach().clone() for p in m.parameters()]
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss, _ = d.p_losses(x0, t, noise, **ukw)
        loss.backward()                                             # (the teacher's forward ran after nothing of the student's:
        opt.step()                                                  #  no stale-forward error)
        losses.append(float(loss))
    torch.cuda.synchronize()
    assert all(torch.isfinite(torch.tensor(losses))) and losses[0] > 0
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
    end = teacher.state_dict()
    assert sorted(end) == sorted(start) and all(torch.equal(end[k], start[k]) for k in start)
    assert all(p.grad is None for p in teacher.parameters())
    print(f"f16 teacher, f16x3 student, two optimizer steps: losses {losses}")


@pytest.mark.parametrize("scale_type,prec,w_id", [("imagen", "f32", 1.0), ("cfg", "f16x3", 0.0)])
def test_fixed_point_at_the_identity_weight(scale_type, prec, w_id):
    """student == teacher and w the identity weight of the scale type: the loss is the squared parity error of the training
    and the inference forward, at most (1e-4)^2 of the target's mean square; w = 2 on the same pair is far above it"""
    from sgdm_amd.train import distill_teacher_from
    m, entry = _student("uf_clusterlayout_c32_s16", prec, scale_type)
    x0, noise, ukw = _batch(entry)
    teacher = distill_teacher_from(m)
    t = torch.tensor([0, 999, 250, 731]).cuda()
    per = {}
    for w in (w_id, 2.0):
        d = _diffusion(distill_guidance=w).train()
        seen = _attach(d, m)
        d.set_distill_teacher(teacher)
        loss, ld = d.p_losses(x0, t, noise, **ukw)
        loss.backward()
        per[w] = ld["train/epoch_stats_y"].double().cpu()
    with torch.no_grad():
        target = teacher.forward(seen["x_noisy"], t, cond_drop_prob=0.0, **ukw)[0].double()
    ms = (target ** 2).reshape(N, -1).mean(1).cpu()
    print(f"fixed point {scale_type} {prec}: per-sample loss / mean(target^2) at w = {w_id}: {(per[w_id] / ms).tolist()}; at w = 2: "
          f"{(per[2.0] / ms).tolist()}")
    assert bool((per[w_id] <= 1e-8 * ms).all())
    assert bool((per[2.0] > 1e-4 * ms).all())


def test_a_fixed_batch_is_learned():
    """8 steps on one batch, lr 1e-3, w = 2, the student initialised from the teacher: the loss goes down"""
    from sgdm_amd.optim import FusedAdamWEma
    from sgdm_amd.train import distill_teacher_from
    m, entry = _student("ca_stego_c32_s16", "f16x3")
    x0, noise, ukw = _batch(entry)
    teacher = distill_teacher_from(m)
    d = _diffusion(distill_guidance=W).train()
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    d.set_distill_teacher(teacher)
    opt = FusedAdamWEma([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    t = torch.tensor([40, 900, 250, 731]).cuda()
    losses = []
    for _ in range(8):
        opt.zero_grad(set_to_none=True)
        loss, _ = d.p_losses(x0, t, noise, **ukw)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(f"fixed batch, 8 steps: losses {[f'{v:.4e}' for v in losses]}, last / first {losses[-1] / losses[0]:.3f}")
    assert all(v == v for v in losses) and losses[-1] < losses[0]


# --------------------------------------------------------------------------------------------------------------- sampling

B = 2
SHAPE = (B, 3, S, S)
METHODS = (("ddim", 6), ("dpmsolver", 6), ("pndm", 4), ("native", 1000))
NATIVE_ROWS = list(range(9, -1, -1))


def _sampling_diffusion(par, m):
    d = _diffusion(parameterization=par)
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    return d


def _times(d, method, steps):
    """the UNet time of every evaluation of the trajectory"""
    s = d.sampler_list[method]
    if method == "native":
        return list(NATIVE_ROWS)
    if method == "ddim":
        s.make_schedule(_sk(d, method, steps))
        return [int(v) for v in s.ddim_timesteps]
    if method == "pndm":
        return [int(v) for v in s.plan(steps)[0]]
    return [int(v) for v in s.plan(_sk(d, method, steps))[0]]


def _run(d, method, steps, dkw, x_T, seed, **skx):
    kw = dict(denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs=dict(dkw), x_T=x_T.clone())
    torch.manual_seed(seed)
    if method == "native":
        return d.sampler.sample(SHAPE, sampling_kwargs=_sk(d, method, steps, **skx), step_indices=list(NATIVE_ROWS), **kw)[0].cpu()
    return d.sampler_list[method].sample(shape=SHAPE, sampling_kwargs=_sk(d, method, steps, **skx), **kw)[0].cpu()


def _sampling_inputs(entry):
    from sgdm_amd.synth import synth_batch
    kw = entry["ctor"]
    batch = synth_batch(kw["condition_method"], B, S, kw["cond_dim"], entry["layout_dim"], seed=23)
    cond = batch["cond"].cuda() if entry["kind"] == "unet_fast" else batch["cond"].float().cuda()
    x_T = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(61)).cuda()
    return dict(cond=cond, layout=batch["layout"].cuda() if "layout" in batch else None), x_T


@pytest.mark.parametrize("name,par,form", [("uf_clusterlayout_c32_s16", "eps", None), ("ca_stego_c32_s16", "v", None),
                                           ("uf_clusterlayout_c32_s16", "v", "data")])
def test_distilled_sampling_is_the_conditional_evaluation_alone(name, par, form):
    """cfg_distilled on the captured and on the eager step, against the mechanism it reuses -- a cfg_interval that contains none
    of the trajectory's times; on a fresh model no 2B engine is ever built; ordinary guided sampling is untouched"""
    from sgdm_amd import _lib as L
    from sgdm_amd.diffusion import V_FORM_SAMPLERS
    m, entry = build_model(name, "f16x3")
    d = _sampling_diffusion(par, m)
    dkw, x_T = _sampling_inputs(entry)
    prec = L.PREC_BY_NAME[m.hip_precision]
    # 1. a fresh model: the distilled trajectories alone, captured; cond_scale is not read (absent here)
    captured = {}
    for method, steps in METHODS:
        skx = dict(v_form="data") if form == "data" and method in V_FORM_SAMPLERS else {}
        captured[method] = _run(d, method, steps, dkw, x_T, 5, cfg_distilled=True, **skx)
        assert torch.isfinite(captured[method]).all()
    assert sorted(m._engines) == [(B, S, S, prec)], sorted(m._engines)          # no batch-2B key
    steps_ = list(m.__dict__["_hip_graph_steps"].values())
    assert len(steps_) == len(METHODS)
    for (method, steps), g in zip(METHODS, steps_):
        n = len(_times(d, method, steps))
        assert g.replays == dict(guided=0, cond=n), (method, g.replays)
        assert g.graph is None and g.graph1 is not None and g.eng is g.eng1 and g.eng.n == B
    # 2. an ordinary guided trajectory before and after: bit-equal, and it is another trajectory
    guided = _run(d, "ddim", 6, dict(dkw, cond_scale=W), x_T, 5)
    assert (2 * B, S, S, prec) in m._engines and not torch.equal(guided, captured["ddim"])
    for method, steps in METHODS:
        skx = dict(v_form="data") if form == "data" and method in V_FORM_SAMPLERS else {}
        times = _times(d, method, steps)
        a = next(v for v in range(T) if v not in times)
        # 3. eager == captured (now on the cached step), whatever cond_scale says
        eager = _run(d, method, steps, dict(dkw, cond_scale=7.5), x_T, 5, cfg_distilled=True, hip_graph=False, **skx)
        again = _run(d, method, steps, dict(dkw, cond_scale=W), x_T, 5, cfg_distilled=True, **skx)
        # 4. both == the empty interval, eager and (one capture of a graph pair is enough: ddim) captured
        iv_e = _run(d, method, steps, dict(dkw, cond_scale=W), x_T, 5, cfg_interval=(a, a), hip_graph=False, **skx)
        iv_c = _run(d, method, steps, dict(dkw, cond_scale=W), x_T, 5, cfg_interval=(a, a), **skx) if method == "ddim" else iv_e
        diffs = [float((v - captured[method]).abs().max()) for v in (eager, again, iv_c, iv_e)]
        print(f"cfg_distilled {name} {par}{'/data' if skx else ''} {method}: max abs diff to the first captured run -- eager, "
              f"captured again, empty interval captured / eager: {diffs}")
        for v in (eager, again, iv_c, iv_e):
            assert torch.equal(v, captured[method])
    assert torch.equal(_run(d, "ddim", 6, dict(dkw, cond_scale=W), x_T, 5), guided)
    # 5. plms (no captured step) runs too, as its empty-interval trajectory
    times = _times(d, "ddim", 6)
    a = next(v for v in range(T) if v not in times)
    p1 = _run(d, "plms", 6, dkw, x_T, 5, cfg_distilled=True)
    p2 = _run(d, "plms", 6, dict(dkw, cond_scale=W), x_T, 5, cfg_interval=(a, a))
    assert torch.isfinite(p1).all() and torch.equal(p1, p2)
    assert not torch.equal(p1, _run(d, "plms", 6, dict(dkw, cond_scale=W), x_T, 5))


def test_distilled_sampling_refusals_and_the_hparam():
    from sgdm_amd import diffusion as Dm
    m, entry = build_model("uf_clusterlayout_c32_s16", "f16x3")
    d = _sampling_diffusion("eps", m)
    dkw, x_T = _sampling_inputs(entry)
    for bad in (dict(cfg_interval=(100, 900)), dict(cfg_rescale=PHI)):
        with pytest.raises(ValueError, match="cfg_distilled"):
            _run(d, "ddim", 6, dict(dkw, cond_scale=W), x_T, 5, cfg_distilled=True, **bad)
    generic = _diffusion()
    generic.set_denoise_fn(m.forward, lambda x, t, **kw: m.forward_with_cond_scale(x, t, **kw))
    with pytest.raises(ValueError, match="drop-in UNet"):
        _run(generic, "ddim", 6, dict(dkw, cond_scale=W), x_T, 5, cfg_distilled=True)
    assert not m._engines                                           # refused before anything was built or launched
    # the hparam guidance_distilled makes p_sample_loop set the kwarg: the same images as the kwarg itself
    sk = dict(sampling_method="ddim", vis=None, num_timesteps=6, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True, dtp=1,
              temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True, disable_tqdm=True)
    hd = _diffusion(guidance_distilled=True)
    hd.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    torch.manual_seed(5)
    by_hparam, _ = hd.p_sample_loop("ddim", SHAPE, sk, denoise_sample_fn_kwargs=dict(dkw, cond_scale=W), x_T=x_T.clone())
    torch.manual_seed(5)
    by_kwarg, _ = d.p_sample_loop("ddim", SHAPE, dict(sk, cfg_distilled=True), denoise_sample_fn_kwargs=dict(dkw), x_T=x_T.clone())
    torch.manual_seed(5)
    guided, _ = d.p_sample_loop("ddim", SHAPE, sk, denoise_sample_fn_kwargs=dict(dkw, cond_scale=W), x_T=x_T.clone())
    assert torch.equal(by_hparam, by_kwarg) and not torch.equal(by_kwarg, guided)
    (g,) = [s for s in m.__dict__["_hip_graph_steps"].values() if s.distilled]
    assert isinstance(g, Dm._GraphedStep) and g.replays == dict(guided=0, cond=len(_times(d, "ddim", 6)))
