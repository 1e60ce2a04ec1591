"""Progressive distillation on the HIP path (Salimans & Ho 2022, Algorithm 2 = stage 2 of Meng et al. 2023): csrc/progressive.hip:
sgd_pd_half_step, sgd_pd_loss_fwd / sgd_pd_loss_bwd; sgdm_amd/losses.py: _ProgressiveLossFn, p_losses_hip with the hparam
progressive_steps; sgdm_amd/train.py: progressive_next_stage; sgdm_amd/diffusion.py: the sampling defaults.  The reference has no
counterpart; the expected values are the formulas restated here -- z_mid, head and the gradient in torch fp32, product by product
in the kernels' documented order (bit-exact gate), the loss in float64 over the same fp32 inputs -- and the project's own paths:
one teacher-forced step of the ddim sampler on the 2K-step trailing grid, and the explicit-target training step through
progressive_target_torch and _MSEFn.  GPU only.

Bounds (those of tests/test_hip_distill.py, whose device core these kernels share): per-sample loss 1e-6 relative against float64,
z_mid / head / gradient bit-equal to torch fp32, gradient 1e-5 rel-L2 against float64; z_mid against the sampler's own step 1e-4
rel-L2 (the project's parity contract: that kernel contracts and divides); training step: loss 1e-6 relative, first / last
parameter gradient 1e-4 max-rel against the explicit-target step.  Every test prints the figure it asserts on (run with -s).
Measured on the MI355X: per-sample loss at most 1.0e-7 from float64, z_mid / head / gradient bit-equal to torch fp32, gradient at
most 4.9e-7 rel-L2 from float64; z_mid 7.6e-8 rel-L2 from the sampler's step; training step loss at most 1.1e-7, parameter
gradients bit-equal (at most 1.7e-6 with trunc_snr) to the explicit-target step; fixed batch, 8 steps at K = 4: last / first loss
0.148."""
import functools

import pytest
import torch

from conftest import max_rel, rel_l2
from test_hip_distill import SHAPES, _attach, _batch, _count, _dev, _diffusion, _rel, _sampling_inputs, _step, _student
from test_hip_unet import build_model
from test_hip_vpred import _guided32, _sk, _st

pytestmark = pytest.mark.gpu

T, S, N, W, K = 1000, 16, 4, 2.0, 4
PARS = ("eps", "x0", "v")


@functools.lru_cache(maxsize=None)
def _rows32(par, k=K):
    """the table the host uploads: progressive_rows rounded once, [k, 8] fp32 (include/sgdm_hip.h: sgd_pd_row)"""
    from sgdm_amd.diffusion import progressive_rows
    ac = _diffusion(parameterization=par).sampler.alphas_cumprod
    tab = torch.zeros(k, 8, dtype=torch.float32)
    tab[:, :5] = progressive_rows(ac, k, par).float()
    return tab


# ---------------------------------------------------------------------------------------------------------------- kernels

def _case(b, c, hw, mode, w, seed, offset, rows):
    """z_t NCHW [b, c, hw], the teacher's two raw outputs NHWC [2b | b, hw, c] and the student's output; a few elements have
    z_t and both teacher outputs 0, so that the target is 0 exactly in fp32 AND in float64, and `out` 0 there: d == 0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, hw, generator=g)
    t1, t2 = (torch.randn(2 * b if mode else b, hw, c, generator=g) for _ in range(2))
    zero = torch.zeros(b, c, hw, dtype=torch.bool)
    zero.view(-1)[::7] = True
    z = zero.permute(0, 2, 1)
    x[zero] = 0.0
    for tt in (t1, t2):
        tt[:b][z] = 0.0
        if mode:
            tt[b:][z] = 0.0
    idx = torch.tensor(([0, K - 1, 1, 2] * b)[:b]) if b > 1 else torch.tensor([K - 1 - seed % 2 * (K - 1)])
    zm, head, target = _restate_target(x, t1, t2, mode, w, idx, rows, torch.float32)
    out = target + 1.2 * torch.randn(b, c, hw, generator=g)
    out[zero] = 0.0
    d = out - target
    assert bool((d == 0).any()) and not target[zero].any()
    if c * hw >= 64:
        assert bool((d.abs() > 1).any()) and bool(((d.abs() < 1) & (d != 0)).any())
    t = torch.randint(0, T, (b,), generator=g)
    return dict(x=_dev(x, offset), t1=_dev(t1, offset), t2=_dev(t2, offset), out=_dev(out, offset), idx=idx.cuda(), t=t.cuda(),
                host=(x, t1, t2, out, idx, t))


def _restate_target(x, t1, t2, mode, w, idx, rows, dtype):
    """(z_mid, head, target) in `dtype` from the fp32 inputs and the fp32 rows; in fp32 every product is rounded before it is
    added, in the kernels' order: z_mid = a1 x + b1 g1, head = d0 x + d1 g1, target = head + d2 g2"""
    b = x.shape[0]
    xx, r = x.to(dtype), rows.to(dtype)[idx]
    a1, b1, d0, d1, d2 = (r[:, k].view(b, 1, 1) for k in range(5))

    def guided(tc):
        tc = tc.to(dtype)
        if dtype == torch.float32:
            return _guided32(tc, mode, w, b).permute(0, 2, 1)
        return (tc if mode == 0 else (1.0 - w) * tc[b:] + w * tc[:b] if mode == 1 else (1.0 + w) * tc[:b] - w * tc[b:]).permute(0, 2, 1)
    g1, g2 = guided(t1), guided(t2)
    zm = a1 * xx + b1 * g1
    head = d0 * xx + d1 * g1
    return zm, head, head + d2 * g2


def _restate_loss(host, mode, w, rows, wt, kind, gper, gscale, dtype):
    """(per_raw, per_w, gout) in `dtype`; the gradient in the kernel's order: k = (gper * wt[t]) / chw, k = k * gscale,
    g = (2 k) d | k sign(d) | k clamp(d, -1, 1)"""
    x, t1, t2, out, idx, t = host
    b, c, hw = out.shape
    d = out.to(dtype) - _restate_target(x, t1, t2, mode, w, idx, rows, dtype)[2]
    el = d * d if kind == 0 else d.abs() if kind == 1 else torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    wts = wt.cpu().to(dtype)[t] if wt is not None else torch.ones(b, dtype=dtype)
    raw = el.reshape(b, -1).mean(1)
    k = (gper.to(dtype) * wts) / torch.tensor(float(c * hw), dtype=dtype)
    k = (k * torch.tensor(gscale, dtype=dtype)).view(b, 1, 1)
    g = (2 * k) * d if kind == 0 else k * torch.sign(d) if kind == 1 else k * d.clamp(-1, 1)
    return raw, wts * raw, g


def _guarded(n, offset):
    """a NaN-filled buffer and the [n] view `offset` floats in that a kernel writes"""
    buf = torch.full((n + 4,), float("nan"), device="cuda")
    return buf, buf[offset:offset + n]


def _untouched(buf, n, offset):
    return bool(torch.isnan(torch.cat([buf[:offset], buf[offset + n:]])).all())


def _half(lib, cs, mode, w_dev, rows_dev, b, c, hw, offset):
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    n = b * c * hw
    (bz, zm), (bh, head) = _guarded(n, offset), _guarded(n, offset)
    L.check(lib.sgd_pd_half_step(_ptr(cs["x"]), _ptr(cs["t1"]), mode, _ptr(w_dev), cs["idx"].data_ptr(), rows_dev.data_ptr(), b, c, hw,
                                 _ptr(zm), _ptr(head), _st()), "sgd_pd_half_step")
    torch.cuda.synchronize()
    assert _untouched(bz, n, offset) and _untouched(bh, n, offset)          # nothing written outside [b, c, hw]
    return zm.view(b, c, hw), head.view(b, c, hw)


def _fwd(lib, cs, head, mode, w_dev, rows_dev, wt, kind, b, c, hw):
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    bufs = [torch.full((b + 2,), float("nan"), device="cuda") for _ in range(2)]
    raw, pw = (v[1:1 + b] for v in bufs)
    L.check(lib.sgd_pd_loss_fwd(_ptr(cs["out"]), _ptr(head), _ptr(cs["t2"]), mode, _ptr(w_dev), cs["idx"].data_ptr(), rows_dev.data_ptr(),
                                _ptr(cs["t"]), _ptr(wt), kind, b, c, hw, _ptr(raw), _ptr(pw), _st()), "sgd_pd_loss_fwd")
    torch.cuda.synchronize()
    for v in bufs:                                                  # nothing written outside [b]
        assert bool(torch.isnan(v[0])) and bool(torch.isnan(v[-1]))
    return raw.clone(), pw.clone()


def _bwd(lib, cs, head, mode, w_dev, rows_dev, wt, kind, b, c, hw, gper, gscale, offset):
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    n = b * c * hw
    buf, gout = _guarded(n, offset)
    L.check(lib.sgd_pd_loss_bwd(_ptr(cs["out"]), _ptr(head), _ptr(cs["t2"]), mode, _ptr(w_dev), cs["idx"].data_ptr(), rows_dev.data_ptr(),
                                _ptr(cs["t"]), _ptr(wt), kind, b, c, hw, gper.data_ptr(), gscale, _ptr(gout), _st()), "sgd_pd_loss_bwd")
    torch.cuda.synchronize()
    assert _untouched(buf, n, offset)
    return gout.view(b, c, hw)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("b,c,hw,offset", SHAPES)
def test_kernels_every_guided_form_and_loss(b, c, hw, offset, mode):
    from sgdm_amd import _lib as L
    lib = L.load()
    table = torch.rand(T, generator=torch.Generator().manual_seed(5)).cuda() + 0.25
    worst_f, worst_g = 0.0, 0.0
    for kind in range(3):
        w, rows = (W, -0.3, 7.5)[kind], _rows32(PARS[kind])             # (the rows of another parameterization per loss kind)
        w_dev, rows_dev = torch.tensor([w], dtype=torch.float32, device="cuda"), rows.cuda()
        cs = _case(b, c, hw, mode, w, seed=31 * mode + 7 * kind + hw % 5, offset=offset, rows=rows)
        x, t1, t2, out, idx, t = cs["host"]
        if b > 1:
            assert 0 in idx.tolist() and K - 1 in idx.tolist()
        # the half step: both outputs bit-equal to the fp32 restatement, run to run identical
        zm, head = _half(lib, cs, mode, w_dev, rows_dev, b, c, hw, offset)
        zm32, head32, _ = _restate_target(x, t1, t2, mode, w, idx, rows, torch.float32)
        assert torch.equal(zm.cpu(), zm32), (mode, kind, float((zm.cpu() - zm32).abs().max()))
        assert torch.equal(head.cpu(), head32), (mode, kind, float((head.cpu() - head32).abs().max()))
        zm_b, head_b = _half(lib, cs, mode, w_dev, rows_dev, b, c, hw, offset)
        assert torch.equal(zm, zm_b) and torch.equal(head, head_b)
        gper = torch.rand(b, generator=torch.Generator().manual_seed(hw + mode)) + 0.5
        for wt, gscale in ((table, 1.0), (None, 3.0)):
            raw, pw = _fwd(lib, cs, head, mode, w_dev, rows_dev, wt, kind, b, c, hw)
            raw2, pw2 = _fwd(lib, cs, head, mode, w_dev, rows_dev, wt, kind, b, c, hw)
            gout = _bwd(lib, cs, head, mode, w_dev, rows_dev, wt, kind, b, c, hw, gper.cuda(), gscale, offset)
            assert torch.equal(raw, raw2) and torch.equal(pw, pw2)                  # fixed fold order: run-to-run identical
            assert torch.equal(gout, _bwd(lib, cs, head, mode, w_dev, rows_dev, wt, kind, b, c, hw, gper.cuda(), gscale, offset))
            _, _, g32 = _restate_loss(cs["host"], mode, w, rows, wt, kind, gper, gscale, torch.float32)
            raw64, pw64, g64 = _restate_loss(cs["host"], mode, w, rows, wt, kind, gper, gscale, torch.float64)
            assert torch.equal(gout.cpu(), g32), (mode, kind, wt is not None, float((gout.cpu() - g32).abs().max()))
            worst_f = max(worst_f, _rel(raw, raw64), _rel(pw, pw64))
            worst_g = max(worst_g, rel_l2(gout.cpu(), g64))
            if wt is None:
                assert torch.equal(raw, pw)
    print(f"progressive kernels (b, c, hw) = {(b, c, hw)} offset {offset} mode {mode}: z_mid, head and gradient bit-equal to torch "
          f"fp32; per-sample loss max rel {worst_f:.2e}, gradient max rel-L2 vs float64 {worst_g:.2e}")
    assert worst_f <= 1e-6
    assert worst_g <= 1e-5


@pytest.mark.parametrize("b,c,hw,offset", SHAPES)
def test_zero_d2_and_zero_head_reduce_to_the_distillation_loss(b, c, hw, offset):
    """rows (.., d0 = 0, d1 = 0, d2 = 1): head is 0 and the target is the guided second output -- sgd_distill_loss_fwd / _bwd on
    that output agree bit for bit (the same device core)"""
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    rows = torch.zeros(K, 8)
    rows[:, 0], rows[:, 4] = 1.0, 1.0
    w_dev, rows_dev = torch.tensor([W], dtype=torch.float32, device="cuda"), rows.cuda()
    cs = _case(b, c, hw, 2, W, seed=hw, offset=offset, rows=rows)
    zm, head = _half(lib, cs, 2, w_dev, rows_dev, b, c, hw, offset)
    assert torch.equal(zm, cs["x"]) and not bool(head.any())
    gper = (torch.rand(b, generator=torch.Generator().manual_seed(3)) + 0.5).cuda()
    for kind in range(3):
        raw, pw = _fwd(lib, cs, head, 2, w_dev, rows_dev, None, kind, b, c, hw)
        gout = _bwd(lib, cs, head, 2, w_dev, rows_dev, None, kind, b, c, hw, gper, 1.0, offset)
        raw_d, pw_d, g_d = torch.empty(b, device="cuda"), torch.empty(b, device="cuda"), torch.empty(b * c * hw + 4, device="cuda")
        g_d = g_d[offset:offset + b * c * hw].view(b, c, hw)
        L.check(lib.sgd_distill_loss_fwd(_ptr(cs["out"]), _ptr(cs["t2"]), 2, _ptr(w_dev), _ptr(cs["t"]), None, kind, b, c, hw,
                                         _ptr(raw_d), _ptr(pw_d), _st()), "sgd_distill_loss_fwd")
        L.check(lib.sgd_distill_loss_bwd(_ptr(cs["out"]), _ptr(cs["t2"]), 2, _ptr(w_dev), _ptr(cs["t"]), None, kind, b, c, hw,
                                         gper.data_ptr(), 1.0, _ptr(g_d), _st()), "sgd_distill_loss_bwd")
        torch.cuda.synchronize()
        assert torch.equal(raw, raw_d) and torch.equal(pw, pw_d), (kind, raw.tolist(), raw_d.tolist())
        assert torch.equal(gout, g_d)


def test_entry_points_refuse_bad_arguments():
    from sgdm_amd.unet import _ptr
    from sgdm_amd import _lib as L
    lib = L.load()
    f, t = torch.zeros(128, device="cuda"), torch.zeros(2, dtype=torch.long, device="cuda")
    rows = torch.zeros(K, 8, device="cuda")
    o1, o2 = torch.full((64,), -7.0, device="cuda"), torch.full((64,), -7.0, device="cuda")
    half = dict(x=_ptr(f), teach=_ptr(f), mode=2, w=_ptr(f), idx=t.data_ptr(), rows=rows.data_ptr(), b=1, c=4, hw=8, zm=_ptr(o1),
                head=_ptr(o2), st=_st())
    fwd = dict(out=_ptr(f), head=_ptr(f), teach=_ptr(f), mode=2, w=_ptr(f), idx=t.data_ptr(), rows=rows.data_ptr(), t=_ptr(t),
               wt=_ptr(f), kind=0, b=1, c=4, hw=8, raw=_ptr(o1), pw=_ptr(o2), st=_st())
    bwd = dict(out=_ptr(f), head=_ptr(f), teach=_ptr(f), mode=2, w=_ptr(f), idx=t.data_ptr(), rows=rows.data_ptr(), t=_ptr(t),
               wt=_ptr(f), kind=0, b=1, c=4, hw=8, gper=f.data_ptr(), gscale=1.0, gout=_ptr(o1), st=_st())
    common = (dict(teach=None), dict(idx=None), dict(rows=None), dict(b=0), dict(b=-1), dict(c=0), dict(c=-3), dict(hw=0),
              dict(hw=-4), dict(mode=3), dict(mode=-1), dict(w=None), dict(mode=1, w=None), dict(c=2 ** 20, hw=2 ** 20),
              dict(b=2 ** 30))
    loss = (dict(out=None), dict(head=None), dict(t=None), dict(kind=3), dict(kind=-1))
    for args, fn, own in ((half, lib.sgd_pd_half_step, (dict(x=None), dict(zm=None), dict(head=None))),
                          (fwd, lib.sgd_pd_loss_fwd, loss + (dict(raw=None), dict(pw=None))),
                          (bwd, lib.sgd_pd_loss_bwd, loss + (dict(gper=None), dict(gout=None)))):
        for bad in common + own:                                    # (keyword order is the C argument order)
            assert fn(*dict(args, **bad).values()) == 1, (fn.__name__, bad)     # SGD_ERR_ARG: refused before any launch
    torch.cuda.synchronize()
    assert bool((o1 == -7.0).all()) and bool((o2 == -7.0).all())               # nothing written
    for args, fn in ((half, lib.sgd_pd_half_step), (fwd, lib.sgd_pd_loss_fwd), (bwd, lib.sgd_pd_loss_bwd)):
        for ok in (dict(mode=0, w=None), {}) + ((dict(wt=None),) if "wt" in args else ()):    # what a call does not read may be missing
            assert fn(*dict(args, **ok).values()) == 0, (fn.__name__, ok)
    torch.cuda.synchronize()
    assert not bool((o1 == -7.0).all())
    # host memory where the kernels dereference is a TypeError in the binding, not a fault on the device
    import ctypes as C
    with pytest.raises(C.ArgumentError):
        lib.sgd_pd_half_step(*dict(half, rows=(C.c_float * 8)()).values())


# ------------------------------------------------------------------------------------------- against the project's own sampler

B = 4
SHAPE = (B, 3, S, S)


@pytest.fixture(scope="module")
def pair():
    """the c32 student in training mode (f32), a frozen teacher that differs from it, one fixed batch"""
    from sgdm_amd.train import distill_teacher_from
    m, entry = _student("uf_clusterlayout_c32_s16", "f32")
    teacher = distill_teacher_from(m)
    with torch.no_grad():
        teacher.P("out.2.weight").mul_(1.5)
        teacher.P("out.2.bias").mul_(1.5)
    return (m, teacher) + _batch(entry)


@pytest.mark.parametrize("i", [0, K - 1])
@pytest.mark.parametrize("guided", [True, False])
def test_half_step_is_the_samplers_own_ddim_step(guided, i, pair):
    """z_mid of sgd_pd_half_step against ONE teacher-forced step of the ddim sampler (row 2 i + 1 of the 2K-step trailing grid,
    x_T = z_t, eta 0, no clip) of the same teacher on the same input"""
    from sgdm_amd.losses import _distill_teacher_eval, progressive_half_step
    _, teacher, x0, noise, ukw = pair
    d = _diffusion(progressive_steps=K, **(dict(distill_guidance=W) if guided else {}))
    d.set_denoise_fn(teacher.forward, teacher.forward_with_cond_scale)
    idx = torch.full((B,), i, dtype=torch.long, device="cuda")
    t = (idx + 1) * (T // K) - 1
    z_t = d.sampler.q_sample(x0, noise, t).contiguous()
    with torch.no_grad():
        teach, mode, w_dev = _distill_teacher_eval(d, teacher, W if guided else None, 0.0, z_t, t, ukw)
        z_mid, _ = progressive_half_step(z_t, teach, mode, w_dev, idx, d.progressive_rows_dev(z_t.device))
    assert mode == (teacher._scale_mode() if guided else 0) and teach.shape[0] == (2 * B if guided else B)
    dkw = dict(ukw, cond_scale=W) if guided else dict(ukw)
    skx = {} if guided else dict(cfg_distilled=True)
    sk = _sk(d, "ddim", 2 * K, timestep_spacing="trailing", **skx)
    sk["clip_denoised"] = False
    want, _ = d.sampler_list["ddim"].sample(shape=SHAPE, sampling_kwargs=sk, denoise_sample_fn=d.denoise_sample_fn,
                                            denoise_sample_fn_kwargs=dkw, x_T=z_t.clone(), step_indices=[2 * i + 1])
    times = d.sampler_list["ddim"].ddim_timesteps
    assert int(times[2 * i + 1]) == int(t[0]) and int(times[2 * i]) == int(t[0]) - T // (2 * K)    # the rows t and m
    err = rel_l2(z_mid.cpu(), want.cpu())
    print(f"half step vs the ddim sampler's step, guided {guided}, grid point {i} (t = {int(t[0])}): rel-L2 {err:.2e}")
    assert err <= 1e-4


# --------------------------------------------------------------------------------------------------------------- training

ENTRIES = ("sgd_pd_half_step", "sgd_pd_loss_fwd", "sgd_pd_loss_bwd", "sgd_distill_loss_fwd", "sgd_distill_loss_bwd",
           "sgd_cfg_combine", "sgd_cfg_guide", "sgd_nhwc_to_nchw", "sgd_q_sample", "sgd_q_sample_v", "sgd_loss_fwd", "sgd_loss_bwd")


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("par,weighting", [("eps", None), ("v", None), ("v", "trunc_snr")])
def test_training_step_against_the_explicit_target(par, weighting, guided, pair, monkeypatch):
    """one progressive p_losses + backward on the c32 model against the same student step with the target built by the torch
    chain (progressive_target_torch) from two forward_with_cond_scale calls of the teacher and fed to _MSEFn; the launches
    counted: one half step, one loss kernel each way, no combine, no re-layout of either teacher output"""
    from sgdm_amd.losses import _MSEFn, progressive_target_torch
    m, teacher, x0, noise, ukw = pair
    hp = dict(distill_guidance=W) if guided else {}
    d = _diffusion(parameterization=par, loss_weighting=weighting, progressive_steps=K, **hp).train()
    seen = _attach(d, m)
    d.set_distill_teacher(teacher)
    t = torch.tensor([0, 999, 250, 731]).cuda()
    idx = t // (T // K)
    ts = (idx + 1) * (T // K) - 1
    assert idx.tolist() == [0, 3, 1, 2]
    calls = _count(monkeypatch, *ENTRIES)
    loss, ld, first, last = _step(d, m, x0, t, noise, dict(ukw, cond_drop_prob=0.5))
    # (the one sgd_nhwc_to_nchw is the student's own output)
    assert calls == dict(sgd_pd_half_step=1, sgd_pd_loss_fwd=1, sgd_pd_loss_bwd=1, sgd_distill_loss_fwd=0, sgd_distill_loss_bwd=0,
                         sgd_cfg_combine=0, sgd_cfg_guide=0, sgd_nhwc_to_nchw=1, sgd_q_sample=1, sgd_q_sample_v=0, sgd_loss_fwd=0,
                         sgd_loss_bwd=0)
    assert seen["kw"]["cond_drop_prob"] == 0.0
    assert torch.equal(ld["train/epoch_stats_x"], ts)                       # the snapped timestep
    s = d.sampler
    sa, s1 = s.sqrt_alphas_cumprod[ts].view(N, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod[ts].view(N, 1, 1, 1)
    assert torch.equal(seen["x_noisy"], sa * x0 + s1 * noise)       # the bits of the plain path's x_noisy, at the snapped t
    # the same student step with the explicit target
    m.zero_grad(set_to_none=True)

    def teacher_eval(z, tt):
        if guided:
            return teacher.forward_with_cond_scale(z, tt, W, **ukw)
        return teacher.forward_with_cond_scale(z, tt, 1, **ukw)             # imagen scale type: the conditional evaluation
    with torch.no_grad():
        target = progressive_target_torch(_rows32(par), idx, seen["x_noisy"], teacher_eval, ts, ts - T // (2 * K))
    out = m.forward(seen["x_noisy"], ts, cond_drop_prob=0.0, **ukw)[0]
    assert torch.equal(out.detach(), seen["out"])
    per = _MSEFn.apply(out, target)
    want = (per if weighting is None else per * s.loss_weights[ts]).mean()
    want.backward()
    params = [p for p in m.parameters() if p.requires_grad]
    want = float(want.detach())
    err_l = abs(float(loss) - want) / want
    err_y = max_rel(ld["train/epoch_stats_y"].cpu(), per.detach().cpu())
    err_f, err_b = max_rel(first, params[0].grad), max_rel(last, params[-1].grad)
    print(f"progressive step {par} weighting {weighting} guided {guided}: loss {float(loss):.4e}, rel err {err_l:.2e}, per-sample "
          f"{err_y:.2e}; grad first / last parameter vs explicit target {err_f:.2e} / {err_b:.2e}")
    assert float(first.abs().max()) > 0 and float(last.abs().max()) > 0
    assert all(p.grad is None for p in teacher.parameters())
    assert err_l <= 1e-6
    assert err_f < 1e-4 and err_b < 1e-4


def test_a_fixed_batch_is_learned():
    """8 steps on one batch at K = 4, lr 1e-3, a guided teacher at w = 2 (stages 1 and 2 in one), the student initialised from
    the teacher: the loss goes down"""
    from sgdm_amd.optim import FusedAdamWEma
    from sgdm_amd.train import distill_teacher_from
    m, entry = _student("ca_stego_c32_s16", "f16x3")
    x0, noise, ukw = _batch(entry)
    teacher = distill_teacher_from(m)
    d = _diffusion(progressive_steps=K, distill_guidance=W).train()
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
    print(f"fixed batch, 8 steps at K = {K}: losses {[f'{v:.4e}' for v in losses]}, last / first {losses[-1] / losses[0]:.3f}")
    assert all(v == v for v in losses) and losses[-1] < losses[0]


def test_next_stage_trains_against_the_frozen_student():
    """progressive_next_stage on the device: K 4 -> 2, the teacher a frozen copy evaluated ONCE per teacher step at B"""
    from sgdm_amd import _lib as L
    from sgdm_amd.train import distill_teacher_from, progressive_next_stage
    m, entry = _student("uf_clusterlayout_c32_s16", "f32")
    x0, noise, ukw = _batch(entry)
    d = _diffusion(progressive_steps=K, distill_guidance=W).train()
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    d.set_distill_teacher(distill_teacher_from(m))
    t = torch.tensor([0, 999, 250, 731]).cuda()
    first, _ = d.p_losses(x0, t, noise, **ukw)
    first.backward()
    assert d.progressive_rows_dev(x0.device).shape == (K, 8)
    assert progressive_next_stage(d) == K // 2
    teacher = d._distill_teacher
    loss, ld = d.p_losses(x0, t, noise, **ukw)
    loss.backward()
    assert d.progressive_rows_dev(x0.device).shape == (K // 2, 8)
    assert sorted(teacher._engines) == [(N, S, S, L.PREC_BY_NAME["f32"])]   # one conditional evaluation at B: no 2B engine
    assert ld["train/epoch_stats_x"].tolist() == [499, 999, 499, 999]
    print(f"next stage: loss at K = {K} (guided teacher) {float(first):.4e}, at K = {K // 2} (frozen student) {float(loss):.4e}")
    assert float(loss) == float(loss) and float(loss) > 0


# --------------------------------------------------------------------------------------------------------------- sampling

def _loop_sk(**kw):
    return dict(dict(sampling_method="ddim", vis=None, log_num_per_prog=10, clip_denoised=True, dtp=1, temperature=1.0,
                     noise_dropout=0, random_sample_condition=False, return_inter_dict=True, disable_tqdm=True), **kw)


def test_sampling_defaults_walk_the_students_grid():
    """progressive_steps = 4 and no step kwargs: the bytes of the call with the four kwargs spelled out on a model without the
    hparam, 4 evaluations at batch B, no 2B engine"""
    from sgdm_amd import _lib as L
    m, entry = build_model("uf_clusterlayout_c32_s16", "f16x3")
    dkw, x_T = _sampling_inputs(entry)
    shape = tuple(x_T.shape)
    d = _diffusion(progressive_steps=K)
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    torch.manual_seed(5)
    got, _ = d.p_sample_loop("ddim", shape, _loop_sk(), denoise_sample_fn_kwargs=dict(dkw, cond_scale=W), x_T=x_T.clone())
    assert sorted(m._engines) == [(shape[0], S, S, L.PREC_BY_NAME[m.hip_precision])], sorted(m._engines)
    (g,) = list(m.__dict__["_hip_graph_steps"].values())
    assert g.distilled and g.replays == dict(guided=0, cond=K), g.replays
    plain = _diffusion()
    plain.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    torch.manual_seed(5)
    want, _ = plain.p_sample_loop("ddim", shape, _loop_sk(num_timesteps=K, ddim_eta=0, timestep_spacing="trailing", cfg_distilled=True),
                                  denoise_sample_fn_kwargs=dict(dkw), x_T=x_T.clone())
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    # an explicit kwarg still wins: 6 steps is another trajectory
    torch.manual_seed(5)
    six, _ = d.p_sample_loop("ddim", shape, _loop_sk(num_timesteps=6), denoise_sample_fn_kwargs=dict(dkw), x_T=x_T.clone())
    assert not torch.equal(six, got)
    assert sorted(m._engines) == [(shape[0], S, S, L.PREC_BY_NAME[m.hip_precision])]


def test_without_the_hparam_training_and_sampling_keep_their_bits(pair):
    m, _, x0, noise, ukw = pair
    t = torch.tensor([0, 999, 250, 731]).cuda()
    steps = []
    for kw in ({}, dict(progressive_steps=None)):
        d = _diffusion(parameterization="v", loss_weighting="min_snr", **kw).train()
        d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
        torch.manual_seed(11)
        steps.append(_step(d, m, x0, t, noise, dict(ukw, cond_drop_prob=0.5)))
    (l0, ld0, f0, b0), (l1, ld1, f1, b1) = steps
    assert torch.equal(l0, l1) and torch.equal(f0, f1) and torch.equal(b0, b1) and sorted(ld0) == sorted(ld1)
    assert torch.equal(ld0["train/epoch_stats_x"], t)
    ms, entry = build_model("uf_clusterlayout_c32_s16", "f16x3")
    dkw, x_T = _sampling_inputs(entry)
    runs = []
    for kw in ({}, dict(progressive_steps=None)):
        d = _diffusion(**kw)
        d.set_denoise_fn(ms.forward, ms.forward_with_cond_scale)
        torch.manual_seed(5)
        runs.append(d.p_sample_loop("ddim", tuple(x_T.shape), _loop_sk(num_timesteps=6, ddim_eta=0.0),
                                    denoise_sample_fn_kwargs=dict(dkw, cond_scale=W), x_T=x_T.clone())[0])
    assert torch.equal(runs[0], runs[1])
