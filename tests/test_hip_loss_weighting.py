"""Loss weighting on the HIP path (csrc/loss.hip: sgd_loss_fwd, sgd_loss_bwd; sgdm_amd/train.py: _WeightedLossFn, p_losses_hip;
sgdm_amd/diffusion.py: loss_weight_table).  The reference weighs every timestep alike; the expected values are the formulas
restated here -- the gradient in torch fp32, product by product in the kernel's documented order (bit-exact gate), the loss
in float64 over the same fp32 inputs -- and the project's own unweighted path (equivalence gates).  GPU only.

Bounds: loss 1e-6 relative (one fp32 rounding of a double sum of fp32 terms whose own roundings average out), gradient 1e-5
rel-L2 against float64 (an element-wise fp32 kernel), parameter gradients 1e-4 max-rel (tests/test_hip_vpred.py).
Every test prints the figure it asserts on (run with -s).  Measured on the MI355X: per-sample loss at most 9.9e-8 from float64,
gradient bit-equal to torch fp32 and at most 9.1e-8 rel-L2 from float64; training step loss 8.2e-9 ('v' + min_snr) / 1.0e-7
('eps' + p2), parameter gradients at most 1.6e-6 from the explicit-weight step; a table of ones against the default path:
per-sample loss at most 1.1e-7 apart, first and last gradient bit-equal."""
import pytest
import torch

from conftest import max_rel, rel_l2
from test_hip_unet import build_model

pytestmark = pytest.mark.gpu

T, S, GAMMA = 1000, 16, 5.0
PARS, KINDS = ("eps", "x0", "v"), ("l2", "l1", "huber")


def _diffusion(**kw):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, **kw))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _pick_t(sampler):
    """table indices on both sides of min(SNR, gamma)'s clamp: SNR > gamma, SNR < gamma, nearest the crossing, 0 and T-1"""
    a = sampler.alphas_cumprod.double().cpu()
    snr = a / (1 - a)
    hi, lo = int((snr > 2 * GAMMA).nonzero()[-1]), int((snr < GAMMA / 2).nonzero()[0])
    cross = int((snr - GAMMA).abs().argmin())
    assert snr[hi] > GAMMA > snr[lo] and 0 < hi < cross < lo < T - 1
    return [hi, lo, cross, 0, T - 1]


@pytest.fixture(scope="module")
def tables():
    """(sa, s1, wt, t list) on the device for the plain and the zero-terminal-SNR schedule, 'v' + min_snr"""
    out = {}
    for name, kw in (("plain", {}), ("zt", dict(zero_terminal_snr=True))):
        s = _diffusion(parameterization="v", loss_weighting="min_snr", loss_weighting_gamma=GAMMA, **kw).sampler
        out[name] = (s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod, s.loss_weights, _pick_t(s))
    assert float(out["zt"][0][-1]) == 0.0 and float(out["zt"][2][-1]) == 0.0           # sa == 0, weight == 0 at T-1
    return out


def _case(b, chw, par, kind, tab, seed, offset=0):
    """device tensors of one kernel call ([b, chw] each; `offset` floats past a 16-byte boundary), `out` drawn so that
    |d| lies on both sides of 1 and a few elements have d == 0 exactly"""
    sa, s1, wt, ts = tab
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor([ts[(i + seed) % len(ts)] for i in range(b)], dtype=torch.long)
    x0, noise = torch.randn(b, chw, generator=g), torch.randn(b, chw, generator=g)
    a, s = sa.cpu()[t].view(b, 1), s1.cpu()[t].view(b, 1)
    if par == 2:                        # (a v target that is exact in fp32 AND in float64, so that d == 0 in both)
        x0.view(-1)[::7] = 0.0
        noise.view(-1)[::7] = 0.0
    target = noise if par == 0 else x0 if par == 1 else a * noise - s * x0
    out = target + 1.2 * torch.randn(b, chw, generator=g)
    out.view(-1)[::7] = target.reshape(-1)[::7]                     # d == 0 exactly: l1's sign(0) = 0
    d = out - target
    assert bool((d == 0).any())
    if chw >= 64:
        assert bool((d.abs() > 1).any()) and bool(((d.abs() < 1) & (d != 0)).any())

    def dev(x):
        buf = torch.empty(x.numel() + 4, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[offset:offset + x.numel()].view(x.shape)
        v.copy_(x)
        return v
    return dict(out=dev(out), x0=dev(x0), noise=dev(noise), t=t.cuda(), host=(out, x0, noise, t))


def _launch_fwd(lib, c, tab, par, kind, weighted, b, chw):
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    sa, s1, wt, _ = tab
    raw, pw = torch.full((b,), float("nan"), device="cuda"), torch.full((b,), float("nan"), device="cuda")
    L.check(lib.sgd_loss_fwd(_ptr(c["out"]), _ptr(c["x0"]), _ptr(c["noise"]), _ptr(c["t"]), _ptr(sa), _ptr(s1),
                             _ptr(wt if weighted else None), par, kind, b, chw, _ptr(raw), _ptr(pw), _st()), "sgd_loss_fwd")
    return raw, pw


def _launch_bwd(lib, c, tab, par, kind, weighted, b, chw, gper, gscale, offset=0):
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    sa, s1, wt, _ = tab
    buf = torch.full((b * chw + 4,), float("nan"), device="cuda")
    gout = buf[offset:offset + b * chw].view(b, chw)
    L.check(lib.sgd_loss_bwd(_ptr(c["out"]), _ptr(c["x0"]), _ptr(c["noise"]), _ptr(c["t"]), _ptr(sa), _ptr(s1),
                             _ptr(wt if weighted else None), gper.data_ptr(), gscale, par, kind, b, chw, _ptr(gout), _st()),
            "sgd_loss_bwd")
    torch.cuda.synchronize()
    guard = torch.cat([buf[:offset], buf[offset + b * chw:]])
    assert bool(torch.isnan(guard).all())                           # nothing written outside [b, chw]
    return gout


def _restate(host, tab, par, kind, weighted, gper, gscale, dtype):
    """(per_raw, per_w, gout) in `dtype` from the fp32 inputs; in fp32 every product is rounded before it is added and the
    gradient follows the kernel's order: k = (gper * w) / chw, k = k * gscale, g = (2 k) d | k sign(d) | k clamp(d, -1, 1)"""
    out, x0, noise, t = (v.to(dtype) if v.is_floating_point() else v for v in host)
    sa, s1, wt, _ = tab
    b, chw = out.shape
    a, s = sa.cpu().to(dtype)[t].view(b, 1), s1.cpu().to(dtype)[t].view(b, 1)
    target = noise if par == 0 else x0 if par == 1 else a * noise - s * x0
    d = out - target
    el = d * d if kind == 0 else d.abs() if kind == 1 else torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    w = wt.cpu().to(dtype)[t] if weighted else torch.ones(b, dtype=dtype)
    raw = el.mean(1)
    k = (gper.to(dtype) * w) / torch.tensor(float(chw), dtype=dtype)
    k = (k * torch.tensor(gscale, dtype=dtype)).view(b, 1)
    g = (2 * k) * d if kind == 0 else k * torch.sign(d) if kind == 1 else k * d.clamp(-1, 1)
    return raw, w * raw, g


def _rel(got, want):
    """max relative error; entries whose expected value is exactly 0 (a zero weight) must be exactly 0"""
    got, want = got.double().cpu(), want.double().cpu()
    z = want == 0
    assert bool((got[z] == 0).all())
    return float(((got - want).abs()[~z] / want.abs()[~z]).max()) if bool((~z).any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------- kernels

# (b, chw, offset in floats): the scalar path (chw % 4 != 0, more than one stride of the workgroup's loop not needed), the
# 16-byte path on one and on several blocks per sample, a sample shorter than a quad, and the 16-byte shapes once more from
# pointers one float past the boundary (scalar path with a partial last block)
SHAPES = [(3, 3 * 35, 0), (2, 4 * 256, 0), (1, 3, 0), (2, 3 * 4096, 0), (2, 3 * 4096, 1), (3, 3 * 35, 1)]


@pytest.mark.parametrize("sched", ["plain", "zt"])
@pytest.mark.parametrize("b,chw,offset", SHAPES)
def test_kernels_every_target_and_loss(b, chw, offset, sched, tables):
    """every par x kind, with and without the weight table, on one shape: the gradient bit-equal to the torch-fp32
    restatement and within 1e-5 rel-L2 of float64, the two per-sample losses within 1e-6 of float64, two launches bit-equal"""
    from sgdm_amd import _lib as L
    lib = L.load()
    tab = tables[sched]
    worst_f, worst_g = 0.0, 0.0
    for par in range(3):
        if sched == "zt" and par == 0:
            continue                                                # no 'eps' model on a zero-terminal-SNR schedule
        for kind in range(3):
            c = _case(b, chw, par, kind, tab, seed=31 * par + 7 * kind + chw % 5, offset=offset)
            gper = torch.rand(b, generator=torch.Generator().manual_seed(chw + par)) + 0.5
            for weighted, gscale in ((True, 1.0), (False, 3.0)):
                raw, pw = _launch_fwd(lib, c, tab, par, kind, weighted, b, chw)
                raw2, pw2 = _launch_fwd(lib, c, tab, par, kind, weighted, b, chw)
                gout = _launch_bwd(lib, c, tab, par, kind, weighted, b, chw, gper.cuda(), gscale, offset)
                assert torch.equal(raw, raw2) and torch.equal(pw, pw2)
                _, _, g32 = _restate(c["host"], tab, par, kind, weighted, gper, gscale, torch.float32)
                raw64, pw64, g64 = _restate(c["host"], tab, par, kind, weighted, gper, gscale, torch.float64)
                assert torch.equal(gout.cpu(), g32), (par, kind, weighted, float((gout.cpu() - g32).abs().max()))
                worst_f = max(worst_f, _rel(raw, raw64), _rel(pw, pw64))
                if float(g64.abs().max()) > 0:
                    worst_g = max(worst_g, rel_l2(gout.cpu(), g64))
                else:
                    assert not gout.any()
                if not weighted:
                    assert torch.equal(raw, pw)
    print(f"loss kernels b={b} chw={chw} offset={offset} [{sched}]: per-sample loss max rel {worst_f:.2e}; gradient bit-equal "
          f"to torch fp32, max rel-L2 vs float64 {worst_g:.2e}")
    assert worst_f <= 1e-6
    assert worst_g <= 1e-5


def test_weighted_loss_at_the_picked_timesteps(tables):
    """one sample per picked index, in order: both sides of the clamp, the crossing, 0, T-1; on the zero-terminal table the
    last sample has sa == 0 (target = noise * 1 - 0) and weight 0"""
    from sgdm_amd import _lib as L
    lib = L.load()
    for sched in ("plain", "zt"):
        tab = tables[sched]
        sa, s1, wt, ts = tab
        b, chw = len(ts), 3 * 64
        c = _case(b, chw, 2, 0, tab, seed=0)
        assert c["host"][3].tolist() == ts
        raw, pw = _launch_fwd(lib, c, tab, 2, 0, True, b, chw)
        gper = torch.full((b,), 1.0 / b)
        gout = _launch_bwd(lib, c, tab, 2, 0, True, b, chw, gper.cuda(), 1.0)
        raw64, pw64, g64 = _restate(c["host"], tab, 2, 0, True, gper, 1.0, torch.float64)
        w = wt.cpu()[ts].double()
        err = max(_rel(raw, raw64), _rel(pw, pw64))
        print(f"picked timesteps {ts} [{sched}]: weights {[round(float(v), 4) for v in w]}, loss max rel {err:.2e}")
        assert err <= 1e-6 and rel_l2(gout.cpu(), g64) <= 1e-5
        if sched == "zt":
            assert float(pw[-1]) == 0.0 and float(raw[-1]) > 0 and not gout[-1].any()


def test_entry_points_refuse_bad_arguments():
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    f, t = torch.zeros(64, device="cuda"), torch.zeros(2, dtype=torch.long, device="cuda")
    fwd = dict(out=_ptr(f), x0=_ptr(f), noise=_ptr(f), t=_ptr(t), sa=_ptr(f), s1=_ptr(f), wt=_ptr(f), par=2, kind=0, b=1, chw=8,
               raw=_ptr(f), pw=_ptr(f), st=_st())
    bwd = dict(out=_ptr(f), x0=_ptr(f), noise=_ptr(f), t=_ptr(t), sa=_ptr(f), s1=_ptr(f), wt=_ptr(f), gper=f.data_ptr(), gscale=1.0,
               par=2, kind=0, b=1, chw=8, gout=_ptr(f), st=_st())
    common = (dict(out=None), dict(t=None), dict(b=0), dict(b=-1), dict(chw=0), dict(chw=-4), dict(par=3), dict(par=-1),
              dict(kind=3), dict(kind=-1), dict(sa=None), dict(s1=None), dict(x0=None), dict(noise=None),
              dict(par=0, noise=None), dict(par=1, x0=None), dict(b=2 ** 20, chw=2 ** 50))
    for args, fn, own in ((fwd, lib.sgd_loss_fwd, (dict(raw=None), dict(pw=None))),
                          (bwd, lib.sgd_loss_bwd, (dict(gper=None), dict(gout=None)))):
        for bad in common + own:                                    # (keyword order is the C argument order)
            assert fn(*dict(args, **bad).values()) == 1, (fn.__name__, bad)     # SGD_ERR_ARG: refused before any launch
        # what a target does not read may be missing
        for ok in (dict(par=0, x0=None, sa=None, s1=None), dict(par=1, noise=None, sa=None, s1=None), dict(wt=None)):
            assert fn(*dict(args, **ok).values()) == 0, (fn.__name__, ok)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------- training

N = 4


@pytest.fixture(scope="module")
def trainer():
    """the c32 model in training mode and one fixed batch"""
    from sgdm_amd.synth import synth_batch
    m, entry = build_model("uf_clusterlayout_c32_s16", "f32")
    m.train()
    kw = entry["ctor"]
    batch = synth_batch(kw["condition_method"], N, S, kw["cond_dim"], entry["layout_dim"], seed=26)
    g = torch.Generator().manual_seed(3)
    x0, noise = batch["image"].cuda(), torch.randn(N, 3, S, S, generator=g).cuda()
    ukw = dict(cond=batch["cond"].float().cuda(), layout=batch["layout"].cuda(), cond_drop_prob=0.5,
               cond_drop_mask=torch.tensor([True, False, False, True]).cuda())
    return m, x0, noise, ukw


def _attach(d, m):
    seen = {}

    def denoise_fn(x, t, **kw):
        out = m.forward(x, t, **kw)
        seen["x_noisy"], seen["out"] = x.detach().clone(), out[0].detach().clone()
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


def _per64(d, par, loss_type, x0, noise, out, t):
    s = d.sampler
    sa, s1 = s.sqrt_alphas_cumprod.double()[t].view(N, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod.double()[t].view(N, 1, 1, 1)
    target = dict(eps=noise.double(), x0=x0.double(), v=sa * noise.double() - s1 * x0.double())[par]
    diff = out.double() - target
    el = diff ** 2 if loss_type == "l2" else diff.abs() if loss_type == "l1" else \
        torch.where(diff.abs() < 1, 0.5 * diff ** 2, diff.abs() - 0.5)
    return el.reshape(N, -1).mean(1)


@pytest.mark.parametrize("par,scheme", [("v", "min_snr"), ("eps", "p2")])
def test_training_step_with_weights(par, scheme, trainer, monkeypatch):
    """one weighted p_losses + backward on the c32 model: the loss against the float64 restatement on the observed x_noisy
    and model output, the gradients against the same step through the existing l2 path times the weights"""
    from sgdm_amd.losses import _MSEFn
    m, x0, noise, ukw = trainer
    d = _diffusion(parameterization=par, loss_weighting=scheme).train()
    seen = _attach(d, m)
    s = d.sampler
    ts = _pick_t(s)
    t = torch.tensor([ts[0], ts[1], ts[2], T - 1]).cuda()
    calls = _count(monkeypatch, "sgd_q_sample_v", "sgd_q_sample", "sgd_loss_fwd", "sgd_loss_bwd")
    loss, ld, first, last = _step(d, m, x0, t, noise, ukw)
    assert calls == dict(sgd_q_sample_v=0, sgd_q_sample=1, sgd_loss_fwd=1, sgd_loss_bwd=1)
    sa, s1 = s.sqrt_alphas_cumprod[t].view(N, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod[t].view(N, 1, 1, 1)
    assert torch.equal(seen["x_noisy"], sa * x0 + s1 * noise)       # the bits of the unweighted path's x_noisy
    per = _per64(d, par, "l2", x0, noise, seen["out"], t)
    w = s.loss_weights[t]
    assert len(set(w.tolist())) == N
    want = (w.double() * per).mean()
    err_l = abs(float(loss) - float(want)) / float(want)
    assert sorted(ld) == ["train/ddpm_loss", "train/ddpm_loss_raw", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    err_y = max_rel(ld["train/epoch_stats_y"].cpu(), per.cpu())
    assert float(ld["train/ddpm_loss_raw"]) == pytest.approx(float(per.mean()), rel=1e-6)
    assert float(ld["train/ddpm_loss"]) == float(loss)
    # the same step with an explicit target and explicit weights
    m.zero_grad(set_to_none=True)
    out = m.forward(seen["x_noisy"], t, **ukw)[0]
    assert torch.equal(out.detach(), seen["out"])
    target = noise if par == "eps" else sa * noise - s1 * x0
    (_MSEFn.apply(out, target) * w).mean().backward()
    params = [p for p in m.parameters() if p.requires_grad]
    err_f, err_b = max_rel(first, params[0].grad), max_rel(last, params[-1].grad)
    print(f"weighted training step {par} + {scheme}, t {t.tolist()}: loss rel err {err_l:.2e}, unweighted per-sample {err_y:.2e}; "
          f"grad first / last parameter vs explicit weights {err_f:.2e} / {err_b:.2e}")
    assert float(first.abs().max()) > 0 and float(last.abs().max()) > 0
    assert err_l < 1e-6 and err_y < 1e-6
    assert err_f < 1e-4 and err_b < 1e-4


@pytest.mark.parametrize("loss_type", KINDS)
@pytest.mark.parametrize("par", ["v", "eps"])
def test_table_of_ones_is_the_default_path(par, loss_type, trainer):
    """a table of ones through the kernels against the project's unweighted path (_MSEFn / the torch l1 and huber branches)
    on the same inputs"""
    m, x0, noise, ukw = trainer
    t = torch.tensor([0, 999, 250, 731]).cuda()
    plain = _diffusion(parameterization=par, loss_type=loss_type).train()
    ones = _diffusion(parameterization=par, loss_type=loss_type, loss_weighting="table", loss_weighting_table=[1.0] * T).train()
    _attach(plain, m), _attach(ones, m)
    loss_p, ld_p, first_p, last_p = _step(plain, m, x0, t, noise, ukw)
    loss_1, ld_1, first_1, last_1 = _step(ones, m, x0, t, noise, ukw)
    err_y = _rel(ld_1["train/epoch_stats_y"], ld_p["train/epoch_stats_y"])
    err_l = abs(float(loss_1) - float(loss_p)) / float(loss_p)
    err_f, err_b = max_rel(first_1, first_p), max_rel(last_1, last_p)
    print(f"table of ones vs default path, {par} {loss_type}: per-sample loss {err_y:.2e}, loss {err_l:.2e}, grad first / last "
          f"{err_f:.2e} / {err_b:.2e}")
    assert float(first_p.abs().max()) > 0 and float(last_p.abs().max()) > 0
    assert err_y <= 1e-6 and err_l <= 1e-6
    assert err_f < 1e-4 and err_b < 1e-4


@pytest.mark.parametrize("par", ["v", "eps"])
def test_without_the_hparam_the_step_is_untouched(par, trainer, monkeypatch):
    """the plain step before and after a weighted step on the same model: bit-equal, and neither new entry is called"""
    m, x0, noise, ukw = trainer
    t = torch.tensor([0, 999, 250, 731]).cuda()
    plain = _diffusion(parameterization=par).train()
    weighted = _diffusion(parameterization=par, loss_weighting="min_snr").train()
    _attach(plain, m), _attach(weighted, m)
    assert not hasattr(plain.sampler, "loss_weights")
    calls = _count(monkeypatch, "sgd_loss_fwd", "sgd_loss_bwd", "sgd_q_sample_v", "sgd_q_sample")
    before = _step(plain, m, x0, t, noise, ukw)
    assert calls == dict(sgd_loss_fwd=0, sgd_loss_bwd=0, sgd_q_sample_v=int(par == "v"), sgd_q_sample=int(par != "v"))
    mid = _step(weighted, m, x0, t, noise, ukw)
    assert calls["sgd_loss_fwd"] == calls["sgd_loss_bwd"] == 1
    after = _step(plain, m, x0, t, noise, ukw)
    assert calls["sgd_loss_fwd"] == calls["sgd_loss_bwd"] == 1
    assert sorted(before[1]) == sorted(after[1]) == ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    assert torch.equal(before[0], after[0]) and torch.equal(before[2], after[2]) and torch.equal(before[3], after[3])
    assert torch.equal(before[1]["train/epoch_stats_y"], after[1]["train/epoch_stats_y"])
    assert not torch.equal(before[0], mid[0]) and not torch.equal(before[2], mid[2])


def test_validation_launches_the_forward_kernel_only(trainer, monkeypatch):
    """p_losses under torch.no_grad() on an eval() diffusion object: the val/ keys, one forward launch, no backward one"""
    m, x0, noise, ukw = trainer
    d = _diffusion(parameterization="v", loss_weighting="min_snr").eval()
    seen = _attach(d, m)
    t = torch.tensor([0, 999, 250, 731]).cuda()
    calls = _count(monkeypatch, "sgd_loss_fwd", "sgd_loss_bwd", "sgd_q_sample_v")
    with torch.no_grad():
        vloss, vd = d.p_losses(x0, t, noise, **ukw)
    assert calls == dict(sgd_loss_fwd=1, sgd_loss_bwd=0, sgd_q_sample_v=0)
    assert sorted(vd) == ["val/ddpm_loss", "val/ddpm_loss_raw", "val/loss"]
    assert not vloss.requires_grad
    per = _per64(d, "v", "l2", x0, noise, seen["out"], t)
    want = (d.sampler.loss_weights[t].double() * per).mean()
    err = abs(float(vloss) - float(want)) / float(want)
    print(f"validation loss vs float64 restatement: rel {err:.2e}")
    assert err < 1e-6
    assert float(vd["val/ddpm_loss"]) == float(vloss) and float(vd["val/ddpm_loss_raw"]) == pytest.approx(float(per.mean()), rel=1e-6)
