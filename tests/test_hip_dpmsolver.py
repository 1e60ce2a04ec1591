"""sampling_method='dpmsolver' (sgdm_amd/diffusion.py: DPMSolverSampler, csrc/dpm.hip: sgd_dpmpp_step): DPM-Solver++(2M).
The reference has no such sampler; the expected values are the method restated here -- in torch fp32 in the kernel's
documented operation order (bit-exact gates) and in float64 from the formulas (accuracy gates).  GPU only."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_hip_unet import build_model

pytestmark = pytest.mark.gpu

B, S = 2, 16


def _diffusion(model=None, fn=None):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    d = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS)
    if model is not None:
        d.set_denoise_fn(model.forward, model.forward_with_cond_scale)
    else:
        d.set_denoise_fn(None, fn)
    return d


def _skw(steps, method="dpmsolver", **kw):
    # dynamic_input/misc.py:128-141
    return dict(dict(sampling_method=method, vis=None, num_timesteps=steps, ddim_eta=0.0, log_num_per_prog=10,
                     clip_denoised=True, dtp=1, temperature=1.0, noise_dropout=0, random_sample_condition=False,
                     return_inter_dict=True, disable_tqdm=True), **kw)


def _direct(d, steps, **kw):
    """sampling kwargs of a direct ``sampler.sample`` call: what p_sample_loop adds"""
    return _skw(steps, alphas_cumprod=d.sampler.alphas_cumprod, **kw)


def _dkw():
    from sgdm_amd.synth import synth_batch
    return dict(cond=synth_batch("label", B, S, 10, seed=23)["cond"].cuda(), layout=None, cond_scale=2.0)


def _coef64(a, ts, order, lof):
    """float64 (s1ma, rsa, A, B, cc, cp) per row from the formulas (lam(v) = log(v / (1 - v)) / 2), scalar by scalar"""
    lam = lambda v: 0.5 * np.log(v / (1.0 - v))
    n = len(ts)
    rows, h_prev = [None] * n, None
    for k, i in enumerate(reversed(range(n))):
        at, ap = a[ts[i]], (a[ts[i - 1]] if i > 0 else a[0])
        A = np.sqrt((1 - ap) / (1 - at))
        h = lam(ap) - lam(at)
        first = k == 0 or order == 1 or (lof and i == 0)
        r = None if first else h_prev / h
        rows[i] = (np.sqrt(1 - at), 1 / np.sqrt(at), A, np.sqrt(ap) - A * np.sqrt(at), 1.0 if first else 1 + 1 / (2 * r),
                   0.0 if first else -1 / (2 * r))
        h_prev = h
    return np.array(rows, dtype=np.float64)


def _restate(x_T, eps, coef, clip):
    """the update in the kernel's documented order with the dtype of ``coef``'s rows: returns (inputs per call, final).
    fp32: every op is one correctly rounded IEEE add or multiply, as in the un-contracted kernel"""
    x, hist, ins = x_T.to(coef.dtype), None, []
    for k, i in enumerate(reversed(range(coef.shape[0]))):
        ins.append(x)
        s1ma, rsa, A, Bc, cc, cp = coef[i, :6]
        x0 = (x - s1ma * eps[k].to(coef.dtype)) * rsa
        if clip:
            x0 = x0.clamp(-1, 1)
        D = cc * x0
        if float(cp) != 0.0:
            D = D + cp * hist
        hist = x0
        x = A * x + Bc * D
    return ins, x


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("n", [10, 13])
def test_teacher_forced_update_is_bit_exact(n, clip, order):
    """a plain-Python denoiser (generic path, cfg_mode 0) returns seeded recorded tensors: every UNet input and the final
    image equal, max abs diff 0, the sampler's own table applied with torch fp32 CPU ops in the kernel's order; against
    the float64 restatement from the formulas the rel-L2 stays below 1e-5 (fp32 restated sits 2-4e-7 from float64 over
    10-100 steps; 1e-5 is ten times inside the project's 1e-4 parity contract)"""
    g = torch.Generator().manual_seed(1000 + n)
    x_T = torch.randn(B, 3, S, S, generator=g)
    seen = []
    d = _diffusion(fn=lambda x, t, **_: fn(x, t))
    sk = _direct(d, n, clip_denoised=clip, dpm_order=order)
    s = d.sampler_list["dpmsolver"]
    ts, tab = s.plan(sk)
    eps = torch.randn(len(ts), B, 3, S, S, generator=g)
    visit = list(reversed([int(v) for v in ts]))

    def fn(x, t):
        k = len(seen)
        assert torch.equal(t.cpu(), torch.full((B,), visit[k], dtype=torch.long)), (k, t)
        seen.append(x.detach().cpu().clone())
        return eps[k].cuda()

    final, inter = s.sample(shape=(B, 3, S, S), sampling_kwargs=sk, denoise_sample_fn=d.denoise_sample_fn,
                            denoise_sample_fn_kwargs={}, x_T=x_T)
    assert len(seen) == len(ts)
    ins32, out32 = _restate(x_T, eps, tab, clip)
    diff_in = max(float((a - ins32[k]).abs().max()) for k, a in enumerate(seen))
    diff_out = float((final.cpu() - out32).abs().max())
    a64 = d.sampler.alphas_cumprod.double().cpu().numpy()
    _, out64 = _restate(x_T, eps, torch.from_numpy(_coef64(a64, ts, order, len(ts) < 15)), clip)
    r = rel_l2(final.cpu(), out64)
    print(f"dpmsolver n={n} clip={clip} order={order} teacher-forced: max abs diff inputs {diff_in}, final {diff_out}; "
          f"rel_l2 vs float64 {r:.3e}")
    assert diff_in == 0.0 and diff_out == 0.0
    assert r < 1e-5
    assert set(inter) == {"x_inter", "pred_x0"}


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("mode,w", [(0, 0.0), (1, 2.0), (2, 1.5)])
def test_kernel_reads_the_doubled_nhwc_eps_in_all_three_cfg_modes(mode, w, inplace):
    """sgd_dpmpp_step directly: one second-order step with a finite history, doubled NHWC eps, bit-equal to torch fp32 (the
    guidance weights are exact in fp32 and 1 - w / 1 + w are formed in fp32, as the kernel does)"""
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    Cc, H = 3, 8
    g = torch.Generator().manual_seed(31 + mode)
    x = torch.randn(B, Cc, H, H, generator=g)
    eps = torch.randn(2 * B, H, H, Cc, generator=g)
    hist = torch.randn(B, Cc, H, H, generator=g).clamp(-1, 1)
    row = torch.tensor([0.8, 1.6, 0.9, 0.07, 1.375, -0.375, 0.0, 0.0], dtype=torch.float32)
    for clip in (0, 1):
        ec, eu, wt, one = eps[:B], eps[B:], torch.tensor(w, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32)
        e = ec if mode == 0 else (one - wt) * eu + wt * ec if mode == 1 else (one + wt) * ec - wt * eu
        e = e.permute(0, 3, 1, 2)
        x0 = (x - row[0] * e) * row[1]
        if clip:
            x0 = x0.clamp(-1, 1)
        want = row[2] * x + row[3] * (row[4] * x0 + row[5] * hist)
        xd, hd, rd, ed = x.cuda().contiguous(), hist.cuda().contiguous(), row.cuda(), eps.cuda().contiguous()
        out = xd if inplace else torch.empty_like(xd)
        L.check(lib.sgd_dpmpp_step(_ptr(xd), _ptr(ed), mode, w, _ptr(rd), _ptr(hd), clip, B, Cc, H * H, _ptr(out),
                                   torch.cuda.current_stream().cuda_stream), "sgd_dpmpp_step")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), (clip, float((out.cpu() - want).abs().max()))
        assert torch.equal(hd.cpu(), x0.contiguous())


def test_first_order_row_leaves_a_nan_history_unread():
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    x, e = torch.randn(B * 3, 1, 8, 8, generator=g), torch.randn(B * 3, 8, 8, 1, generator=g)
    row = torch.tensor([0.8, 1.6, 0.9, 0.07, 1.0, 0.0, 0.0, 0.0], dtype=torch.float32)
    xd, hd, out = x.cuda(), torch.full((B * 3, 1, 8, 8), float("nan"), device="cuda"), torch.empty(B * 3, 1, 8, 8, device="cuda")
    ed, rd = e.cuda(), row.cuda()               # named: a temporary's memory could be handed out again before the launch
    L.check(lib.sgd_dpmpp_step(_ptr(xd), _ptr(ed), 0, 0.0, _ptr(rd), _ptr(hd), 1, B * 3, 1, 64, _ptr(out),
                               torch.cuda.current_stream().cuda_stream), "sgd_dpmpp_step")
    torch.cuda.synchronize()
    x0 = ((x - row[0] * e.reshape(x.shape)) * row[1]).clamp(-1, 1)
    assert torch.isfinite(out).all() and torch.isfinite(hd).all()
    assert torch.equal(out.cpu(), row[2] * x + row[3] * (row[4] * x0)) and torch.equal(hd.cpu(), x0)


def test_entry_point_refuses_bad_arguments():
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    t = torch.zeros(64, device="cuda")
    args = dict(x=_ptr(t), eps=_ptr(t), mode=0, w=0.0, row=_ptr(t), hist=_ptr(t), clip=0, b=1, c=1, hw=8, out=_ptr(t),
                st=torch.cuda.current_stream().cuda_stream)
    call = lambda **k: lib.sgd_dpmpp_step(*dict(args, **k).values())        # (keyword order is the C argument order)
    for bad in (dict(x=None), dict(eps=None), dict(row=None), dict(hist=None), dict(out=None), dict(b=0), dict(c=-1), dict(hw=0),
                dict(mode=3), dict(mode=-1), dict(b=2 ** 31 - 1, c=2), dict(b=2 ** 16, c=2 ** 14, hw=2 ** 30)):
        assert call(**bad) == 1, bad                                         # SGD_ERR_ARG: refused before any launch
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [10, 50])
def test_first_order_on_uniform_times_is_ddim(n):
    """dpm_order=1, 'uniform', no clipping, teacher-forced: A x + B x0 and DDIM's sqrt(ap) x0 + sqrt(1-ap) e (eta = 0) are
    two algebraically equal forms; final images within 1e-5 rel-L2 (the bound of the float64 comparison, same reason)"""
    g = torch.Generator().manual_seed(77 + n)
    x_T = torch.randn(B, 3, S, S, generator=g)
    eps = torch.randn(n, B, 3, S, S, generator=g)
    out = {}
    for method, extra in (("dpmsolver", dict(dpm_order=1, dpm_spacing="uniform")), ("ddim", {})):
        calls = []

        def fn(x, t, **_):
            calls.append(int(t[0]))
            return eps[len(calls) - 1].cuda()

        d = _diffusion(fn=fn)
        final, _ = d.sampler_list[method].sample(shape=(B, 3, S, S), sampling_kwargs=_direct(d, n, method=method, clip_denoised=False, **extra),
                                                 denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs={}, x_T=x_T)
        out[method] = (final.cpu(), calls)
    assert out["dpmsolver"][1] == out["ddim"][1] and len(out["ddim"][1]) == n
    r = rel_l2(out["dpmsolver"][0], out["ddim"][0])
    print(f"dpmsolver order 1 uniform n={n} vs ddim eta=0, teacher-forced: rel_l2 {r:.3e}")
    assert r < 1e-5


def _count_replays(monkeypatch):
    from sgdm_amd import diffusion as Dm
    count = [0]
    orig = Dm._GraphedStep.step

    def step(self, *a, **k):
        count[0] += 1
        return orig(self, *a, **k)
    monkeypatch.setattr(Dm._GraphedStep, "step", step)
    return count


@pytest.mark.parametrize("name", ["uf_label_c32_s16", "ca_stego_c32_s16"])
def test_graph_captured_equals_eager(name, monkeypatch):
    from sgdm_amd.synth import synth_batch
    replays = _count_replays(monkeypatch)
    m, entry = build_model(name, "f16x3")
    d = _diffusion(m)
    kw = entry["ctor"]
    batch = synth_batch(kw["condition_method"], B, S, kw["cond_dim"], entry["layout_dim"], seed=23)
    cond = batch["cond"].cuda() if entry["kind"] == "unet_fast" else batch["cond"].float().cuda()
    dkw = dict(cond=cond, layout=batch["layout"].cuda() if "layout" in batch else None, cond_scale=2.0)
    s = d.sampler_list["dpmsolver"]
    n = len(s.plan(_direct(d, 10))[0])
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(8))
    x_T2 = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(9))
    out = {}
    for graph in (False, True):
        before = replays[0]
        torch.manual_seed(1234)
        final, _ = s.sample(shape=(B, 3, S, S), sampling_kwargs=_direct(d, 10, hip_graph=graph),
                            denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs=dict(dkw), x_T=x_T)
        torch.manual_seed(1234)
        samples, _ = d.p_sample_loop("dpmsolver", (B, 3, S, S), _skw(10, hip_graph=graph), denoise_sample_fn_kwargs=dict(dkw),
                                     condition_kwargs={}, x_T=x_T)
        assert replays[0] - before == (2 * n if graph else 0)
        # a second trajectory (on the cached graph when captured): the first one's history must not leak into it
        torch.manual_seed(4321)
        final2, _ = s.sample(shape=(B, 3, S, S), sampling_kwargs=_direct(d, 10, hip_graph=graph),
                             denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs=dict(dkw), x_T=x_T2)
        out[graph] = (final.cpu(), samples.cpu(), final2.cpu())
    assert replays[0] == 3 * n
    assert all(torch.isfinite(t.float()).all() for t in out[True])
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)
    assert not torch.equal(out[True][0], out[True][2])


@pytest.mark.parametrize("graph", [True, False])
def test_rng_consumption_is_one_mask_draw_per_evaluation(graph):
    """deterministic sampler: per evaluation only the UNet's cond-drop mask is drawn (uniform_ over 2B), no z"""
    m, _ = build_model("uf_label_c32_s16", "f16x3")
    d = _diffusion(m)
    n = len(d.sampler_list["dpmsolver"].plan(_direct(d, 10))[0])
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(9))
    run = lambda: d.p_sample_loop("dpmsolver", (B, 3, S, S), _skw(10, hip_graph=graph), denoise_sample_fn_kwargs=_dkw(),
                                  condition_kwargs={}, x_T=x_T)
    run()                                       # engine, packed weights and the captured step built outside the count
    torch.manual_seed(77)
    run()
    got = torch.cuda.get_rng_state()
    torch.manual_seed(77)
    for _ in range(n):
        torch.empty(2 * B, device="cuda").uniform_()
    assert torch.equal(got, torch.cuda.get_rng_state())


@pytest.mark.parametrize("graph", [True, False])
def test_ignored_sampling_kwargs_x_T_and_return_value(graph):
    from sgdm_amd.diffusion import to_uint8
    m, _ = build_model("uf_label_c32_s16", "f16x3")
    d = _diffusion(m)
    x_T = torch.randn(B, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    keep = x_T.clone()

    class Vis:
        interp = True
        chainvis = True

    outs = []
    for extra in ({}, dict(ddim_eta=1.0, temperature=0.5, noise_dropout=0.1, vis=Vis())):
        samples, inter = d.p_sample_loop("dpmsolver", (B, 3, S, S), _skw(10, hip_graph=graph, dpm_spacing="uniform", **extra),
                                         denoise_sample_fn_kwargs=_dkw(), condition_kwargs={}, x_T=x_T)
        outs.append((samples.cpu(), inter))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(x_T, keep)
    # shapes, dtypes and devices of the PLMS loop's snapshots at the same number of schedule rows
    _, ref = d.p_sample_loop("plms", (B, 3, S, S), _skw(10, method="plms"), denoise_sample_fn_kwargs=_dkw(), condition_kwargs={},
                             x_T=x_T)
    samples, inter = outs[0]
    assert set(inter) == set(ref) == {"x_inter", "pred_x0"}
    for k in inter:
        assert (inter[k].shape, inter[k].dtype, inter[k].device) == (ref[k].shape, ref[k].dtype, ref[k].device), k
    assert inter["pred_x0"].shape[0] == 9 and inter["pred_x0"].dtype == torch.uint8 and inter["x_inter"].dtype == torch.float32
    # the last snapshot row is schedule row 0: the final image
    assert torch.equal(to_uint8(inter["x_inter"][-1]).cpu(), samples)
    with pytest.raises(ValueError):
        d.p_sample_loop("dpmsolver", (B, 3, S, S), _skw(10, hip_graph=graph, dtp=0.9), denoise_sample_fn_kwargs=_dkw(),
                        condition_kwargs={}, x_T=x_T)


def test_c2_dpmsolver20_captured_vs_torch_loop():
    """C2 shapes (unet_fast ch128, 64x64, bs 40 -> UNet batch 80, f16x3, w=2), 20 steps on the captured step, against the
    method restated in torch (coefficients from the formulas in float64) over the same HIP UNet's forward_with_cond_scale
    from the same x_T; the bounds of test_c2_pndm50_captured_vs_torch_loop"""
    import bench
    from sgdm_amd.diffusion import to_uint8
    wl = bench.WORKLOADS["c2"]
    m, _, data = bench.build_model(wl, "cuda", "f16x3")
    Bc, Sc = wl["batch"], wl["image"]
    d = _diffusion(m)
    dkw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=2.0)
    x_T = torch.randn(Bc, 3, Sc, Sc, generator=torch.Generator().manual_seed(50)).cuda()
    s = d.sampler_list["dpmsolver"]
    sk = _direct(d, 20)
    final, _ = s.sample(shape=(Bc, 3, Sc, Sc), sampling_kwargs=sk, denoise_sample_fn=d.denoise_sample_fn,
                        denoise_sample_fn_kwargs=dict(dkw), x_T=x_T)
    for eng in m._engines.values():
        eng.check_health()
    assert torch.isfinite(final).all()
    ts = s.plan(sk)[0]
    assert len(ts) == 20
    coef = _coef64(d.sampler.alphas_cumprod.double().cpu().numpy(), ts, 2, False)
    with torch.no_grad():
        x, hist = x_T.clone(), None
        for i in reversed(range(len(ts))):
            e = m.forward_with_cond_scale(x, torch.full((Bc,), int(ts[i]), device="cuda", dtype=torch.long), **dkw)
            s1ma, rsa, A, Bq, cc, cp = (float(v) for v in coef[i])
            x0 = ((x - s1ma * e) * rsa).clamp(-1, 1)
            D = x0 if cp == 0.0 else cc * x0 + cp * hist
            x, hist = A * x + Bq * D, x0
    r = rel_l2(final.cpu(), x.cpu())
    du8 = (to_uint8(final).int() - to_uint8(x).int()).abs()
    print(f"C2 dpmsolver-20 captured vs torch loop: rel_l2 {r:.3e}, u8 max diff {int(du8.max())}")
    assert r < 1e-4
    assert du8.max() <= 1
