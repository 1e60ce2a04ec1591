"""The single-product inference modes hip_precision = 'f16' / 'bf16' (SGD_PREC_F16 / SGD_PREC_BF16): operands rounded once to a
16-bit float, one MFMA product per term, fp32 accumulate.  GPU only.

A. Plain launches against EXACT arithmetic on the rounded operands.  A product of two 11-bit (8-bit) significands is exact in
   fp32, so a single-product launch computes, up to fp32 accumulation order, the float64 convolution of the rounded operands:
   both modes are held to the per-launch bound tests/test_hip_kernels.py holds f16x3 to (2e-5, max_rel).  The operands are
   rounded on the host first -- x with .half() / .bfloat16(), w as the pack does (times the scale reported through w_scale_inv,
   rounded, divided) -- because a comparison with the unrounded result would show only the rounding (1e-3) and hide a wrong tap.
B. Fused prologues / the whole UNet against a yardstick from the reference: the CPU oracle under torch.autocast(float16 |
   bfloat16) against the reference's golden eps of the same fixture, computed here, per fixture:
       rel_l2(hip, golden) <= 1.0 * rel_l2(autocast oracle, golden),  max_rel(hip, golden) <= 2.0 * max_rel(autocast oracle, golden)
   (this path rounds in fewer places than autocast -- fp32 storage, norms, epilogues, attention -- so it must sit below; rel-L2
   is a stable statistic and gets no slack, a maximum over a few thousand elements is an extreme value and gets a factor two).
C. CFG and the samplers: captured graph == eager bit for bit, repeatable, finite; teacher-forced guided evaluations under B's rule.
D. Guards: training refuses, use_fp16 still raises, unknown prec is an argument error, packed size is half the x3 sibling's.

Every figure is printed before it is asserted (pytest -s / -rP shows them; profiles/r9_half_modes_parity.txt keeps one run).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import cfg_from_index, load_npz, max_rel, rel_l2
from test_hip_subpixel_up import ROWS
from test_hip_unet import INDEX, build_model, inputs

pytestmark = pytest.mark.gpu

MODES = ["f16", "bf16"]
DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16}
X3 = {"f16": "f16x3", "bf16": "bf16x3"}
LAUNCH_TOL = 2e-5          # tests/test_hip_kernels.py PRECS: the f16x3 per-launch bound, for BOTH modes (products are exact)


def _lib():
    from sgdm_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _rnd(t, mode):
    """round to the mode's 16-bit format (RNE), back in float64"""
    return t.float().to(DTYPE[mode]).double()


def _pack_scaled(w, ks, prec, sub=False):
    """the scaled pack the engine uses; returns (buf, cin_p, cout_p, scale_inv tensor)"""
    L, lib = _lib()
    cout, cin = w.shape[0], w.shape[1]
    nb = lib.sgd_packed_weight_subpixel_bytes(cout, cin, prec) if sub else lib.sgd_packed_weight_bytes(cout, cin, ks, prec)
    buf = torch.zeros(nb // 4, device="cuda")
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")
    sinv = torch.ones(1, device="cuda")
    cp, op = C.c_int32(), C.c_int32()
    if sub:
        L.check(lib.sgd_weight_amax_subpixel(_p(w), cout, cin, _p(amax), _stream()), "amax_subpixel")
        L.check(lib.sgd_pack_weight_subpixel_scaled(_p(w), _p(buf), cout, cin, prec, _p(amax), _p(sinv), C.byref(cp), C.byref(op),
                                                    _stream()), "pack_subpixel")
    else:
        L.check(lib.sgd_weight_amax(_p(w), w.numel(), _p(amax), _stream()), "amax")
        L.check(lib.sgd_pack_weight_scaled(_p(w), _p(buf), cout, cin, ks, prec, 0, _p(amax), _p(sinv), C.byref(cp), C.byref(op),
                                           _stream()), "pack")
    return buf, cp.value, op.value, sinv


def _rounded_weight(w, sinv, mode):
    """w as the pack rounds it: (w * 2^k) rounded, / 2^k (the scale is a power of two: both steps exact but the rounding)"""
    s = 1.0 / float(sinv.item())
    return _rnd(w.cpu() * s, mode) / s


def _subpixel_kernels_pack_order(w):
    """V[a][b] = [cout, cin, 2, 2] of tests/test_hip_subpixel_up.py::subpixel_kernels, summed in fp32 in csrc/pack.hip's order
    (rows outer, columns inner, ascending: (w[y0][x0] + w[y0][x1]) + (w[y1][x0] + w[y1][x1])) -- the rounding that follows
    sees the very fp32 number the pack rounds"""
    w = w.float()
    V = [[None, None], [None, None]]
    for a in (0, 1):
        for b in (0, 1):
            k = torch.zeros(w.shape[0], w.shape[1], 2, 2)
            for r in (0, 1):
                for s in (0, 1):
                    v = None
                    for y in ROWS[a][r]:
                        rs = w[:, :, y, ROWS[b][s][0]]
                        if len(ROWS[b][s]) > 1:
                            rs = rs + w[:, :, y, ROWS[b][s][1]]
                        v = rs if v is None else v + rs
                    k[:, :, r, s] = v
            V[a][b] = k
    return V


def _conv_launch(x, w, bias, mode_name, stride=1, resample=0, tune=0, sub=False):
    """x NCHW cpu, w OIHW cpu; one sgd_igemm launch with the scaled pack.  Returns (y NCHW cpu, scale_inv)"""
    L, lib = _lib()
    prec = L.PREC_BY_NAME[mode_name]
    n, c0, hi, wi = x.shape
    hc, wc = (hi * 2, wi * 2) if resample else (hi, wi)
    ho, wo = (hc // 2, wc // 2) if stride == 2 else (hc, wc)
    cout = w.shape[0]
    wd = w.cuda().contiguous()
    buf, cin_p, cout_p, sinv = _pack_scaled(wd, 3, prec, sub)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    y = torch.full((n, ho, wo, cout), float("nan"), device="cuda")
    bd = bias.cuda()
    a = L.IgemmArgs()
    a.x0, a.c0, a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride = xd.data_ptr(), c0, L.MODE_CONV3, n, hi, wi, ho, wo, stride
    a.resample = (L.RS_UP2_SUBPIXEL if sub else L.RS_UP2) if resample else L.RS_NONE
    a.w, a.cin_p, a.cout_p, a.w_scale_inv, a.bias = buf.data_ptr(), cin_p, cout_p, sinv.data_ptr(), bd.data_ptr()
    a.y, a.cout, a.y_ld, a.prec, a.tune = y.data_ptr(), cout, cout, prec, tune
    if sub:
        assert lib.sgd_igemm_subpixel_ok(C.byref(a)) == 1, "the new modes must take the sub-pixel path"
    L.check(lib.sgd_igemm(C.byref(a), _stream()), "igemm")
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2).contiguous(), sinv


def _flat_launch(x, w, bias, mode_name):
    L, lib = _lib()
    prec = L.PREC_BY_NAME[mode_name]
    m, k = x.shape
    nout = w.shape[0]
    buf, cin_p, cout_p, sinv = _pack_scaled(w.cuda().contiguous(), 1, prec)
    xd, bd = x.cuda(), bias.cuda()
    y = torch.full((m, nout), float("nan"), device="cuda")
    a = L.IgemmArgs()
    a.x0, a.c0, a.mode, a.m, a.stride = xd.data_ptr(), k, L.MODE_FLAT, m, 1
    a.w, a.cin_p, a.cout_p, a.w_scale_inv, a.bias = buf.data_ptr(), cin_p, cout_p, sinv.data_ptr(), bd.data_ptr()
    a.y, a.cout, a.y_ld, a.prec = y.data_ptr(), nout, nout, prec
    L.check(lib.sgd_igemm(C.byref(a), _stream()), "igemm")
    torch.cuda.synchronize()
    return y.cpu(), sinv


# ===================================================================================================================== A
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(2, 32, 16, 16, 128), (3, 64, 8, 8, 64), (1, 3, 16, 16, 32), (2, 96, 4, 4, 3),
                                   (1, 128, 32, 32, 128), (5, 30, 8, 8, 128)])
def test_conv3x3_plain_is_exact_on_rounded_operands(shape, mode):
    """the shapes of test_hip_kernels.py::test_conv3x3_plain (ragged channel counts, the scalar-input path)"""
    n, cin, h, w_, cout = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, cin, h, w_, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g)
    got, sinv = _conv_launch(x, w, b, mode)
    ref = F.conv2d(_rnd(x, mode), _rounded_weight(w, sinv, mode), b.double(), padding=1)
    err = max_rel(got, ref)
    print(f"A conv3x3 {shape} {mode}: max_rel vs exact-on-rounded {err:.3e}; vs unrounded {max_rel(got, F.conv2d(x, w, b, padding=1)):.3e}")
    assert err < LAUNCH_TOL


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,k,nout", [(160, 128, 512), (7, 5000, 256), (300, 96, 96), (1024, 512, 1536)])
def test_linear_flat_is_exact_on_rounded_operands(m, k, nout, mode):
    """1x1 / linear at test_linear_flat's shapes, without its SiLU prologue (a prologue ends the exact statement: see B)"""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(m, k, generator=g)
    w = torch.randn(nout, k, generator=g) / math.sqrt(k)
    b = torch.randn(nout, generator=g)
    got, sinv = _flat_launch(x, w, b, mode)
    ref = F.linear(_rnd(x, mode), _rounded_weight(w, sinv, mode), b.double())
    err = max_rel(got, ref)
    print(f"A flat {(m, k, nout)} {mode}: max_rel vs exact-on-rounded {err:.3e}")
    assert err < LAUNCH_TOL


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["stride2", "up_direct", "up_subpixel"])
def test_conv3x3_resample_is_exact_on_rounded_operands(form, mode):
    L, _ = _lib()
    g = torch.Generator().manual_seed(3)
    # stride 2 at test_conv3x3_resample's shape; the upsampling pair at a shape the sub-pixel rule accepts (128-column tiles,
    # more than a quarter of the device in tiles) so that both launch forms see the same problem
    n, c, h = (2, 64, 16) if form == "stride2" else (24, 128, 16)
    x = torch.randn(n, c, h, h, generator=g)
    w = torch.randn(c, c, 3, 3, generator=g) / math.sqrt(c * 9)
    b = torch.randn(c, generator=g)
    xr = _rnd(x, mode)
    if form == "stride2":
        got, sinv = _conv_launch(x, w, b, mode, stride=2)
        ref = F.conv2d(xr, _rounded_weight(w, sinv, mode), b.double(), stride=2, padding=1)
    elif form == "up_direct":
        got, sinv = _conv_launch(x, w, b, mode, resample=1, tune=L.TUNE_NO_SUBPIXEL)
        ref = F.conv2d(F.interpolate(xr, scale_factor=2, mode="nearest"), _rounded_weight(w, sinv, mode), b.double(), padding=1)
    else:
        got, sinv = _conv_launch(x, w, b, mode, resample=1, sub=True)
        # the four summed 2x2 kernels, summed in fp32 in the pack's order, THEN rounded (tests/test_hip_subpixel_up.py)
        V = _subpixel_kernels_pack_order(w)
        ref = torch.empty(n, c, 2 * h, 2 * h, dtype=torch.float64)
        xp = F.pad(xr, (1, 1, 1, 1))
        for a_ in (0, 1):
            for b_ in (0, 1):
                ref[:, :, a_::2, b_::2] = F.conv2d(xp[:, :, a_:a_ + h + 1, b_:b_ + h + 1], _rounded_weight(V[a_][b_], sinv, mode), b.double())
    err = max_rel(got, ref)
    print(f"A {form} {mode}: max_rel vs exact-on-rounded {err:.3e}")
    assert got.shape == ref.shape
    assert err < LAUNCH_TOL


@pytest.mark.parametrize("mode", MODES)
def test_representable_operands_agree_with_the_x3_sibling(mode):
    """inputs and weights that are already representable (all lo halves zero): one product == three, up to fp32 order"""
    g = torch.Generator().manual_seed(8)
    # weights: representable AFTER the pack's power-of-two scale whatever it is (a scale moves only the exponent)
    x = torch.randn(3, 64, 16, 16, generator=g).to(DTYPE[mode]).float()
    w = (torch.randn(128, 64, 3, 3, generator=g) / math.sqrt(64 * 9)).to(DTYPE[mode]).float()
    b = torch.randn(128, generator=g)
    one, _ = _conv_launch(x, w, b, mode)
    three, _ = _conv_launch(x, w, b, X3[mode])
    xf = torch.randn(300, 256, generator=g).to(DTYPE[mode]).float()
    wf = (torch.randn(384, 256, generator=g) / 16).to(DTYPE[mode]).float()
    bf = torch.randn(384, generator=g)
    onef, _ = _flat_launch(xf, wf, bf, mode)
    threef, _ = _flat_launch(xf, wf, bf, X3[mode])
    e1, e2 = max_rel(one, three), max_rel(onef, threef)
    print(f"A representable operands {mode} vs {X3[mode]}: conv {e1:.3e}, flat {e2:.3e}")
    assert e1 < LAUNCH_TOL and e2 < LAUNCH_TOL


# ===================================================================================================================== B
_YARD = {}


def _autocast_oracle(name, v, mode, tag):
    """stock PyTorch half inference of the reference network: the CPU oracle (pinned bit for bit to the reference) under autocast
    (kept per (fixture, mode, tag): the CFG test reads the keep / drop evaluations of the forward test again)"""
    key = (name, mode, tag)
    if key not in _YARD:
        _YARD[key] = _autocast_oracle_eval(INDEX[name], v, mode, tag)
    return _YARD[key]


def _autocast_oracle_eval(entry, v, mode, tag):
    from oracle import unet_ref as U
    from sgdm_amd.synth import weights_from_seed
    cfg, sd = cfg_from_index(entry), weights_from_seed(entry["manifest"], entry["seed"])
    x, t = torch.from_numpy(v["x"]), torch.from_numpy(v["t"])
    B = x.shape[0]
    cond = torch.from_numpy(v["cond"]) if "cond" in v else None
    if entry["kind"] == "unetca_fast" and cond is not None:
        cond = cond.float()
    layout = torch.from_numpy(v["layout"]).float() if "layout" in v else None
    mask = {"keep": torch.zeros(B, dtype=torch.bool), "drop": torch.ones(B, dtype=torch.bool),
            "mixed": torch.tensor([False, True][:B])}[tag]
    with torch.no_grad(), torch.autocast("cpu", dtype=DTYPE[mode]):
        return U.unet_forward(cfg, sd, x, t, cond, layout, mask).float()


def _yardstick_check(label, got, golden, yard, mode):
    """B's two inequalities; prints the ratios first"""
    got, golden, yard = got.float().cpu(), torch.as_tensor(golden).float(), yard.float()
    assert torch.isfinite(got).all(), label
    l2, l2y = rel_l2(got, golden), rel_l2(yard, golden)
    mr, mry = max_rel(got, golden), max_rel(yard, golden)
    print(f"B {label} {mode}: rel_l2 hip {l2:.3e} / yardstick {l2y:.3e} = {l2 / l2y:.3f}   "
          f"max_rel hip {mr:.3e} / yardstick {mry:.3e} = {mr / mry:.3f}")
    assert l2 <= 1.0 * l2y, (label, l2, l2y)
    assert mr <= 2.0 * mry, (label, mr, mry)


S16 = [n for n in sorted(INDEX) if n.endswith("_s16")]
S64 = ["uf_cluster5000_c128_s64", "ca_stego_c128_s64"]                # one 64x64 entry per UNet class


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", S16 + S64)
def test_unet_forward_within_the_autocast_yardstick(name, mode):
    m, entry = build_model(name, mode)
    v, x, t, cond, layout = inputs(name)
    B = x.shape[0]
    if entry["kind"] == "unetca_fast" and cond is not None:
        cond = cond.float()
    with torch.no_grad():
        for tag, p in (("keep", torch.zeros(B)), ("drop", torch.ones(B)), ("mixed", torch.tensor([0.0, 1.0][:B]))):
            eps = m(x, t, cond=cond, layout=layout, cond_drop_prob=p.cuda())[0]
            yard = _autocast_oracle(name, v, mode, tag)
            _yardstick_check(f"{name} {tag}", eps, v[f"eps_{tag}"], yard, mode)
    for eng in m._engines.values():
        eng.check_health()


# ===================================================================================================================== C
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["uf_label_c32_s16", "ca_stego_c32_s16"])
def test_cfg_within_the_autocast_yardstick(name, mode):
    """forward_with_cond_scale, both scale_types, w = 2: golden cfg_* of the fixture; yardstick = the oracle's guided score of its
    autocast keep / drop evaluations"""
    from oracle import unet_ref as U
    v, x, t, cond, layout = inputs(name)
    for st in ("imagen", "cfg"):
        m, entry = build_model(name, mode, st)
        if entry["kind"] == "unetca_fast" and cond is not None:
            cond = cond.float()
        cfg = dict(cfg_from_index(entry))
        with torch.no_grad():
            e = m.forward_with_cond_scale(x, t, cond_scale=2.0, cond=cond, layout=layout)
        cfg["scale_type"] = st
        yard = U.guided_score(cfg, _autocast_oracle(name, v, mode, "drop"), _autocast_oracle(name, v, mode, "keep"), 2.0)
        _yardstick_check(f"{name} cfg_{st}_2.0", e, v[f"cfg_{st}_2.0"], yard, mode)


def _diffusion(model):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    d = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS)
    d.set_denoise_fn(model.forward, model.forward_with_cond_scale)
    return d


def _skw(method, steps, eta=0.0, **extra):
    return dict(dict(sampling_method=method, vis=None, num_timesteps=steps, ddim_eta=eta, log_num_per_prog=10,
                     clip_denoised=True, dtp=1, temperature=1.0, noise_dropout=0, random_sample_condition=False,
                     return_inter_dict=True, disable_tqdm=True), **extra)


def _dkw(entry):
    from sgdm_amd.synth import synth_batch
    kw = entry["ctor"]
    batch = synth_batch(kw["condition_method"], 2, 16, kw["cond_dim"], entry["layout_dim"], seed=23)
    cond = batch["cond"].cuda() if entry["kind"] == "unet_fast" else batch["cond"].float().cuda()
    return dict(cond=cond, layout=batch["layout"].cuda() if "layout" in batch else None, cond_scale=2.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("method", ["native", "ddim", "plms", "pndm"])
@pytest.mark.parametrize("name", ["uf_label_c32_s16", "ca_stego_c32_s16"])
def test_samplers_graph_equals_eager_and_repeat(name, method, mode):
    """the samplers take the engine's precision: captured step == eager launch sequence bit for bit (the property
    test_graph_captured_step_equals_eager pins for the existing modes), two runs identical, outputs finite"""
    m, entry = build_model(name, mode)
    d = _diffusion(m)
    if method == "native":
        skw, extra = _skw("native", 1000), dict(step_indices=list(range(999, 979, -1)))
    else:
        skw, extra = _skw(method, 20, 1.0 if method == "ddim" else 0.0), {}
    runs = []
    for graph in (False, True, True):
        torch.manual_seed(1234)
        samples, inter = d.p_sample_loop(method, (2, 3, 16, 16), dict(skw, hip_graph=graph), denoise_sample_fn_kwargs=_dkw(entry),
                                         condition_kwargs={}, **extra)
        runs.append((samples.cpu(), inter.get("x_inter", inter["pred_x0"]).cpu().float()))     # (pndm logs pred_x0 only)
    assert torch.isfinite(runs[0][1]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])       # eager == graph
    assert torch.equal(runs[1][0], runs[2][0]) and torch.equal(runs[1][1], runs[2][1])       # graph == graph
    for eng in m._engines.values():
        eng.check_health()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["uf_label_c32_s16", "ca_stego_c32_s16"])
def test_teacher_forced_guided_evaluations(name, mode):
    """(x_t, t) at the first, middle and last step of an f32-mode DDIM-20 trajectory; the guided evaluation there in the new mode
    against the f32 mode, yardstick: the autocast oracle against the fp32 oracle at the same (x_t, t).  (The update kernels are
    fp32: a step adds nothing to the evaluation's error.)"""
    from oracle import unet_ref as U
    from sgdm_amd.synth import weights_from_seed
    m32, entry = build_model(name, "f32")
    mh, _ = build_model(name, mode)
    d = _diffusion(m32)
    dkw = _dkw(entry)
    calls, run32 = [], m32._run

    def recording_run(x, t, *a, **k):                       # the eager step evaluates the UNet through model._run(x_t, t, ...)
        calls.append((x.detach().clone(), t.detach().clone()))
        return run32(x, t, *a, **k)

    m32._run = recording_run
    torch.manual_seed(77)
    d.p_sample_loop("ddim", (2, 3, 16, 16), _skw("ddim", 20, 0.0, hip_graph=False), denoise_sample_fn_kwargs=dict(dkw),
                    condition_kwargs={})
    del m32._run
    assert len(calls) >= 20, len(calls)
    cfg, sd = cfg_from_index(entry), weights_from_seed(entry["manifest"], entry["seed"])
    picks = [0, len(calls) // 2, len(calls) - 1]
    for k in picks:
        x_t, t = calls[k][0].float().contiguous(), calls[k][1].reshape(-1)[:2].to(torch.int64).contiguous()
        with torch.no_grad():
            e32 = m32.forward_with_cond_scale(x_t, t, cond_scale=2.0, cond=dkw["cond"], layout=dkw["layout"])
            eh = mh.forward_with_cond_scale(x_t, t, cond_scale=2.0, cond=dkw["cond"], layout=dkw["layout"])
            lay = dkw["layout"].cpu() if dkw["layout"] is not None else None
            o32 = U.forward_with_cond_scale(cfg, sd, x_t.cpu(), t.cpu(), 2.0, dkw["cond"].cpu(), lay)
            with torch.autocast("cpu", dtype=DTYPE[mode]):
                oh = U.forward_with_cond_scale(cfg, sd, x_t.cpu(), t.cpu(), 2.0, dkw["cond"].cpu(), lay).float()
        got, ref, yard, yref = eh.float().cpu(), e32.float().cpu(), oh, o32.float()
        assert torch.isfinite(got).all()
        l2, l2y, mr, mry = rel_l2(got, ref), rel_l2(yard, yref), max_rel(got, ref), max_rel(yard, yref)
        print(f"C teacher-forced {name} step {k} (t={int(t[0])}) {mode}: rel_l2 {l2:.3e} / {l2y:.3e} = {l2 / l2y:.3f}   "
              f"max_rel {mr:.3e} / {mry:.3e} = {mr / mry:.3f}")
        assert l2 <= 1.0 * l2y, (k, l2, l2y)
        assert mr <= 2.0 * mry, (k, mr, mry)


# ===================================================================================================================== D
@pytest.mark.parametrize("mode", MODES)
def test_training_refuses_the_mode_before_any_launch(mode):
    from sgdm_amd.losses import p_losses_hip
    m, entry = build_model("uf_label_c32_s16", mode)
    m.train()
    v, x, t, cond, layout = inputs("uf_label_c32_s16")
    with pytest.raises(ValueError, match=f"'{mode}'.*inference only"):
        m(x, t, cond=cond, cond_drop_prob=0.0)
    assert not m._engines                                   # refused before an engine (workspace, packs) was even built
    d = _diffusion(m)
    with pytest.raises(ValueError, match=f"'{mode}'.*inference only"):
        p_losses_hip(d, x, t, None, cond=cond)
    assert not m._engines


def test_use_fp16_still_raises_and_points_at_the_mode():
    from sgdm_amd.unet import UNetModel
    kw = dict(INDEX["uf_label_c32_s16"]["ctor"], use_fp16=True)
    with pytest.raises(NotImplementedError, match="hip_precision='f16'"):
        UNetModel(condition=dict(scale_type="imagen"), **kw)


def test_unknown_precision_is_an_argument_error_and_packed_sizes_halve():
    L, lib = _lib()
    x = torch.randn(128, 64, device="cuda")
    w = torch.randn(128, 64, device="cuda")
    y = torch.zeros(128, 128, device="cuda")
    buf, cin_p, cout_p, sinv = _pack_scaled(w, 1, L.PREC_F16)
    a = L.IgemmArgs()
    a.x0, a.c0, a.mode, a.m, a.stride = x.data_ptr(), 64, L.MODE_FLAT, 128, 1
    a.w, a.cin_p, a.cout_p, a.y, a.cout, a.y_ld, a.prec = buf.data_ptr(), cin_p, cout_p, y.data_ptr(), 128, 128, 5
    assert lib.sgd_igemm(C.byref(a), _stream()) == 1                       # SGD_ERR_ARG
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0                                     # nothing was launched
    for one, three in ((L.PREC_F16, L.PREC_F16X3), (L.PREC_BF16, L.PREC_BF16X3)):
        for cout, cin, ks in ((256, 128, 3), (96, 40, 1)):
            assert lib.sgd_packed_weight_bytes(cout, cin, ks, one) * 2 == lib.sgd_packed_weight_bytes(cout, cin, ks, three)
        assert lib.sgd_packed_weight_subpixel_bytes(256, 128, one) * 2 == lib.sgd_packed_weight_subpixel_bytes(256, 128, three)


@pytest.mark.parametrize("mode", MODES)
def test_state_dict_roundtrip_and_repack(mode):
    """test_hip_unet.py::test_state_dict_roundtrip_and_repack's scenario in a new mode (the batched re-pack of the half-size units)"""
    from sgdm_amd.synth import weights_from_seed
    m, entry = build_model("uf_label_c32_s16", mode)
    v, x, t, cond, layout = inputs("uf_label_c32_s16")
    with torch.no_grad():
        e1 = m(x, t, cond=cond, cond_drop_prob=0.0)[0]
        m.load_state_dict(weights_from_seed(entry["manifest"], 77))
        e2 = m(x, t, cond=cond, cond_drop_prob=0.0)[0]
        m.load_state_dict(weights_from_seed(entry["manifest"], entry["seed"]))
        e3 = m(x, t, cond=cond, cond_drop_prob=0.0)[0]
    assert rel_l2(e2.cpu(), e1.cpu()) > 1e-2
    assert torch.equal(e1, e3)
