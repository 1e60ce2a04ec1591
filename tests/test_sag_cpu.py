"""Self-attention guidance (Hong et al. 2023; sampling kwargs sag_scale / sag_layer / sag_threshold / sag_blur_sigma) where it
needs no GPU: the option parsing (sgdm_amd/sampling_plan.py: sag_options -- every refusal is raised before the library is
loaded), the plan's new field and its part of the captured-step key, the binding of the two new entries (include/sgdm_hip.h:
sgd_attention_colmass, sgd_sag_degrade) and the torch restatements the GPU tests compare the kernels with (sgdm_amd/sag.py),
each against an independent formulation: the blur against F.pad(mode='reflect') + conv2d, the attention mass against the
softmax of the oracle's ``attention_block``.  The reference project has no such guidance; oracle/ is not touched."""
import dataclasses
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import PKG, ROOT, cfg_from_index
from test_pag_cpu import INDEX, _oracle_case, _plan_model

DKW = dict(cond_scale=2.0)
T = 1000
MID = "middle_block.1"


def _sk(**kw):
    return dict(dict(num_timesteps=10, clip_denoised=True, temperature=1.0, ddim_eta=1.0, log_num_per_prog=10), **kw)


# ------------------------------------------------------------------------------------------ the exposed oracle (shared)

def exposed_attention(U, prefix, store):
    """``oracle.unet_ref.attention_block`` unchanged, but for layer ``prefix`` its softmax map is re-formed from the same
    q and k and left in ``store`` as ``probs`` [b, heads, T queries, T keys], next to ``q`` / ``k`` [b, T, heads, d]"""
    orig = U.attention_block

    def attention_block(sd, p, x, heads, new_order=False):
        if p == prefix:
            b, c, hh, ww = x.shape
            qkv = F.conv1d(U._gn(sd, p + ".norm", x.reshape(b, c, -1)), sd[p + ".qkv.weight"], sd[p + ".qkv.bias"])
            length, ch = qkv.shape[-1], c // heads
            if new_order:
                q, k, _ = (t.reshape(b * heads, ch, length) for t in qkv.chunk(3, dim=1))
            else:
                q, k, _ = qkv.reshape(b * heads, ch * 3, length).split(ch, dim=1)
            scale = 1 / math.sqrt(math.sqrt(ch))
            w = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, k * scale).float(), dim=-1)
            store.update(probs=w.reshape(b, heads, length, length), hw=(hh, ww),
                         q=q.reshape(b, heads, ch, length).permute(0, 3, 1, 2), k=k.reshape(b, heads, ch, length).permute(0, 3, 1, 2))
        return orig(sd, p, x, heads, new_order)
    return attention_block


def oracle_mass(monkeypatch, cfg, sd, x, t, cond, prefix=MID):
    """(the oracle's conditional evaluation [B, C, H, W], the attention mass of ``prefix`` [B, T] = probs.mean(heads)
    .sum(queries), the layer's map size)"""
    from oracle import unet_ref as U
    store = {}
    with monkeypatch.context() as mp:
        mp.setattr(U, "attention_block", exposed_attention(U, prefix, store))
        with torch.no_grad():
            out = U.unet_forward(cfg, sd, x, t, cond, None, torch.zeros(x.shape[0], dtype=torch.bool))
    return out, store["probs"].mean(1).sum(1), store["hw"]


# ------------------------------------------------------------------------------------------------------------- options

def test_defaults_and_off():
    from sgdm_amd.sampling_plan import DEFAULTS, resolve_plan, sag_options
    m = _plan_model()
    for sk in (None, {}, dict(sag_scale=0), dict(sag_scale=0.0), dict(cfg_rescale=0.5), dict(pag_scale=1.0)):
        assert sag_options(sk, True, m) is None
    assert sag_options({}, False, None) is None                                 # off: nothing asked of the step
    assert sag_options(dict(sag_scale=0.75), True, m) == (0.75, MID, 1.0, 1.0)
    assert MID in m.attention_prefixes()
    other = [p for p in m.attention_prefixes() if p != MID][0]
    got = sag_options(dict(sag_scale=2, sag_layer=other, sag_threshold=0.5, sag_blur_sigma=2), True, m, (2, 3, 5, 5))
    assert got == (2.0, other, 0.5, 2.0) and all(isinstance(v, float) for v in (got[0], got[2], got[3]))
    assert sag_options(dict(sag_scale=3.0, cond_scale=7.0), True, m)[0] == 3.0  # cond_scale is not read
    assert all(DEFAULTS[k] is None for k in ("sag_layer", "sag_threshold", "sag_blur_sigma")) and DEFAULTS["sag_scale"] == 0
    # at sag_scale = 0 nothing of the plan differs from the plain one
    for opt in ({}, dict(cfg_rescale=0.5), dict(parameterization="v", v_form="data")):
        plain = resolve_plan(_sk(**opt), "ddim", m, DKW, T=T)
        off = resolve_plan(_sk(sag_scale=0, **opt), "ddim", m, DKW, T=T, shape=(2, 3, 16, 16))
        assert off == plain and off.sag is None and off.capture_key() == plain.capture_key()
    on = resolve_plan(_sk(sag_scale=0.75), "ddim", m, {}, T=T)
    assert on.sag == (0.75, MID, 1.0, 1.0) and (on.mode, on.weight, on.fused) == (2, 0.75, True) and on.layers is None


BAD = [dict(sag_scale=-0.1), dict(sag_scale="1.5"), dict(sag_scale=True), dict(sag_scale=False), dict(sag_scale=None),
       dict(sag_scale=float("nan")), dict(sag_scale=float("inf")), dict(sag_scale=[1.0]),
       dict(sag_layer=MID), dict(sag_threshold=1.0), dict(sag_blur_sigma=1.0), dict(sag_scale=0, sag_layer=MID),
       dict(sag_scale=0.0, sag_threshold=0.5), dict(sag_scale=0, sag_blur_sigma=2.0),
       dict(sag_scale=1.0, pag_scale=1.0), dict(sag_scale=1.0, cfg_distilled=True), dict(sag_scale=1.0, lv_native=True),
       dict(sag_scale=1.0, sag_layer="mid"), dict(sag_scale=1.0, sag_layer="middle_block.0"), dict(sag_scale=1.0, sag_layer=[MID]),
       dict(sag_scale=1.0, sag_layer=3),
       dict(sag_scale=1.0, sag_threshold=0), dict(sag_scale=1.0, sag_threshold=-1.0), dict(sag_scale=1.0, sag_threshold=True),
       dict(sag_scale=1.0, sag_threshold=float("inf")), dict(sag_scale=1.0, sag_threshold=float("nan")),
       dict(sag_scale=1.0, sag_threshold="1"),
       dict(sag_scale=1.0, sag_blur_sigma=0), dict(sag_scale=1.0, sag_blur_sigma=-2.0), dict(sag_scale=1.0, sag_blur_sigma=False),
       dict(sag_scale=1.0, sag_blur_sigma=float("inf")), dict(sag_scale=1.0, sag_blur_sigma=float("nan"))]


@pytest.mark.parametrize("sk", BAD, ids=lambda sk: ",".join(f"{k}={v!r}" for k, v in sk.items()))
def test_refusals_of_the_option_function_and_of_the_resolver(sk, monkeypatch):
    from sgdm_amd import _lib as L
    from sgdm_amd.sampling_plan import resolve_plan, sag_options
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    m = _plan_model()
    with pytest.raises(ValueError):
        sag_options(sk, True, m)
    with pytest.raises(ValueError):
        resolve_plan(_sk(**sk), "ddim", m, DKW, T=T)


def test_refusals_that_depend_on_the_step_the_model_and_the_image(monkeypatch):
    from sgdm_amd import _lib as L
    from sgdm_amd import diffusion as Dm
    from sgdm_amd.sampling_plan import resolve_plan, sag_options
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    m = _plan_model()
    on = dict(sag_scale=1.0)
    with pytest.raises(ValueError):
        sag_options(on, False, m)                                               # not the fused step
    with pytest.raises(ValueError):
        sag_options(on, True, None)                                             # no drop-in UNet behind the step
    for name in ("ca_stego_c32_s16", "uf_st_label_c32_s16"):                    # Attention_LR / SpatialTransformer
        with pytest.raises(ValueError):
            sag_options(on, True, _plan_model(name))
        with pytest.raises(ValueError):
            resolve_plan(_sk(**on), "ddim", _plan_model(name), DKW, T=T)
    for shape in ((1, 3, 4, 16), (1, 3, 16, 4), (1, 3, 1, 1)):                  # an image side below 5
        with pytest.raises(ValueError, match="at least 5"):
            sag_options(on, True, m, shape)
        with pytest.raises(ValueError, match="at least 5"):
            resolve_plan(_sk(**on), "dpmsolver", m, DKW, T=T, shape=shape)
    assert sag_options(on, True, m, (1, 3, 5, 5)) is not None
    # the learned-variance 'native' update (the other samplers of such a model run on the C-row head)
    with pytest.raises(ValueError, match="learned-variance"):
        resolve_plan(_sk(num_timesteps=T, **on), "native", m, DKW, T=T, lv=True)
    assert resolve_plan(_sk(**on), "ddim", m, DKW, T=T, lv=False).sag
    # an eps-form trajectory that visits alphas_cumprod == 0 stays refused
    import numpy as np
    with pytest.raises(ValueError, match="alphas_cumprod is 0"):
        resolve_plan(_sk(**on), "ddim", m, DKW, T=T, ac_visited=np.asarray([0.5, 0.0]))
    # a generic denoise_sample_fn, p0 and a tensor cond_scale are not the fused step; the library is never asked for
    from sgdm_amd.unet import UNetModel
    from test_hip_unet import AttrDict
    real = UNetModel(condition=AttrDict(scale_type="imagen"), **INDEX["uf_label_c32_s16"]["ctor"])
    fused = real.forward_with_cond_scale
    cases = [(lambda x, t, **kw: x, dict(cond_scale=2.0), on),
             (fused, dict(cond_scale=2.0, p0=torch.zeros(2)), on),
             (fused, dict(cond_scale=torch.ones(2, 1, 1, 1)), on),
             (fused, dict(cond_scale=2.0), dict(on, cfg_distilled=True)),
             (fused, dict(cond_scale=2.0), dict(on, pag_scale=1.0)),
             (fused, dict(cond_scale=2.0), dict(sag_scale=-1.0)),
             (fused, dict(cond_scale=2.0), dict(sag_layer=MID)),
             (fused, dict(cond_scale=2.0), dict(on, sag_layer="input_blocks.0.0"))]
    for fn, kw, sk in cases:
        with pytest.raises(ValueError):
            Dm._StepRunner(fn, kw, sk, "cpu")
    with pytest.raises(AssertionError, match="library loaded"):                 # accepted: goes on to load the library
        Dm._StepRunner(fused, dict(cond_scale=2.0), on, "cpu")


def test_the_samplers_refuse_through_the_plan_before_the_load(monkeypatch):
    import bench
    from sgdm_amd import _lib as L
    from sgdm_amd import diffusion as Dm
    from sgdm_amd.unet import UNetModel
    from test_hip_unet import AttrDict
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    d = Dm.LatentDiffusion(device="cpu", **bench.MODEL_PARAMS)
    m = UNetModel(condition=AttrDict(scale_type="imagen"), **INDEX["uf_label_c32_s16"]["ctor"])
    ac = d.sampler.alphas_cumprod
    for method in ("ddim", "plms", "pndm", "dpmsolver"):
        for opt, shape in ((dict(sag_scale=1.0), (1, 3, 4, 4)), (dict(sag_scale=1.0, sag_layer="nowhere"), (1, 3, 16, 16))):
            with pytest.raises(ValueError, match="sag_"):
                d.sampler_list[method].sample(shape=shape, sampling_kwargs=_sk(alphas_cumprod=ac, **opt),
                                              denoise_sample_fn=m.forward_with_cond_scale, denoise_sample_fn_kwargs=dict(DKW),
                                              x_T=torch.zeros(shape))
    with pytest.raises(ValueError, match="sag_"):
        d.sampler.sample((1, 3, 4, 4), sampling_kwargs=_sk(num_timesteps=T, sag_scale=1.0),
                         denoise_sample_fn=m.forward_with_cond_scale, denoise_sample_fn_kwargs=dict(DKW))


# ----------------------------------------------------------------------------------------------------- the capture key

SHARE = [
    ((dict(sag_scale=1.5, cfg_rescale=0.7), DKW), (dict(sag_scale=3.0, cfg_rescale=0.7), DKW)),        # scheduled: device data
    ((dict(sag_scale=1.5, cfg_interval=(200, 800)), DKW), (dict(sag_scale=0.5, cfg_interval=(1, 2)), DKW)),
    ((dict(sag_scale=1.5), dict(cond_scale=2.0)), (dict(sag_scale=1.5), dict(cond_scale=9.0))),        # cond_scale is not read
    ((dict(sag_scale=1.5), DKW), (dict(sag_scale=1.5, sag_layer=MID, sag_threshold=1.0, sag_blur_sigma=1.0), DKW)),
    ((dict(sag_scale=0), DKW), (dict(), DKW)),
]
SPLIT = [
    ((dict(sag_scale=1.5), DKW), (dict(sag_scale=2.5), DKW)),                   # unscheduled: a static weight
    ((dict(sag_scale=2.0), DKW), (dict(), DKW)),                                # same weight 2.0: the mode and the SAG part differ
    ((dict(sag_scale=2.0), DKW), (dict(pag_scale=2.0), DKW)),
    ((dict(sag_scale=1.5, cfg_rescale=0.7), DKW), (dict(sag_scale=1.5, cfg_rescale=0.7, sag_layer="input_blocks.7.1"), DKW)),
    ((dict(sag_scale=1.5, cfg_rescale=0.7), DKW), (dict(sag_scale=1.5, cfg_rescale=0.7, sag_threshold=0.9), DKW)),
    ((dict(sag_scale=1.5, cfg_rescale=0.7), DKW), (dict(sag_scale=1.5, cfg_rescale=0.7, sag_blur_sigma=2.0), DKW)),
    ((dict(sag_scale=1.5), DKW), (dict(sag_scale=1.5, sag_threshold=0.9), DKW)),
    ((dict(sag_scale=1.5), DKW), (dict(sag_scale=1.5, parameterization="v"), DKW)),
]


def _key(case, model):
    from sgdm_amd.sampling_plan import resolve_plan
    opt, dkw = case
    return resolve_plan(_sk(num_timesteps=T, **opt), "native", model, dkw, T=T).capture_key()


@pytest.mark.parametrize("a,b", SHARE)
def test_trajectories_that_share_a_captured_step(a, b):
    m = _plan_model()
    assert _key(a, m) == _key(b, m)


@pytest.mark.parametrize("a,b", SPLIT)
def test_trajectories_that_do_not(a, b):
    m = _plan_model()
    assert "input_blocks.7.1" in m.attention_prefixes()
    assert _key(a, m) != _key(b, m)


def test_the_plan_stays_frozen():
    from sgdm_amd.sampling_plan import resolve_plan
    plan = resolve_plan(_sk(sag_scale=1.5, cfg_rescale=0.5), "ddim", _plan_model(), DKW, T=T)
    assert "sag" in [f.name for f in dataclasses.fields(plan)] and isinstance(plan.sag, tuple)
    for f in dataclasses.fields(plan):
        with pytest.raises(dataclasses.FrozenInstanceError):
            setattr(plan, f.name, None)
    hash(plan.capture_key())


def test_binding_and_header_declare_both_entries():
    from sgdm_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()
    want = dict(
        sgd_attention_colmass=[L.vp, L.i32, L.i32, L.vp, L.i32, L.i32, L.vp, L.i32, L.i32, L.i32, L.i32, L.i32, L.f32, L.vp, L.vp],
        sgd_sag_degrade=[L.vp, L.vp, L.i32, L.i32, L.vp, L.vp, L.vp, L.vp, L.i32, L.i32, L.f32, L.vp, L.i32, L.i32, L.i32, L.i32,
                         L.vp, L.vp, L.vp])
    for name, args in want.items():
        res, got = L.SIGNATURES[name]
        assert res is L.i32 and got == args
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == len(args), name
    assert int(re.search(r"#define SGD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == 25       # additive entries
    assert os.path.exists(os.path.join(PKG, "csrc", "sag.hip"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("_sgdm_build", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.FILE_FLAGS["sag.hip"] == ["-ffp-contract=off"]


# ---------------------------------------------------------------------------------------------------- the restatements

def test_gaussian_taps():
    from sgdm_amd.sag import gaussian_taps
    for sigma in (0.5, 1.0, 2.0, 7.5):
        g = gaussian_taps(sigma)
        assert g.dtype == torch.float64 and g.shape == (9,)
        assert abs(float(g.sum()) - 1.0) < 1e-15 and torch.equal(g, g.flip(0)) and int(g.argmax()) == 4
        want = torch.exp(-torch.arange(-4, 5, dtype=torch.float64) ** 2 / (2 * sigma ** 2))
        assert torch.allclose(g, want / want.sum(), rtol=1e-14, atol=0)
        assert float(g[4] / g[3]) == pytest.approx(math.exp(1 / (2 * sigma ** 2)), rel=1e-13)


def _degrade_inputs(b, c, h, w, mh, mw, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, h, w, generator=g, dtype=torch.float64)
    out = torch.randn(b, h * w, c, generator=g, dtype=torch.float64)
    ac = torch.linspace(0.9, 0.1, 10, dtype=torch.float64)
    t = torch.randint(0, 10, (b,), generator=g)
    mass = (1.0 + 0.5 * (torch.rand(b, mh * mw, generator=g) - 0.5)).float()
    return x, out, t, ac.sqrt().float(), (1 - ac).sqrt().float(), mass


@pytest.mark.parametrize("par", ["eps", "x0", "v"])
@pytest.mark.parametrize("b,c,h,w,mh,mw", [(1, 1, 5, 5, 1, 1), (2, 3, 16, 16, 4, 4), (2, 4, 12, 20, 3, 5), (1, 2, 9, 7, 9, 7)])
def test_degrade_restatement_agrees_with_pad_and_conv2d(b, c, h, w, mh, mw, par):
    from sgdm_amd.sag import gaussian_taps, sag_degrade_torch
    x, out, t, sa, s1, mass = _degrade_inputs(b, c, h, w, mh, mw)
    taps = gaussian_taps(1.3)
    got = sag_degrade_torch(x, out, par, t, sa, s1, mass, mh, mw, 1.0, taps)
    assert got.dtype == torch.float64
    # independently: the change of variables written out, torch's own reflect padding and a grouped convolution per pass,
    # the mask by interpolate(mode='nearest') where that is the integer rule (exact ratios), else by the rule's index tables
    a, s = sa[t].double().view(b, 1, 1, 1), s1[t].double().view(b, 1, 1, 1)
    o = out.reshape(b, h, w, c).permute(0, 3, 1, 2)
    if par == "eps":
        x0, e = (x - s * o) / a, o
    elif par == "x0":
        x0, e = o, (x - a * o) / s
    else:
        x0, e = a * x - s * o, a * o + s * x
    kw_ = taps.view(1, 1, 1, 9).expand(c, 1, 1, 9)
    hp = F.conv2d(F.pad(x0, (4, 4, 0, 0), mode="reflect"), kw_, groups=c)
    bl = F.conv2d(F.pad(hp, (0, 0, 4, 4), mode="reflect"), kw_.transpose(2, 3), groups=c)
    m2 = mass.view(b, 1, mh, mw)
    if h % mh == 0 and w % mw == 0:
        up = F.interpolate(m2, size=(h, w), mode="nearest")
    else:
        up = torch.stack([torch.stack([m2[:, :, (y * mh) // h, (xx * mw) // w] for xx in range(w)], -1) for y in range(h)], -2)
    M = up > 1.0
    assert mh * mw == 1 or (bool(M.any()) and bool((~M).any()))                 # (a 1x1 map is one value: the extremes below)
    want = a * torch.where(M, bl, x0) + s * e
    diff = float((got - want).abs().max())
    print(f"sag_degrade_torch float64 {par} {(b, c, h, w)}/{(mh, mw)}: max abs diff vs pad + conv2d {diff:.2e}")
    assert diff <= 1e-12
    # the mask's two extremes
    none = sag_degrade_torch(x, out, par, t, sa, s1, mass, mh, mw, 10.0, taps)
    every = sag_degrade_torch(x, out, par, t, sa, s1, mass, mh, mw, 0.1, taps)
    assert float((none - (a * x0 + s * e)).abs().max()) <= 1e-12 and float((every - (a * bl + s * e)).abs().max()) <= 1e-12
    # the dtype of the input: fp32 in, fp32 out, the same thing to fp32 accuracy
    got32 = sag_degrade_torch(x.float(), out.float(), par, t, sa, s1, mass, mh, mw, 1.0, taps.float())
    assert got32.dtype == torch.float32 and float((got32.double() - got).abs().max() / got.abs().max()) < 1e-4


@pytest.mark.parametrize("name", ["uf_label_c32_s16", "uf_heads8_label_c32_s16", "uf_newattn_label_c32_s16"])
def test_mass_restatement_is_the_column_sum_of_the_oracle_softmax(name, monkeypatch):
    from oracle import unet_ref as U
    from sgdm_amd.sag import sag_mass_torch
    cfg, sd, x, t, cond = _oracle_case(name)
    store = {}
    with monkeypatch.context() as mp:
        mp.setattr(U, "attention_block", exposed_attention(U, MID, store))
        with torch.no_grad():
            out = U.unet_forward(cfg, sd, x, t, cond, None, torch.zeros(2, dtype=torch.bool))
    with torch.no_grad():
        assert torch.equal(out, U.unet_forward(cfg, sd, x, t, cond, None, torch.zeros(2, dtype=torch.bool)))   # unchanged
    probs, q, k = store["probs"].double(), store["q"].double(), store["k"].double()
    b, heads, Tq, Tk = probs.shape
    assert Tq == Tk == store["hw"][0] * store["hw"][1] and heads == U.build_plan(cfg)[1][1][2]
    scale = 1 / math.sqrt(q.shape[-1])
    lse = torch.logsumexp(torch.einsum("bihc,bjhc->bhij", q, k) * scale, dim=-1)
    mass = sag_mass_torch(q, k, lse, scale)
    want = probs.mean(1).sum(1)
    err = float(((mass - want).abs() / want.abs()).max())
    print(f"{name}: sag_mass_torch vs probs.mean(heads).sum(queries): max-rel {err:.2e}; mass in [{float(want.min()):.3f}, "
          f"{float(want.max()):.3f}]")
    assert err < 1e-5                                                           # (the oracle's softmax is fp32)
    assert torch.allclose(mass.sum(1), torch.full((b,), float(Tk), dtype=torch.float64), rtol=1e-12)
    assert float(want.max()) > 1.0 > float(want.min())                          # psi = 1 selects some keys and not others
    # the views of a qkv buffer in either channel order
    from sgdm_amd.sag import qk_views
    g = torch.Generator().manual_seed(1)
    n, T_, h_, d_ = 2, 5, 3, 16
    buf = torch.randn(n, T_, 3 * h_ * d_, generator=g)
    ql, kl = qk_views(buf, h_, d_, (3 * d_, d_, 2 * d_))
    leg = buf.reshape(n, T_, h_, 3, d_)
    assert torch.equal(ql, leg[:, :, :, 0]) and torch.equal(kl, leg[:, :, :, 1])
    qn, kn = qk_views(buf, h_, d_, (d_, h_ * d_, 2 * h_ * d_))
    new = buf.reshape(n, T_, 3, h_, d_)
    assert torch.equal(qn, new[:, :, 0]) and torch.equal(kn, new[:, :, 1])
