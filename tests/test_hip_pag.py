"""Perturbed-attention guidance on the HIP path (Ahn et al. 2024; sampling kwargs pag_scale / pag_layers / pag_drop_cond).
csrc/pag.hip: sgd_attention_identity; sgdm_amd/unet.py: UNetModelBase._engine(pag=...), UNet._build_attn; sgdm_amd/diffusion.py:
pag_options, _StepRunner, _GraphedStep.  The reference has no such guidance.  Expected values: torch indexing (kernel), the
oracle with ``attention_block`` patched to a = v on rows [B, 2B) (engine; tests/test_pag_cpu.py builds it) and every sampler's
update restated from the engine's two halves guided with ``_guided32(out, 2, s, B)`` -- torch fp32 in the kernels' operation
order, max abs diff 0.  The DDPM / DDIM step kernels are compiled with fp contraction (csrc/misc.hip): their restatement forms
the fused multiply-adds of the generated code (``_fma``: the exact product and sum in float64, rounded once to fp32); every
other kernel is a sequence of rounded fp32 products and sums.  GPU only; every test prints the figures it asserts on (-s).

Measured on the MI355X: kernel bit-equal in all 16 cases; engine, perturbed half vs the patched oracle at most 2.9e-6 max-rel in
f32 (bound 2e-5) and 2.1e-6 in f16x3 (bound 5e-5), conditional half bit-equal to the CFG engine's, the halves 9.8e-2 .. 5.9e-1 apart;
all 13 sampler cases max abs diff 0 and captured == eager; learned-variance native 6.0e-8 rel-L2 (2.8e-3 with the perturbed half's
variance)."""
import numpy as np
import pytest
import torch

from conftest import cfg_from_index, max_rel, rel_l2
from test_hip_unet import TOL, AttrDict, INDEX, build_model
from test_hip_vpred import B, S, SHAPE, _diffusion, _guided32, _sk, _st
from test_pag_cpu import pag_forward

pytestmark = pytest.mark.gpu

PAG_S = 1.5
MID = ("middle_block.1",)
HW = S * S


# ---------------------------------------------------------------------------------------------------------------- kernel

SENT = -7.0


def _identity_case(batch, heads, t, d, layout, pad, seed=0):
    """(qkv [batch + 1, t, 3 * heads * d], v offset, head stride, out [batch + 1, t, heads * d + pad] of sentinels, expected)"""
    inner = heads * d
    g = torch.Generator().manual_seed(1000 * t + d + seed)
    qkv = torch.randn(batch + 1, t, 3 * inner, generator=g)
    if layout == "legacy":                      # channel = head * 3d + {q: 0, k: d, v: 2d}
        hs, vo = 3 * d, 2 * d
        want = qkv[:batch].reshape(batch, t, heads, 3, d)[:, :, :, 2, :].reshape(batch, t, inner)
    else:                                       # new order: q | k | v planes, the heads inside
        hs, vo = d, 2 * inner
        want = qkv[:batch, :, 2 * inner:]
    out = torch.full((batch + 1, t, inner + pad), SENT)
    return qkv.cuda(), vo, hs, out.cuda(), want.contiguous()


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("layout", ["legacy", "new"])
@pytest.mark.parametrize("batch,heads,t,d", [(3, 2, 5, 16), (2, 4, 64, 32), (1, 1, 1, 128), (2, 3, 17, 64)])
def test_identity_kernel_is_bit_equal_to_indexing(batch, heads, t, d, layout, pad):
    from sgdm_amd import _lib as L
    inner = heads * d
    qkv, vo, hs, out, want = _identity_case(batch, heads, t, d, layout, pad)
    keep = qkv.clone()
    rc = L.load().sgd_attention_identity(qkv.data_ptr() + 4 * vo, 3 * inner, hs, batch, heads, t, d, out.data_ptr(), inner + pad, _st())
    torch.cuda.synchronize()
    assert rc == 0
    got = out.cpu()
    diff = float((got[:batch, :, :inner] - want).abs().max())
    print(f"sgd_attention_identity {(batch, heads, t, d)} {layout} out_ld {inner + pad}: max abs diff vs indexing {diff}")
    assert torch.equal(got[:batch, :, :inner], want)
    assert bool((got[:batch, :, inner:] == SENT).all()) and bool((got[batch:] == SENT).all())   # padding columns, rows beyond batch
    assert torch.equal(qkv, keep)


def test_identity_kernel_refuses_bad_arguments():
    from sgdm_amd import _lib as L
    lib = L.load()
    batch, heads, t, d = 2, 2, 5, 32
    inner = heads * d
    qkv, vo, hs, out, want = _identity_case(batch, heads, t, d, "legacy", 0)
    v = qkv.data_ptr() + 4 * vo
    args = dict(v=v, kv_ld=3 * inner, kv_hs=hs, batch=batch, heads=heads, t=t, d=d, out=out.data_ptr(), out_ld=inner, st=_st())
    call = lambda **k: lib.sgd_attention_identity(*dict(args, **k).values())        # (keyword order is the C argument order)
    bad = [dict(d=24), dict(v=v + 4), dict(out=out.data_ptr() + 4), dict(kv_ld=3 * inner + 2),
           dict(kv_hs=hs + 1), dict(out_ld=inner + 2), dict(out_ld=inner - 4), dict(v=None), dict(out=None), dict(batch=0),
           dict(heads=0), dict(t=-1), dict(d=0), dict(d=256)]
    for b in bad:
        assert call(**b) == 1, b                                                    # SGD_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                                # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu()[:batch], want)


# ---------------------------------------------------------------------------------------------------------------- engine

ENGINE_MODELS = ["uf_label_c32_s16", "uf_heads8_label_c32_s16", "uf_newattn_label_c32_s16"]


def _engine_inputs(entry):
    from sgdm_amd.synth import synth_batch
    g = torch.Generator().manual_seed(77)
    x, t = torch.randn(B, 3, S, S, generator=g), torch.tensor([999, 3])
    cond = synth_batch(entry["ctor"]["condition_method"], B, S, entry["ctor"]["cond_dim"], seed=77)["cond"]
    return x, t, cond


_REFS = {}


def _oracle(name, layers):
    """the patched oracle's doubled evaluation, computed once per (model, layer set) and shared by the precisions"""
    if (name, layers) not in _REFS:
        from sgdm_amd.synth import weights_from_seed
        entry = INDEX[name]
        x, t, cond = _engine_inputs(entry)
        sd = weights_from_seed(entry["manifest"], entry["seed"])
        assert all(float(sd[p + ".proj_out.weight"].abs().max()) > 0 for p in layers)       # the attention output is projected
        _REFS[name, layers] = pag_forward(pytest.MonkeyPatch(), cfg_from_index(entry), sd, x, t, cond.float(), None, layers)
    return _REFS[name, layers]


@pytest.mark.parametrize("which", ["mid", "all"])
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("name", ENGINE_MODELS)
def test_engine_halves(name, prec, which):
    m, entry = build_model(name, prec)
    layers = MID if which == "mid" else tuple(sorted(m.attention_prefixes()))
    assert which == "mid" or len(layers) > 1
    x, t, cond = (a.cuda() for a in _engine_inputs(entry))
    mask = torch.zeros(2 * B, dtype=torch.bool, device="cuda")
    with torch.no_grad():
        cfg_eng = m._run(x, t, cond, None, mask, 2 * B)
        e_cfg = cfg_eng.eps_nhwc.clone()
        pag_eng = m._run(x, t, cond, None, mask, 2 * B, None, layers)
        e_pag = pag_eng.eps_nhwc.clone()
    torch.cuda.synchronize()
    assert pag_eng is not cfg_eng
    tags = [op[0] for op in pag_eng.prog.ops]
    assert sorted(tg[:-len(".attn_identity")] for tg in tags if tg.endswith(".attn_identity")) == list(layers)
    assert not [op for op in cfg_eng.prog.ops if op[0].endswith(".attn_identity")]
    # the conditional half: only the attention grid changed, and the cores treat each (sample, head) independently
    d_c = float((e_pag[:B] - e_cfg[:B]).abs().max())
    ref = _oracle(name, layers)
    got = e_pag.permute(0, 3, 1, 2).cpu()
    err_p, err_c = max_rel(got[B:], ref[B:]), max_rel(got[:B], ref[:B])
    apart = float((got[B:] - got[:B]).abs().max() / ref.abs().max())
    print(f"{name} [{prec}] pag {which}: conditional half vs the CFG engine max abs diff {d_c}; vs patched oracle max-rel "
          f"perturbed {err_p:.2e}, conditional {err_c:.2e} (bound {TOL[prec]:.0e}); perturbed vs conditional half {apart:.2e}")
    assert torch.equal(e_pag[:B], e_cfg[:B])
    assert err_p < TOL[prec] and err_c < TOL[prec]
    assert apart > 10 * TOL[prec]                           # without this the comparison above would be vacuous


def test_engine_keys_and_refusals():
    from sgdm_amd import _lib as L
    m, entry = build_model("uf_label_c32_s16", "f16x3")
    prec = L.PREC_BY_NAME["f16x3"]
    x, t, cond = (a.cuda() for a in _engine_inputs(entry))
    mask = torch.zeros(2 * B, dtype=torch.bool, device="cuda")
    allp = tuple(sorted(m.attention_prefixes()))
    with torch.no_grad():
        plain = m._run(x, t, cond, None, mask, 2 * B)
        one = m._run(x, t, cond, None, mask[:B], B)
        mid = m._run(x, t, cond, None, mask, 2 * B, None, MID)
        assert m._run(x, t, cond, None, mask, 2 * B, None, MID) is mid                      # one engine per distinct set
        every = m._run(x, t, cond, None, mask, 2 * B, None, allp)
        assert m._run(x, t, cond, None, mask, 2 * B) is plain
    assert len({id(e) for e in (plain, one, mid, every)}) == 4
    assert set(m._engines) == {(2 * B, S, S, prec), (B, S, S, prec), (2 * B, S, S, prec, ("pag",) + MID),
                               (2 * B, S, S, prec, ("pag",) + allp)}
    assert m._engines[(2 * B, S, S, prec)] is plain and m._engines[(B, S, S, prec)] is one  # the plain keys are what they were
    # the training engine: the plain key at its batch, never a PAG one
    m.train()
    out = m.forward(x, t, cond=cond, layout=None, cond_drop_prob=0.0)[0]
    assert out.requires_grad                                                               # (the autograd-capable path)
    m.eval()
    assert [k for k in m._engines if len(k) > 4] == [(2 * B, S, S, prec, ("pag",) + MID), (2 * B, S, S, prec, ("pag",) + allp)]
    assert (B, S, S, prec) in m._engines
    # refused at engine build, before any launch
    n_before = len(m._engines)
    for bad in (("middle_block.0",), ("middle_block.1", "input_blocks.4.1"), ()):
        with pytest.raises(ValueError):
            m._engine(2 * B, S, S, prec, None, bad)
    with pytest.raises(ValueError):
        m._engine(3, S, S, prec, None, MID)                                                  # an odd UNet batch
    assert len(m._engines) == n_before
    for name in ("ca_stego_c32_s16", "uf_st_label_c32_s16"):                                # Attention_LR; SpatialTransformer
        other, _ = build_model(name, "f32")
        with pytest.raises(ValueError):
            other._engine(2 * B, S, S, L.PREC_F32, None, MID)
        assert not other._engines
        d = _diffusion("eps", other)
        with pytest.raises(ValueError):
            d.sampler_list["ddim"].sample(shape=SHAPE, sampling_kwargs=_sk(d, "ddim", 10, pag_scale=PAG_S), denoise_sample_fn=d.denoise_sample_fn,
                                          denoise_sample_fn_kwargs=dict(cond=None, layout=None, cond_scale=2.0))
        assert not other._engines


# -------------------------------------------------------------------------------------------------------------- samplers

@pytest.fixture(scope="module")
def model():
    return build_model("uf_label_c32_s16", "f16x3")[0]


@pytest.fixture(scope="module")
def cond():
    from sgdm_amd.synth import synth_batch
    return synth_batch("label", B, S, 10, seed=23)["cond"].cuda()


def _x_T(seed):
    return torch.randn(*SHAPE, generator=torch.Generator().manual_seed(seed)).cuda()


def _steps(model):
    return list(model.__dict__.get("_hip_graph_steps", {}).values())


def _pag_keys(model):
    return [k for k in model._engines if len(k) > 4 and isinstance(k[-1], tuple) and k[-1][:1] == ("pag",)]


def _zs(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*SHAPE, generator=g) for _ in range(n)]


def _run(d, method, cond, x_T, graph=True, steps=10, zs=None, w=2.0, **skx):
    """one trajectory; (final, inter) on the host.  'native': the strided chain over ``steps`` times"""
    kw = dict(denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs=dict(cond=cond, layout=None, cond_scale=w),
              x_T=x_T.clone())
    if zs is not None and method in ("native", "ddim"):
        kw["noise_fn"] = lambda i: zs[i]
    if method == "native":
        sk = _sk(d, "native", 1000, native_steps=steps, hip_graph=graph, log_num_per_prog=steps + 1, **skx)
        final, inter = d.sampler.sample(SHAPE, sampling_kwargs=sk, **kw)
    else:
        sk = _sk(d, method, steps, hip_graph=graph, log_num_per_prog=10 * steps, **skx)
        final, inter = d.sampler_list[method].sample(shape=SHAPE, sampling_kwargs=sk, **kw)
    return final.cpu(), {k: v.cpu() for k, v in inter.items()}


def _record(mp):
    """every step (row, image before, image after) and every eager evaluation (row, its input) of the trajectories run under
    ``mp``, captured and eager alike"""
    from sgdm_amd import diffusion as Dm
    rec = dict(steps=[], evals=[])
    g0, e0, ev0 = Dm._GraphedStep.step, Dm._EagerStep.step, Dm._EagerStep.eps

    def gstep(self, i, *a, **k):
        x = self.img.clone()
        g0(self, i, *a, **k)
        rec["steps"].append((int(i), x.cpu(), self.img.clone().cpu()))

    def estep(self, i, *a, **k):
        x = self.img.clone()
        e0(self, i, *a, **k)
        rec["steps"].append((int(i), x.cpu(), self.img.clone().cpu()))

    def eeps(self, i, x=None):
        rec["evals"].append((int(i), (self.img if x is None else x).clone().cpu()))
        return ev0(self, i, x)
    mp.setattr(Dm._GraphedStep, "step", gstep)
    mp.setattr(Dm._EagerStep, "step", estep)
    mp.setattr(Dm._EagerStep, "eps", eeps)
    return rec


def _halves(model, x, t, cond, layers=MID, drop=False):
    """the PAG engine's two halves [2B, hw, C] at the step input ``x`` (host) and time ``t``"""
    td = torch.full((B,), int(t), dtype=torch.long, device="cuda")
    mask = torch.cat((torch.zeros(B, dtype=torch.bool), torch.full((B,), bool(drop)))).cuda()
    with torch.no_grad():
        eng = model._run(x.cuda(), td, cond, None, mask, 2 * B, None, layers)
    return eng.eps_nhwc.reshape(2 * B, HW, -1).clone().cpu()


def _nchw(g):
    return g.permute(0, 2, 1).reshape(B, -1, S, S).contiguous()


def _guided(model, x, t, cond, s=PAG_S, **kw):
    """(1 + s) c - s p of the engine's halves in torch fp32, NCHW"""
    return _nchw(_guided32(_halves(model, x, t, cond, **kw), 2, s, B))


def _fma(a, b, c):
    """fl32(a * b + c): the product of two fp32 numbers is exact in float64, the sum is rounded to 53 bits and then to 24"""
    return (torch.as_tensor(a).double() * torch.as_tensor(b).double() + torch.as_tensor(c).double()).float()


def _sqrt32(v):
    """correctly rounded fp32 square root of a scalar (numpy float32; torch's CPU sqrt is not, see PNDM_Sampler.plan)"""
    return torch.tensor(np.sqrt(np.float32(float(v))), dtype=torch.float32)


def _upd_ddim(x, e, row):
    """csrc/misc.hip: ddim_step_kernel at sigma = 0 as compiled: x0 = fma(-s1m, e, x) / sqrt(a_t), clipped;
    x_out = sqrt(a_prev) * x0 + sqrt(1 - a_prev) * e, two rounded products"""
    s1m, a_t, a_prev, sigma = (row[j] for j in range(4))
    assert float(sigma) == 0.0
    x0 = (_fma(-s1m, e, x) / torch.full_like(x, float(_sqrt32(a_t)))).clamp(-1, 1)
    return _sqrt32(a_prev) * x0 + _sqrt32(torch.tensor(1.0) - a_prev) * e, x0


def _upd_ddpm(x, e, row, z):
    """csrc/misc.hip: ddpm_step_kernel as compiled: x0 = fma(k0, x, -(k1 * e)), clipped; mean = fma(k3, x, k2 * x0);
    x_out = mean + k4 * z"""
    k0, k1, k2, k3, k4 = (row[j] for j in range(5))
    x0 = _fma(k0, x, -(k1 * e)).clamp(-1, 1)
    return _fma(k3, x, k2 * x0) + k4 * z, x0


def _upd_dpm(x, e, row, hist):
    """csrc/dpm.hip"""
    s1ma, rsa, A, Bc, cc, cp = (row[j] for j in range(6))
    x0 = ((x - s1ma * e) * rsa).clamp(-1, 1)
    D = cc * x0
    if float(cp) != 0.0:
        D = D + cp * hist
    return A * x + Bc * D, x0


def _upd_v(x, vg, a, s, row, hist, z):
    """csrc/vstep.hip: the data form of 'v'"""
    kx, k0, ke, kz, kh = (row[j] for j in range(5))
    x0 = (a * x - s * vg).clamp(-1, 1)
    eps = a * vg + s * x
    acc = kx * x + k0 * x0
    if float(ke) != 0.0:
        acc = acc + ke * eps
    if float(kh) != 0.0:
        acc = acc + kh * hist
    if float(kz) != 0.0:
        acc = acc + kz * z
    return acc, x0


def _plan(d, method, sk_extra):
    """(UNet time per table row, table) of the sampler's own schedule, as the trajectory under test builds it"""
    from sgdm_amd.diffusion import native_rows, native_times
    data = sk_extra.get("v_form") == "data"
    if method == "native":
        times = native_times(10, 1000)
        kind = "v_native" if data else "ddpm"
        tab, _ = native_rows(d.sampler.alphas_cumprod.detach().cpu().double().numpy()[times], kind, d.hparams.parameterization,
                             [1.0] * 10)
        return [int(v) for v in times], tab
    s = d.sampler_list[method]
    if method in ("ddim", "plms"):
        s.make_schedule(_sk(d, method, 10))
        return [int(v) for v in s.ddim_timesteps], (s.vstep_table(1.0) if data else s.step_table)
    if method == "pndm":
        return s.plan(10)
    ts, tab = s.plan(_sk(d, method, 10, **sk_extra), "data" if data else "eps")
    return [int(v) for v in ts], tab


def _restate(d, method, par, form, model, cond, rec, times, tab, zs):
    """every recorded step from its own input: the engine's halves there, guided in torch fp32, the sampler's update restated.
    Returns the max abs difference over all steps"""
    sa, s1 = d.sampler.sqrt_alphas_cumprod.cpu(), d.sampler.sqrt_one_minus_alphas_cumprod.cpu()
    n = len(times)

    def eps_of(x, t):
        """the guided output at (x, t) as the update reads it: eps; for 'v' on the eps form sa v_g + s1 x (csrc/vpred.hip)"""
        g = _guided(model, x, t, cond)
        return sa[t] * g + s1[t] * x if par == "v" and form == "eps" else g

    diffs, hist = [], None
    if method == "plms":
        # ddim_plms_sampler.py:394-482: the first step evaluates twice; the history arithmetic is the sampler's own torch
        # expressions, formed on the device like there
        evals, steps = rec["evals"], rec["steps"]
        assert len(evals) == n + 1 and len(steps) == n + 1
        es = [eps_of(x, times[i]) for i, x in evals]
        assert torch.equal(evals[1][1], steps[0][2])                    # the second evaluation: at the plain step's x_prev
        dev = lambda a: a.cuda()
        old, k = [], 0
        for j, (i, x, x_out) in enumerate(steps):
            if j == 0:
                e_use = es[0]
            else:
                e_t = es[0] if j == 1 else es[j]
                if len(old) == 0:
                    e_use = ((dev(e_t) + dev(es[1])) / 2).cpu()
                elif len(old) == 1:
                    e_use = ((3 * dev(e_t) - dev(old[-1])) / 2).cpu()
                elif len(old) == 2:
                    e_use = ((23 * dev(e_t) - 16 * dev(old[-1]) + 5 * dev(old[-2])) / 12).cpu()
                else:
                    e_use = ((55 * dev(e_t) - 59 * dev(old[-1]) + 37 * dev(old[-2]) - 9 * dev(old[-3])) / 24).cpu()
                old = (old + [e_t])[-3:]
            want, _ = _upd_ddim(x, e_use, tab[i])
            diffs.append(float((x_out - want).abs().max()))
        return max(diffs), len(diffs)
    if method == "pndm":
        steps = rec["steps"]
        assert [i for i, _, _ in steps] == list(range(n))
        f = tab[:, :3].contiguous().view(torch.float32)
        K16, K13, K124 = (torch.tensor(v, dtype=torch.float32) for v in (1 / 6, 1 / 3, 1 / 24))
        acc = base = None
        ring = [None, None, None]
        for i, x, x_out in steps:
            e = eps_of(x, times[i])
            dd, c1, c2 = f[i]
            phase, r1, r2, r3 = (int(v) for v in tab[i, 4:8])
            if phase == 0:
                src, acc, base, r = x, K16 * e, x, e
                ring[r1 % 3] = e
            elif phase == 1:
                acc, src, r = acc + K13 * e, base, e
            elif phase == 2:
                src, r = base, acc + K16 * e
            else:
                src = x
                r = K124 * (55.0 * e - 59.0 * ring[r1 % 3] + 37.0 * ring[r2 % 3] - 9.0 * ring[r3 % 3])
                ring[r3 % 3] = e
            want = src + dd * (c1 * src - c2 * r)
            diffs.append(float((x_out - want).abs().max()))
        return max(diffs), len(diffs)
    steps = rec["steps"]
    assert [i for i, _, _ in steps] == list(reversed(range(n)))
    for i, x, x_out in steps:
        t = times[i]
        z = None if zs is None else zs[i if method == "native" else n - i - 1]
        if form == "data":
            g = _guided(model, x, t, cond)
            want, hist = _upd_v(x, g, sa[t], s1[t], tab[i], hist, z)
        elif method == "native":
            want, _ = _upd_ddpm(x, eps_of(x, t), tab[i], z)
        elif method == "ddim":
            want, _ = _upd_ddim(x, eps_of(x, t), tab[i])
        else:
            want, hist = _upd_dpm(x, eps_of(x, t), tab[i], hist)
        diffs.append(float((x_out - want).abs().max()))
    return max(diffs), len(diffs)


CASES = [("native", "eps", "eps"), ("native", "v", "eps"), ("native", "v", "data"),
         ("ddim", "eps", "eps"), ("ddim", "v", "eps"), ("ddim", "v", "data"),
         ("plms", "eps", "eps"), ("plms", "v", "eps"), ("pndm", "eps", "eps"), ("pndm", "v", "eps"),
         ("dpmsolver", "eps", "eps"), ("dpmsolver", "v", "eps"), ("dpmsolver", "v", "data")]


@pytest.mark.parametrize("method,par,form", CASES)
def test_trajectory_captured_equals_eager_and_the_restated_method(method, par, form, model, cond, monkeypatch):
    """10 steps at s = 1.5 on the middle attention: captured == eager bit for bit; teacher-forced, every update == the method
    restated in torch fp32 from the engine's two halves, max abs diff 0.  cond_scale (here 2.0) is not read"""
    d = _diffusion(par, model)
    skx = dict(pag_scale=PAG_S, **(dict(v_form="data") if form == "data" else {}))
    times, tab = _plan(d, method, skx)
    zs = _zs(71, 10) if method in ("native", "ddim") else None
    x_T = _x_T(70)
    model.__dict__.pop("_hip_graph_steps", None)
    out, recs = {}, {}
    for graph in (False, True):
        torch.manual_seed(21)
        with monkeypatch.context() as mp:
            recs[graph] = _record(mp)
            out[graph] = _run(d, method, cond, x_T, graph, zs=zs, **skx)
    captured = len(_steps(model))
    assert captured == (0 if method == "plms" else 1)                   # (plms has no captured step: its eps is the caller's)
    same = torch.equal(out[False][0], out[True][0]) and all(torch.equal(out[False][1][k], out[True][1][k]) for k in out[True][1])
    assert len(recs[False]["steps"]) == len(recs[True]["steps"])
    same = same and all(torch.equal(a[2], b[2]) for a, b in zip(recs[False]["steps"], recs[True]["steps"]))
    diff, count = _restate(d, method, par, form, model, cond, recs[True], times, tab, zs)
    print(f"PAG s {PAG_S} 'mid', {method}/{par}/{form}: captured == eager: {same}; {count} updates vs the restated method, "
          f"teacher-forced: max abs diff {diff}")
    assert torch.isfinite(out[True][0]).all() and same
    assert diff == 0.0
    from sgdm_amd import _lib as L
    assert (2 * B, S, S, L.PREC_BY_NAME["f16x3"], ("pag",) + MID) in model._engines
    # the guidance does something: another weight, and CFG, are other trajectories
    torch.manual_seed(21)
    other = _run(d, method, cond, x_T, True, zs=zs, **dict(skx, pag_scale=0.5))[0]
    torch.manual_seed(21)
    cfg = _run(d, method, cond, x_T, True, zs=zs, **{k: v for k, v in skx.items() if k != "pag_scale"})[0]
    assert not torch.equal(other, out[True][0]) and not torch.equal(cfg, out[True][0])


def test_scale_type_and_cond_scale_are_not_read(cond):
    """mode 2 whatever the model's scale_type; the weight is pag_scale whatever cond_scale"""
    outs = []
    for st, w in (("imagen", 2.0), ("cfg", 7.0)):
        m, _ = build_model("uf_label_c32_s16", "f16x3", st)
        d = _diffusion("eps", m)
        torch.manual_seed(3)
        outs.append(_run(d, "dpmsolver", cond, _x_T(72), True, w=w, pag_scale=PAG_S)[0])
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_sweep_over_pag_scale_is_one_capture_and_leaves_no_residue(model, cond, monkeypatch):
    """the weight of a scheduled step is data (a device float), as for the cond_scale sweep of test_hip_cfg_schedule.py"""
    from sgdm_amd import diffusion as Dm
    d = _diffusion("eps", model)
    x_T = _x_T(73)
    model.__dict__.pop("_hip_graph_steps", None)
    captures = []
    cap0 = Dm._GraphedStep._capture
    monkeypatch.setattr(Dm._GraphedStep, "_capture", staticmethod(lambda *a, **k: (captures.append(1), cap0(*a, **k))[1]))
    torch.manual_seed(11)
    before = _run(d, "ddim", cond, x_T)
    n0 = len(captures)
    sweep = []
    for s in (0.5, 1.5, 3.0):
        torch.manual_seed(11)
        sweep.append(_run(d, "ddim", cond, x_T, pag_scale=s, cfg_rescale=0.7))
    steps = _steps(model)
    print(f"sweep over pag_scale 0.5, 1.5, 3.0 (cfg_rescale 0.7): {len(captures) - n0} capture(s), {len(steps)} cached steps")
    assert len(captures) - n0 == 1 and len(steps) == 2
    assert not torch.equal(sweep[0][0], sweep[1][0]) and not torch.equal(sweep[1][0], sweep[2][0])
    torch.manual_seed(11)
    again = _run(d, "ddim", cond, x_T, pag_scale=0.5, cfg_rescale=0.7)
    torch.manual_seed(11)
    after = _run(d, "ddim", cond, x_T)
    assert len(captures) - n0 == 1 and [id(s) for s in _steps(model)] == [id(s) for s in steps]
    assert torch.equal(again[0], sweep[0][0]) and torch.equal(again[1]["x_inter"], sweep[0][1]["x_inter"])
    assert torch.equal(before[0], after[0]) and torch.equal(before[1]["x_inter"], after[1]["x_inter"])
    # the layer set and pag_drop_cond are part of the key: each is a capture of its own
    torch.manual_seed(11)
    _run(d, "ddim", cond, x_T, pag_scale=0.5, cfg_rescale=0.7, pag_drop_cond=True)
    torch.manual_seed(11)
    _run(d, "ddim", cond, x_T, pag_scale=0.5, cfg_rescale=0.7, pag_layers="all")
    assert len(captures) - n0 == 3 and len(_steps(model)) == 4


def test_interval_that_hits_nothing_is_the_conditional_trajectory(model, cond):
    """eta = 1 (the noise matters), same seed: every evaluation is the conditional one at B, as for a distilled student and
    for CFG under the same interval"""
    d = _diffusion("eps", model)
    x_T = _x_T(74)
    torch.manual_seed(9)
    want = _run(d, "ddim", cond, x_T, cfg_distilled=True, ddim_eta=1.0)
    torch.manual_seed(9)
    want_cfg = _run(d, "ddim", cond, x_T, cfg_interval=(2, 100), ddim_eta=1.0)
    assert torch.equal(want[0], want_cfg[0])
    model.__dict__.pop("_hip_graph_steps", None)
    for graph in (True, False):
        torch.manual_seed(9)
        got = _run(d, "ddim", cond, x_T, graph, pag_scale=PAG_S, cfg_interval=(2, 100), ddim_eta=1.0)
        print(f"PAG, empty interval ({'captured' if graph else 'eager'}) vs the conditional trajectory: max abs diff "
              f"{float((got[0] - want[0]).abs().max())}")
        assert torch.equal(got[0], want[0]) and torch.equal(got[1]["x_inter"], want[1]["x_inter"])
    (step,) = _steps(model)
    assert step.replays == dict(guided=0, cond=10)
    # an interval that hits some evaluations: a third trajectory, captured == eager, guided evaluations through sgd_cfg_guide
    outs = []
    for graph in (True, False):
        torch.manual_seed(9)
        outs.append(_run(d, "ddim", cond, x_T, graph, pag_scale=PAG_S, cfg_interval=(301, 601), cfg_rescale=0.7, ddim_eta=1.0)[0])
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], want[0])
    assert _steps(model)[-1].replays == dict(guided=4, cond=6)


def test_without_the_kwargs_nothing_changes_and_no_pag_engine_is_built(cond, monkeypatch):
    from sgdm_amd import _lib as L
    m, _ = build_model("uf_label_c32_s16", "f16x3")
    d = _diffusion("eps", m)
    x_T = _x_T(75)
    calls = []
    fn = L.load().sgd_attention_identity
    monkeypatch.setattr(L.load(), "sgd_attention_identity", lambda *a: (calls.append(1), fn(*a))[1])
    outs = {}
    for method in ("native", "ddim", "plms", "pndm", "dpmsolver"):
        torch.manual_seed(4)
        outs[method] = _run(d, method, cond, x_T, zs=_zs(76, 10))[0]
        torch.manual_seed(4)
        assert torch.equal(_run(d, method, cond, x_T, zs=_zs(76, 10), pag_scale=0)[0], outs[method])     # 0 is off
    assert not _pag_keys(m) and not calls
    assert all(len(k) == 4 for k in m._engines)
    # the guided score of the untouched step: the model's own forward_with_cond_scale, teacher-forced on dpmsolver's first step
    ts, tab = d.sampler_list["dpmsolver"].plan(_sk(d, "dpmsolver", 10))
    t = torch.full((B,), int(ts[-1]), dtype=torch.long, device="cuda")
    e = m.forward_with_cond_scale(x_T, t, cond_scale=2.0, cond=cond, layout=None).cpu()
    with monkeypatch.context() as mp:
        rec = _record(mp)
        torch.manual_seed(4)
        _run(d, "dpmsolver", cond, x_T)
    want, _ = _upd_dpm(x_T.cpu(), e, tab[len(ts) - 1], None)
    assert rel_l2(rec["steps"][0][2], want) <= 1e-5
    # after PAG runs on the same model the default trajectories are the same bits
    torch.manual_seed(4)
    _run(d, "ddim", cond, x_T, zs=_zs(76, 10), pag_scale=PAG_S)
    assert len(_pag_keys(m)) == 1 and calls
    for method in ("ddim", "dpmsolver"):
        torch.manual_seed(4)
        assert torch.equal(_run(d, method, cond, x_T, zs=_zs(76, 10))[0], outs[method])


@pytest.mark.parametrize("drop", [False, True])
def test_drop_mask_of_the_perturbed_half(drop, model, cond, monkeypatch):
    """pag_drop_cond=False: (0, 0), the perturbed half keeps the condition; True: (0, 1), as for CFG.  Through the mask handed
    to ``_run`` (eager) and the captured step's probabilities; the uniforms are drawn either way"""
    d = _diffusion("eps", model)
    x_T = _x_T(77)
    masks, run0 = [], model._run

    def spy(x, t, c, layout, mask, n, *a, **k):
        masks.append((mask.clone().cpu(), n, a, k))
        return run0(x, t, c, layout, mask, n, *a, **k)
    model.__dict__.pop("_hip_graph_steps", None)
    skx = dict(pag_scale=PAG_S, **(dict(pag_drop_cond=True) if drop else {}))
    outs, rng = [], []
    for graph in (False, True):
        torch.manual_seed(13)
        with monkeypatch.context() as mp:
            mp.setattr(model, "_run", spy)
            outs.append(_run(d, "dpmsolver", cond, x_T, graph, **skx)[0])
        rng.append(torch.cuda.get_rng_state().clone())
    want = torch.tensor([False, False, drop, drop])
    assert len(masks) == 10 and all(torch.equal(mk, want) and n == 2 * B and a == (None, MID) for mk, n, a, _ in masks)
    (step,) = _steps(model)
    assert torch.equal(step.p.cpu(), want.float())
    torch.manual_seed(13)
    _run(d, "dpmsolver", cond, x_T, True)                   # CFG: the doubled evaluation's RNG consumption
    assert torch.equal(outs[0], outs[1]) and torch.equal(rng[0], rng[1]) and torch.equal(rng[0], torch.cuda.get_rng_state())
    # teacher-forced on the first step: the halves under that mask
    ts, tab = d.sampler_list["dpmsolver"].plan(_sk(d, "dpmsolver", 10))
    with monkeypatch.context() as mp:
        rec = _record(mp)
        torch.manual_seed(13)
        _run(d, "dpmsolver", cond, x_T, True, **skx)
    i, x, x_out = rec["steps"][0]
    h = _halves(model, x, ts[i], cond, drop=drop)
    assert torch.equal(h[:B], h[B:]) is False
    want_x, _ = _upd_dpm(x, _nchw(_guided32(h, 2, PAG_S, B)), tab[i], None)
    assert float((x_out - want_x).abs().max()) == 0.0
    if drop:                                                # the other mask is another perturbed half
        assert not torch.equal(h[B:], _halves(model, x, ts[i], cond, drop=False)[B:])


def test_dynamic_thresholding_runs_under_pag(model, cond):
    """dtp < 1 takes the eager step (sgd_x0_quantile reads the doubled output with mode 2 and w = s) whatever hip_graph says:
    the same bits both ways, and another trajectory than without thresholding.  (native_steps: the 'native' cases above)"""
    d = _diffusion("eps", model)
    x_T = _x_T(78)
    outs = []
    for graph in (True, False):
        torch.manual_seed(15)
        outs.append(_run(d, "ddim", cond, x_T, graph, zs=_zs(79, 10), pag_scale=PAG_S, dtp=0.9)[0])
    torch.manual_seed(15)
    plain = _run(d, "ddim", cond, x_T, zs=_zs(79, 10), pag_scale=PAG_S)[0]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], plain)


# ---------------------------------------------------------------------------------------- learned variance, 'native'

def test_learned_variance_native_reads_the_variance_from_the_conditional_half(cond):
    """the 2C-wide drop-in UNet under the 'lv_native' update: the mean channels guided with (1 + s) c - s p, the variance
    channels of the CONDITIONAL half; float64 restatement, teacher-forced, as tests/test_hip_learned_variance.py holds the
    CFG form (1e-5 rel-L2: the bound of the sampler kernels against their float64 restatements)"""
    import math

    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    from sgdm_amd.synth import weights_from_seed
    from sgdm_amd.unet import UNetModel
    m = UNetModel(condition=AttrDict(scale_type="imagen"), **dict(INDEX["uf_label_c32_s16"]["ctor"], out_channels=6))
    m.load_state_dict(weights_from_seed([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 23))
    m = m.cuda().eval()
    m.hip_precision = "f16x3"
    d = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, parameterization="eps", learn_sigma=True))
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    K, T = 10, 1000
    times = [int(round(i * (T - 1) / (K - 1))) for i in range(K)]
    zs = _zs(81, K)
    x_T = _x_T(80)
    out = {}
    for graph in (False, True):
        torch.manual_seed(5)
        out[graph] = _run(d, "native", cond, x_T, graph, zs=zs, pag_scale=PAG_S, temperature=0.9)
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1]["x_inter"], out[True][1]["x_inter"])
    final, x_inter = out[True][0], out[True][1]["x_inter"]
    assert tuple(x_inter.shape) == (K,) + SHAPE and bool(torch.isfinite(x_inter).all())
    ac = d.sampler.alphas_cumprod.double().cpu().numpy()[times]
    ap = np.concatenate([[1.0], ac[:-1]])
    beta = 1 - ac / ap
    c1, c2, pv = beta * np.sqrt(ap) / (1 - ac), (1 - ap) * np.sqrt(1 - beta) / (1 - ac), beta * (1 - ap) / (1 - ac)
    mx, mn = np.log(beta), np.log(np.maximum(pv, 1e-300))
    mn[0] = mn[1]
    ins = [x_T.cpu()] + list(x_inter[:-1])
    errs, wrong = [], []
    for k, i in enumerate(reversed(range(K))):
        x = ins[k].double()
        raw = _halves(m, ins[k], times[i], cond).double()                       # [2B, hw, 6]
        mean = _nchw((1 + PAG_S) * raw[:B, :, :3] - PAG_S * raw[B:, :, :3])
        x0 = (math.sqrt(1 / ac[i]) * x - math.sqrt(1 / ac[i] - 1) * mean).clamp(-1, 1)
        nxt = []
        for half in (raw[:B], raw[B:]):
            frac = (_nchw(half[:, :, 3:]) + 1) / 2
            sig = torch.exp(0.5 * (frac * mx[i] + (1 - frac) * mn[i]))
            nxt.append(c1[i] * x0 + c2[i] * x + (0.0 if i == 0 else 0.9) * sig * zs[i].double())
        errs.append(rel_l2(x_inter[k], nxt[0]))
        wrong.append(rel_l2(x_inter[k], nxt[1]))
    print(f"learn_sigma native-10, PAG s {PAG_S}: captured == eager; vs float64 restatement, teacher-forced: max rel_l2 "
          f"{max(errs):.3e}; with the perturbed half's variance instead: {max(wrong):.3e}")
    assert max(errs) <= 1e-5, errs
    assert max(wrong) > 1e-4                                                    # the two halves' variances do differ
    # the guidance schedule stays refused on this update, under PAG too
    with pytest.raises(ValueError):
        _run(d, "native", cond, x_T, pag_scale=PAG_S, cfg_rescale=0.5)
