"""Self-attention guidance on the HIP path (Hong et al. 2023; sampling kwargs sag_scale / sag_layer / sag_threshold /
sag_blur_sigma).  csrc/sag.hip: sgd_attention_colmass, sgd_sag_degrade; sgdm_amd/diffusion.py: _StepRunner.sag_pair / sag_degrade,
_GraphedStep; sgdm_amd/sampling_plan.py: sag_options.  The reference has no such guidance.  Expected values: the float64 formula
on the same fp32 q, k, lse (mass kernel), sgdm_amd/sag.py: sag_degrade_torch in fp32 (max abs diff 0) and float64 (degrade
kernel), the oracle with ``attention_block`` patched to expose its softmax (engine; tests/test_sag_cpu.py builds it), and every
sampler's step restated in torch fp32 from the recorded engine outputs and the kernel's own mass, with the update restatements
of tests/test_hip_pag.py.  GPU only; every test prints the figures it asserts on (-s).

Measured on the MI355X: mass kernel at most 1.9e-7 max-rel from float64 (bound 1e-4), |sum_j mass - T| / T at most 3.0e-7, runs
bit-identical; degrade kernel max abs diff 0 against torch fp32 in all twelve cases and at most 5.8e-8 rel-L2 from float64 (bound
1e-5); engine mass within 4.3e-7 (f32) / 9.4e-7 (f16x3) max-rel of the patched oracle's; all 18 sampler cases max abs diff 0 and
captured == eager; cfg_rescale over the pair 1.2e-8 rel-L2 from the restated guide pass."""
import ctypes
import math

import pytest
import torch

import test_hip_pag as PT
from conftest import cfg_from_index, max_rel, rel_l2
from test_hip_pag import CASES, _engine_inputs, _nchw, _plan, _restate, _run, _steps, _x_T, _zs
from test_hip_unet import INDEX, TOL, build_model
from test_hip_vpred import B, S, SHAPE, _diffusion, _guided32, _sk, _st
from test_sag_cpu import MID, oracle_mass

pytestmark = pytest.mark.gpu

SAG_S = 0.75
SENT = -7.0
PSI = 1.0


# ---------------------------------------------------------------------------------------------------------- mass kernel

def _qkv_case(batch, heads, t, d, layout, pad):
    """qkv [batch + 1, t, 3 * heads * d + pad] on the device, its (head stride, k offset, v offset)"""
    inner = heads * d
    g = torch.Generator().manual_seed(1000 * t + d + batch)
    qkv = (0.7 * torch.randn(batch + 1, t, 3 * inner + pad, generator=g)).cuda()
    return qkv, ((3 * d, d, 2 * d) if layout == "legacy" else (d, inner, 2 * inner))


def _colmass(lib, qkv, lay, batch, heads, t, d, scale, mass, lse):
    hs, ko, vo = lay
    ld = qkv.shape[-1]
    att = torch.empty(batch, t, heads * d, device="cuda")
    k, v = ctypes.c_void_p(qkv.data_ptr() + 4 * ko), ctypes.c_void_p(qkv.data_ptr() + 4 * vo)
    assert lib.sgd_attention(qkv.data_ptr(), ld, hs, k, v, ld, hs, batch, heads, t, t, d, scale, att.data_ptr(), heads * d,
                             lse.data_ptr(), _st()) == 0
    return lib.sgd_attention_colmass(qkv.data_ptr(), ld, hs, k, ld, hs, lse.data_ptr(), batch, heads, t, t, d, scale,
                                     mass.data_ptr(), _st())


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("layout", ["legacy", "new"])
@pytest.mark.parametrize("batch,heads,t,d", [(3, 2, 5, 16), (2, 4, 64, 32), (1, 1, 1, 128), (2, 3, 17, 64), (1, 2, 257, 32)])
def test_colmass_kernel(batch, heads, t, d, layout, pad):
    """against the float64 formula on the same fp32 q, k and the lse sgd_attention wrote.  The bound is the project's parity
    contract, 1e-4 max-rel; a sum of positive terms carries each term's relative error, ~3e-6 here (fp32 dot, exp, the lse)"""
    from sgdm_amd import _lib as L
    from sgdm_amd.sag import qk_views, sag_mass_torch
    lib = L.load()
    qkv, lay = _qkv_case(batch, heads, t, d, layout, pad)
    keep = qkv.clone()
    scale = 1.0 / math.sqrt(d)
    lse = torch.full((batch + 1, heads, t), SENT, device="cuda")
    mass = torch.full((batch + 1, t), SENT, device="cuda")
    assert _colmass(lib, qkv, lay, batch, heads, t, d, scale, mass, lse) == 0
    again = torch.full((batch + 1, t), SENT, device="cuda")
    assert _colmass(lib, qkv, lay, batch, heads, t, d, scale, again, lse) == 0
    torch.cuda.synchronize()
    q, k = (a[:batch].double().cpu() for a in qk_views(qkv[:, :, :qkv.shape[-1]], heads, d, lay))
    want = sag_mass_torch(q, k, lse[:batch].double().cpu(), scale)
    got = mass.cpu()
    err = max_rel(got[:batch], want)
    tot = float((got[:batch].double().sum(1) - t).abs().max() / t)
    print(f"sgd_attention_colmass {(batch, heads, t, d)} {layout} ld {qkv.shape[-1]}: max-rel vs float64 {err:.2e}; "
          f"|sum_j mass - T| / T {tot:.2e}; mass in [{float(want.min()):.3f}, {float(want.max()):.3f}]")
    assert err <= 1e-4 and tot <= 1e-4
    assert torch.equal(mass, again)                                             # run to run: the same bits
    assert bool((got[batch:] == SENT).all()) and bool((lse[batch:] == SENT).all())   # rows beyond batch
    assert torch.equal(qkv, keep)


def test_colmass_kernel_refuses_bad_arguments():
    from sgdm_amd import _lib as L
    lib = L.load()
    batch, heads, t, d = 2, 2, 5, 32
    qkv, (hs, ko, vo) = _qkv_case(batch, heads, t, d, "legacy", 0)
    ld = qkv.shape[-1]
    lse = torch.zeros(batch, heads, t, device="cuda")
    mass = torch.full((batch, t), SENT, device="cuda")
    q, k = qkv.data_ptr(), qkv.data_ptr() + 4 * ko
    args = dict(q=q, q_ld=ld, q_hs=hs, k=k, kv_ld=ld, kv_hs=hs, lse=lse.data_ptr(), batch=batch, heads=heads, tq=t, tk=t, d=d,
                scale=0.25, mass=mass.data_ptr(), st=_st())
    call = lambda **kw: lib.sgd_attention_colmass(*dict(args, **kw).values())      # (keyword order is the C argument order)
    bad = [dict(d=24), dict(d=0), dict(d=256), dict(q=q + 4), dict(k=k + 4), dict(q_ld=ld + 2), dict(kv_ld=ld + 1),
           dict(q_hs=hs + 1), dict(kv_hs=hs + 2), dict(q=None), dict(k=None), dict(lse=None), dict(mass=None), dict(batch=0),
           dict(heads=0), dict(tq=0), dict(tk=-1), dict(q_ld=0), dict(kv_ld=-4)]
    for b in bad:
        assert call(**b) == 1, b                                                    # SGD_ERR_ARG
    torch.cuda.synchronize()
    assert bool((mass == SENT).all())                                               # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((mass != SENT).all())


# ------------------------------------------------------------------------------------------------------- degrade kernel

def _degrade_case(b, c, h, w, mh, mw, seed=0):
    """x, the network output with a padded row stride, times, the two tables, a positive mass centred on psi"""
    g = torch.Generator().manual_seed(seed + 100 * h + w)
    x = torch.randn(b, c, h, w, generator=g)
    out = torch.randn(b, h * w, c + 2, generator=g)
    ac = torch.linspace(0.98, 0.02, 50, dtype=torch.float64)
    t = torch.randint(0, 50, (b,), generator=g)
    mass = (PSI + 0.8 * (torch.rand(b, mh * mw, generator=g) - 0.5)).float()
    return x, out, t, ac.sqrt().float(), (1 - ac).sqrt().float(), mass


def _degrade(lib, x, out, par, t, sa, s1, mass, mh, mw, thr, taps, with_copy=True):
    from sgdm_amd.sag import PAR_ID
    b, c, h, w = x.shape
    dev = [a.cuda() for a in (x, out, t, sa, s1, mass, taps)]
    x_deg = torch.full((b + 1, c, h, w), SENT, device="cuda")
    copy = torch.full((b + 1, h * w, c), SENT, device="cuda")
    rc = lib.sgd_sag_degrade(dev[0].data_ptr(), dev[1].data_ptr(), out.shape[-1], PAR_ID[par], dev[2].data_ptr(),
                             dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), mh, mw, thr, dev[6].data_ptr(), b, c, h, w,
                             x_deg.data_ptr(), copy.data_ptr() if with_copy else None, _st())
    torch.cuda.synchronize()
    assert rc == 0
    return x_deg.cpu(), copy.cpu()


DEGRADE_SHAPES = [(1, 1, 5, 5, 1, 1), (2, 3, 16, 16, 4, 4), (2, 4, 12, 20, 3, 5), (1, 3, 64, 64, 8, 8)]


@pytest.mark.parametrize("par", ["eps", "x0", "v"])
@pytest.mark.parametrize("b,c,h,w,mh,mw", DEGRADE_SHAPES)
def test_degrade_kernel(b, c, h, w, mh, mw, par):
    """max abs diff 0 against sag_degrade_torch in fp32 (the restatement thresholds the same fp32 mass: no element can flip);
    rel-L2 <= 1e-5 against its float64 form, the bound the samplers' float64 restatements use"""
    from sgdm_amd import _lib as L
    from sgdm_amd.sag import gaussian_taps, sag_degrade_torch, sag_mask
    lib = L.load()
    x, out, t, sa, s1, mass = _degrade_case(b, c, h, w, mh, mw)
    taps = gaussian_taps(1.0).float()
    M = sag_mask(mass, mh, mw, h, w, PSI)
    assert mh * mw == 1 or all(bool(M[n].any()) and bool((~M[n]).any()) for n in range(b))    # both values in every sample
    got, copy = _degrade(lib, x, out, par, t, sa, s1, mass, mh, mw, PSI, taps)
    want = sag_degrade_torch(x, out, par, t, sa, s1, mass, mh, mw, PSI, taps)
    want64 = sag_degrade_torch(x.double(), out.double(), par, t, sa, s1, mass, mh, mw, PSI, taps.double())
    diff, err = float((got[:b] - want).abs().max()), rel_l2(got[:b], want64)
    print(f"sgd_sag_degrade {par} {(b, c, h, w)}/{(mh, mw)}: max abs diff vs torch fp32 {diff}; rel-L2 vs float64 {err:.2e}; "
          f"masked {float(M.float().mean()):.2f}")
    assert err <= 1e-5
    assert diff == 0.0
    assert torch.equal(copy[:b], out[:, :, :c].contiguous())                    # out_copy: the rows of out, bit for bit
    assert bool((got[b:] == SENT).all()) and bool((copy[b:] == SENT).all())     # nothing beyond the batch
    # without out_copy: the same image
    assert torch.equal(_degrade(lib, x, out, par, t, sa, s1, mass, mh, mw, PSI, taps, with_copy=False)[0], got)
    # an all-false mask re-noises the prediction unchanged, an all-true mask gives the blurred image
    from sgdm_amd.sag import sag_blur_torch, sag_split_torch
    a, s = sa[t].view(b, 1, 1, 1), s1[t].view(b, 1, 1, 1)
    x0, e = sag_split_torch(x, out[:, :, :c].reshape(b, h, w, c).permute(0, 3, 1, 2), par, a, s)
    none = _degrade(lib, x, out, par, t, sa, s1, mass, mh, mw, 100.0, taps)[0][:b]
    every = _degrade(lib, x, out, par, t, sa, s1, mass, mh, mw, 1e-3, taps)[0][:b]
    assert torch.equal(none, a * x0 + s * e) and torch.equal(every, a * sag_blur_torch(x0, taps) + s * e)
    assert not torch.equal(none, every)


def test_degrade_kernel_refuses_bad_arguments():
    from sgdm_amd import _lib as L
    lib = L.load()
    b, c, h, w, mh, mw = 2, 3, 8, 6, 2, 3
    x, out, t, sa, s1, mass = (a.cuda() for a in _degrade_case(b, c, h, w, mh, mw))
    from sgdm_amd.sag import gaussian_taps
    taps = gaussian_taps(1.0).float().cuda()
    x_deg = torch.full((b, c, h, w), SENT, device="cuda")
    copy = torch.full((b, h * w, c), SENT, device="cuda")
    args = dict(x=x.data_ptr(), out=out.data_ptr(), out_ld=c + 2, par=0, t=t.data_ptr(), sa=sa.data_ptr(), s1=s1.data_ptr(),
                mass=mass.data_ptr(), mh=mh, mw=mw, thr=PSI, taps=taps.data_ptr(), b=b, c=c, h=h, w=w, x_deg=x_deg.data_ptr(),
                copy=copy.data_ptr(), st=_st())
    call = lambda **kw: lib.sgd_sag_degrade(*dict(args, **kw).values())
    bad = [dict(x=None), dict(out=None), dict(t=None), dict(sa=None), dict(s1=None), dict(mass=None), dict(taps=None),
           dict(x_deg=None), dict(b=0), dict(c=0), dict(par=3), dict(par=-1), dict(out_ld=c - 1), dict(h=4), dict(w=4), dict(h=0),
           dict(mh=0), dict(mw=0), dict(mh=h + 1), dict(mw=w + 1), dict(x_deg=x.data_ptr())]
    for k in bad:
        assert call(**k) == 1, k                                                    # SGD_ERR_ARG
    torch.cuda.synchronize()
    assert bool((x_deg == SENT).all()) and bool((copy == SENT).all())               # nothing was launched
    assert call() == 0 and call(copy=None) == 0
    torch.cuda.synchronize()
    assert bool((x_deg != SENT).all())


# ---------------------------------------------------------------------------------------------------------------- engine

ENGINE_MODELS = ["uf_label_c32_s16", "uf_heads8_label_c32_s16", "uf_newattn_label_c32_s16"]
_REFS = {}


def _oracle(name):
    if name not in _REFS:
        from sgdm_amd.synth import weights_from_seed
        entry = INDEX[name]
        x, t, cond = _engine_inputs(entry)
        sd = weights_from_seed(entry["manifest"], entry["seed"])
        _REFS[name] = oracle_mass(pytest.MonkeyPatch(), cfg_from_index(entry), sd, x, t, cond.float())
    return _REFS[name]


def _engine_mass(m, eng, layer=MID):
    """the mass kernel over the tape buffers ``layer`` left in ``eng``, as _StepRunner.sag_degrade launches it"""
    from sgdm_amd import _lib as L
    rec = next(r for r in eng.tape if r["kind"] == "attn" and r["p"] == layer)
    qkv, heads, dp = rec["qkv"], rec["heads"], rec["dp"]
    hs, ko, _ = rec["qkv_layout"]
    mass = torch.empty(eng.n, rec["T"], device="cuda")
    rc = L.load().sgd_attention_colmass(qkv.data_ptr(), 3 * heads * dp, hs, ctypes.c_void_p(qkv.data_ptr() + 4 * ko), 3 * heads * dp,
                                        hs, rec["lse"].data_ptr(), eng.n, heads, rec["T"], rec["T"], dp, 1.0 / math.sqrt(rec["d"]),
                                        mass.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0
    return mass.cpu(), rec["hw"]


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("name", ENGINE_MODELS)
def test_engine_mass_agrees_with_the_patched_oracle(name, prec):
    m, entry = build_model(name, prec)
    x, t, cond = (a.cuda() for a in _engine_inputs(entry))
    with torch.no_grad():
        eng = m._run(x, t, cond, None, torch.zeros(B, dtype=torch.bool, device="cuda"), B)
    got, hw = _engine_mass(m, eng)
    out, want, hw_ref = _oracle(name)
    err, err_out = max_rel(got, want), max_rel(eng.eps_nhwc.permute(0, 3, 1, 2).cpu(), out)
    tot = float((got.double().sum(1) - got.shape[1]).abs().max() / got.shape[1])
    print(f"{name} [{prec}] mass of {MID} {hw}: max-rel vs the patched oracle {err:.2e} (output {err_out:.2e}, bound "
          f"{TOL[prec]:.0e}); |sum - T| / T {tot:.2e}; mass in [{float(want.min()):.3f}, {float(want.max()):.3f}]")
    assert tuple(hw) == tuple(hw_ref) and got.shape == want.shape
    assert err < TOL[prec] and err_out < TOL[prec] and tot <= 1e-4


# ---------------------------------------------------------------------------------------------------------- trajectories

@pytest.fixture(scope="module")
def model():
    return build_model("uf_label_c32_s16", "f16x3")[0]


@pytest.fixture(scope="module")
def cond():
    from sgdm_amd.synth import synth_batch
    return synth_batch("label", B, S, 10, seed=23)["cond"].cuda()


def _record(mp):
    """tests/test_hip_pag.py's record of steps and eager evaluations, plus per SAG evaluation what the two launches read and
    wrote -- the image, the pair [o ; o~], the degraded image, the mass, the times -- captured (the step's static buffers after
    the replay) and eager (the buffers handed to sag_degrade, after sag_pair returns) alike"""
    from sgdm_amd import diffusion as Dm
    rec = PT._record(mp)
    rec.update(sag=[], runner=[], launches=[])
    g1, deg0, pair0 = Dm._GraphedStep.step, Dm._StepRunner.sag_degrade, Dm._StepRunner.sag_pair

    def gstep(self, i, *a, **k):
        x = self.img.clone()
        n0 = self.replays["guided"]
        g1(self, i, *a, **k)
        if getattr(self, "sag", None) and self.replays["guided"] > n0:
            rec["sag"].append(dict(x=x.cpu(), t=self.t.cpu(), pair=self.pair.cpu(), x_deg=self.x_deg.cpu(), mass=self.mass.cpu()))

    def degrade(self, eng, x, t, pair, x_deg, mass, st, tables=None, taps=None):
        rec["runner"].append(self)
        rec["launches"].append(1)
        self._held = (x, t, pair, x_deg, mass)                  # (references only: this also runs under a capture)
        return deg0(self, eng, x, t, pair, x_deg, mass, st, tables, taps)

    def spair(self, x, t):
        pair = pair0(self, x, t)
        x_, t_, pair_, x_deg, mass = self._held
        assert pair_ is pair
        rec["sag"].append(dict(x=x_.cpu(), t=t_.cpu(), pair=pair.cpu(), x_deg=x_deg.cpu(), mass=mass.cpu()))
        return pair
    mp.setattr(Dm._GraphedStep, "step", gstep)
    mp.setattr(Dm._StepRunner, "sag_degrade", degrade)
    mp.setattr(Dm._StepRunner, "sag_pair", spair)
    return rec


def _restate_sag(rec, par, opts=(SAG_S, MID, PSI, 1.0)):
    """every recorded SAG evaluation: the second UNet input restated in torch fp32 from the recorded first output and the
    kernel's own mass.  Returns the max abs difference"""
    from sgdm_amd.sag import gaussian_taps, sag_degrade_torch
    runner = rec["runner"][0]
    sa, s1 = (a.cpu() for a in runner.tables)
    taps = gaussian_taps(opts[3]).float()
    eng = next(e for k, e in runner.model._engines.items() if k[0] == B and len(k) == 4)
    mh, mw = runner.sag_record(eng)["hw"]                                       # the layer's map size
    diffs = []
    for ev in rec["sag"]:
        assert ev["mass"].shape == (B, mh * mw) and abs(float(ev["mass"].sum(1).mean()) - mh * mw) < 1e-3
        want = sag_degrade_torch(ev["x"], ev["pair"][:B], par, ev["t"], sa, s1, ev["mass"], mh, mw, opts[2], taps)
        diffs.append(float((ev["x_deg"] - want).abs().max()))
    return max(diffs), len(diffs)


# 'x0': only 'native' reads the network output as x0 (its rows), the other samplers read it as eps like the reference; SAG forms
# its degraded image from the parameterization in force either way
X0_CASES = [(method, "x0", "eps") for method in ("native", "ddim", "plms", "pndm", "dpmsolver")]


@pytest.mark.parametrize("method,par,form", CASES + X0_CASES)
def test_trajectory_captured_equals_eager_and_the_restated_method(method, par, form, model, cond, monkeypatch):
    """10 steps at s = 0.75 on the middle attention: captured == eager bit for bit; every UNet input -- the image of each step
    and the degraded image of its second evaluation -- and the final image equal the method restated in torch fp32 from the
    recorded engine outputs and the kernel's own mass, max abs diff 0.  cond_scale (here 2.0) is not read"""
    d = _diffusion(par, model)
    skx = dict(sag_scale=SAG_S, **(dict(v_form="data") if form == "data" else {}))
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
    assert len(_steps(model)) == (0 if method == "plms" else 1)             # (plms has no captured step: its eps is the caller's)
    same = torch.equal(out[False][0], out[True][0]) and all(torch.equal(out[False][1][k], out[True][1][k]) for k in out[True][1])
    assert len(recs[False]["steps"]) == len(recs[True]["steps"]) and len(recs[False]["sag"]) == len(recs[True]["sag"])
    same = same and all(torch.equal(a[2], b[2]) for a, b in zip(recs[False]["steps"], recs[True]["steps"]))
    same = same and all(torch.equal(a[k], b[k]) for a, b in zip(recs[False]["sag"], recs[True]["sag"]) for k in a)
    rec = recs[True]
    d_deg, n_deg = _restate_sag(rec, par)
    # the update of every step from the recorded pair, guided in torch fp32: tests/test_hip_pag.py's restatement, its engine
    # call replaced by the record (in the order the restatement asks: the evaluations' own)
    pairs = iter(rec["sag"])

    def guided(model_, x, t, cond_, **kw):
        ev = next(pairs)
        assert torch.equal(ev["x"], x) and int(ev["t"][0]) == int(t)       # the first UNet input: the step's own image
        return _nchw(_guided32(ev["pair"], 2, SAG_S, B))
    with monkeypatch.context() as mp:
        mp.setattr(PT, "_guided", guided)
        d_upd, n_upd = _restate(d, method, par, form, model, cond, rec, times, tab, zs)
    final = torch.equal(out[True][0], rec["steps"][-1][2])
    print(f"SAG s {SAG_S} {MID}, {method}/{par}/{form}: captured == eager: {same}; {n_deg} degraded inputs vs the restated "
          f"method: max abs diff {d_deg}; {n_upd} updates, teacher-forced: max abs diff {d_upd}; final image is the last update: {final}")
    assert torch.isfinite(out[True][0]).all() and same and final
    assert n_deg == (11 if method == "plms" else len(times)) and d_deg == 0.0 and d_upd == 0.0
    assert all(bool((ev["mass"] > PSI).any()) for ev in rec["sag"])             # the mask selected something at every step
    # the guidance does something: another weight, and the plain conditional trajectory, are other trajectories
    torch.manual_seed(21)
    other = _run(d, method, cond, x_T, True, zs=zs, **dict(skx, sag_scale=0.25))[0]
    torch.manual_seed(21)
    plain = _run(d, method, cond, x_T, True, zs=zs, cfg_distilled=True, **{k: v for k, v in skx.items() if k != "sag_scale"})[0]
    assert not torch.equal(other, out[True][0]) and not torch.equal(plain, out[True][0])


# ---------------------------------------------------------------------------------------------------- further assertions

def test_scale_type_and_cond_scale_are_not_read(cond):
    outs = []
    for st, w in (("imagen", 2.0), ("cfg", 7.0)):
        m, _ = build_model("uf_label_c32_s16", "f16x3", st)
        d = _diffusion("eps", m)
        torch.manual_seed(3)
        outs.append(_run(d, "dpmsolver", cond, _x_T(72), True, w=w, sag_scale=SAG_S)[0])
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_sweep_over_sag_scale_under_cfg_rescale_is_one_capture(model, cond, monkeypatch):
    from sgdm_amd import diffusion as Dm
    d = _diffusion("eps", model)
    x_T = _x_T(73)
    model.__dict__.pop("_hip_graph_steps", None)
    captures = []
    cap0 = Dm._GraphedStep._capture
    monkeypatch.setattr(Dm._GraphedStep, "_capture", staticmethod(lambda *a, **k: (captures.append(1), cap0(*a, **k))[1]))
    sweep = []
    for s in (0.25, 0.75, 1.5):
        torch.manual_seed(11)
        sweep.append(_run(d, "ddim", cond, x_T, sag_scale=s, cfg_rescale=0.7))
    print(f"sweep over sag_scale 0.25, 0.75, 1.5 (cfg_rescale 0.7): {len(captures)} capture(s), {len(_steps(model))} cached step(s)")
    assert len(captures) == 1 and len(_steps(model)) == 1
    assert not torch.equal(sweep[0][0], sweep[1][0]) and not torch.equal(sweep[1][0], sweep[2][0])
    torch.manual_seed(11)
    again = _run(d, "ddim", cond, x_T, sag_scale=0.25, cfg_rescale=0.7)
    assert len(captures) == 1 and torch.equal(again[0], sweep[0][0])
    # the threshold, sigma and the layer are part of the key: each is a capture of its own
    for extra in (dict(sag_threshold=0.9), dict(sag_blur_sigma=2.0), dict(sag_layer="output_blocks.0.1")):
        torch.manual_seed(11)
        got = _run(d, "ddim", cond, x_T, sag_scale=0.25, cfg_rescale=0.7, **extra)
        assert torch.isfinite(got[0]).all() and not torch.equal(got[0], sweep[0][0])
    assert len(captures) == 4 and len(_steps(model)) == 4


def test_cfg_rescale_is_the_restated_guide_pass_over_the_pair(model, cond, monkeypatch):
    """teacher-forced on every step of a dpmsolver trajectory: g = (1 + s) o - s o~ in torch fp32, scaled per sample towards
    std(o) as sgd_cfg_guide does (float64 restatement of the two standard deviations: rel-L2 <= 1e-5), then the update"""
    phi = 0.7
    d = _diffusion("eps", model)
    times, tab = _plan(d, "dpmsolver", {})
    model.__dict__.pop("_hip_graph_steps", None)
    out = {}
    for graph in (False, True):
        torch.manual_seed(17)
        with monkeypatch.context() as mp:
            rec = _record(mp)
            out[graph] = _run(d, "dpmsolver", cond, _x_T(74), graph, sag_scale=SAG_S, cfg_rescale=phi)[0]
    assert torch.equal(out[False], out[True])
    errs, hist = [], None
    for (i, x, x_out), ev in zip(rec["steps"], rec["sag"]):
        g = _guided32(ev["pair"], 2, SAG_S, B).double()
        k = phi * ev["pair"][:B].double().reshape(B, -1).std(1) / g.reshape(B, -1).std(1) + (1 - phi)
        e = _nchw((k.view(B, 1, 1) * g).float())
        want, hist = PT._upd_dpm(x, e, tab[i], hist)
        errs.append(rel_l2(x_out, want))
    print(f"SAG + cfg_rescale {phi}, dpmsolver: captured == eager; {len(errs)} steps vs the restated guide pass: max rel-L2 {max(errs):.2e}")
    assert len(errs) == 10 and max(errs) <= 1e-5
    assert _restate_sag(rec, "eps")[0] == 0.0


def test_interval_that_hits_nothing_is_the_conditional_trajectory_and_launches_no_sag_kernel(model, cond, monkeypatch):
    d = _diffusion("eps", model)
    x_T = _x_T(75)
    torch.manual_seed(9)
    want = _run(d, "ddim", cond, x_T, cfg_distilled=True, ddim_eta=1.0)
    model.__dict__.pop("_hip_graph_steps", None)
    from sgdm_amd import _lib as L
    calls = []
    lib = L.load()
    for name in ("sgd_attention_colmass", "sgd_sag_degrade"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, fn=fn, name=name: (calls.append(name), fn(*a))[1])
    for graph in (True, False):
        torch.manual_seed(9)
        got = _run(d, "ddim", cond, x_T, graph, sag_scale=SAG_S, cfg_interval=(2, 100), ddim_eta=1.0)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1]["x_inter"], want[1]["x_inter"])
    (step,) = _steps(model)
    assert step.replays == dict(guided=0, cond=10)
    assert calls == ["sgd_attention_colmass", "sgd_sag_degrade"]                # the capture of the guided graph, no replay of it
    # an interval that hits some evaluations: a third trajectory, captured == eager
    outs = []
    for graph in (True, False):
        torch.manual_seed(9)
        outs.append(_run(d, "ddim", cond, x_T, graph, sag_scale=SAG_S, cfg_interval=(301, 601), ddim_eta=1.0)[0])
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], want[0])
    assert step.replays == dict(guided=4, cond=6)
    assert len(calls) == 2 + 2 * 4                                              # eager: two launches per guided evaluation


def test_dynamic_thresholding_runs_under_sag(model, cond):
    d = _diffusion("eps", model)
    x_T = _x_T(78)
    outs = []
    for graph in (True, False):
        torch.manual_seed(15)
        outs.append(_run(d, "ddim", cond, x_T, graph, zs=_zs(79, 10), sag_scale=SAG_S, dtp=0.9)[0])
    torch.manual_seed(15)
    plain = _run(d, "ddim", cond, x_T, zs=_zs(79, 10), sag_scale=SAG_S)[0]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], plain)


def test_rng_is_that_of_two_single_evaluations(model, cond):
    """each of the two evaluations draws as the model's single forward(cond_drop_prob=p0) does, captured and eager"""
    d = _diffusion("eps", model)
    x_T = _x_T(77)
    rng = []
    for graph in (False, True):
        torch.manual_seed(13)
        _run(d, "dpmsolver", cond, x_T, graph, sag_scale=SAG_S)
        rng.append(torch.cuda.get_rng_state().clone())
    torch.manual_seed(13)
    for _ in range(20):
        model._draw_mask(B, 0.0, "cuda")
    assert torch.equal(rng[0], rng[1]) and torch.equal(rng[0], torch.cuda.get_rng_state())


def test_without_the_kwargs_engines_and_launches_are_what_they_were(cond, monkeypatch):
    from sgdm_amd import _lib as L
    m, _ = build_model("uf_label_c32_s16", "f16x3")
    d = _diffusion("eps", m)
    x_T = _x_T(75)
    calls = []
    lib = L.load()
    for name in ("sgd_attention_colmass", "sgd_sag_degrade"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, fn=fn, name=name: (calls.append(name), fn(*a))[1])
    launches = []
    from sgdm_amd.unet import _Engine
    launch0 = _Engine.launch
    monkeypatch.setattr(_Engine, "launch", lambda self, st, inputs=None: (launches.append(self.n), launch0(self, st, inputs))[1])
    outs = {}
    for method in ("native", "ddim", "plms", "pndm", "dpmsolver"):
        torch.manual_seed(4)
        outs[method] = _run(d, method, cond, x_T, zs=_zs(76, 10))[0]
        torch.manual_seed(4)
        assert torch.equal(_run(d, method, cond, x_T, zs=_zs(76, 10), sag_scale=0)[0], outs[method])       # 0 is off
    prec = L.PREC_BY_NAME["f16x3"]
    assert not calls and set(m._engines) == {(2 * B, S, S, prec)} and set(launches) == {2 * B}
    # eager launches of the plain step: one engine launch at 2B per evaluation, as before
    n0 = len(launches)
    torch.manual_seed(4)
    assert torch.equal(_run(d, "ddim", cond, x_T, False, zs=_zs(76, 10))[0], outs["ddim"])
    assert launches[n0:] == [2 * B] * 10
    # SAG on the same model: the engine at B, twice per step, and afterwards the default trajectories are the same bits
    n0 = len(launches)
    torch.manual_seed(4)
    _run(d, "ddim", cond, x_T, False, zs=_zs(76, 10), sag_scale=SAG_S)
    assert launches[n0:] == [B] * 20 and len(calls) == 20 and set(m._engines) == {(2 * B, S, S, prec), (B, S, S, prec)}
    for method in ("ddim", "dpmsolver"):
        torch.manual_seed(4)
        assert torch.equal(_run(d, method, cond, x_T, zs=_zs(76, 10))[0], outs[method])
