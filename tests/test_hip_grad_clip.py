"""Global-norm gradient clipping fused into the AdamW + EMA step (include/sgdm_hip.h: sgd_grad_norm, sgd_grad_scale,
sgd_adamw_ema_clip_step; sgdm_amd/optim.py: FusedAdamWEma(max_grad_norm=...), clip_grad_norm_).  GPU only.

Bounds.  The norm is accumulated in double (the square of an fp32 value is exact there, the sum of n of them is off by ~n 2^-53
relative at worst) and rounded to fp32 once: it lies within one fp32 ulp (2^-23 relative) of the float64 norm.  The coefficient is
torch's fp32 formula operation by operation, so it is compared bit for bit with its numpy-fp32 restatement.  The clipped step is
the plain step's kernel body on g * coef: bitwise against a twin optimizer fed the pre-multiplied gradients.  Against torch
(clip_grad_norm_ + AdamW + LitEma) the bounds are those of the unclipped comparison in tests/test_hip_train.py (2e-6 of the value
scale); torch's norm is an fp32 accumulation, hence 2^-22 there."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SIZES = [(1,), (255,), (4096,), (4097,), (2 * 4096 + 1,), (3, 10000), (257 * 4096 + 1,)]     # chunk and fold boundaries
MAGS = [1e-12, 1e-8, 1e-4, 1.0, 1e4, 1e8, 1e12]
NULL_ROW_N = 5000                        # a row with g == NULL: two chunks that contribute nothing


def _bits(x):
    return np.float32(x).view(np.uint32)


class _Abi:
    """the C-ABI entries on a list of gradient tensors (None: a row with g == NULL), with a record of its own"""

    def __init__(self):
        from sgdm_amd import _lib as L
        self.L, self.lib = L, L.load()
        self.rec = torch.zeros(8, dtype=torch.int32, device="cuda")

    def table(self, grads):
        from sgdm_amd.optim import chunk_table
        rows = [(0, g.data_ptr() if g is not None else 0, 0, 0, 0, g.numel() if g is not None else NULL_ROW_N) for g in grads]
        start = chunk_table([r[5] for r in rows])
        return (torch.tensor(rows, dtype=torch.int64).cuda(), torch.tensor(start, dtype=torch.int32).cuda(), len(rows), start[-1])

    def norm(self, grads, max_norm=float("inf")):
        tab, cs, count, total = self.table(grads)
        partials = torch.full((total,), float("nan"), dtype=torch.float64, device="cuda")     # every slot must be written
        self.L.check(self.lib.sgd_grad_norm(tab.data_ptr(), cs.data_ptr(), count, total, partials.data_ptr(), max_norm,
                                            self.rec.data_ptr(), torch.cuda.current_stream().cuda_stream), "sgd_grad_norm")
        return self.stats()

    def stats(self):
        h = self.rec.cpu().numpy()
        f = h[:2].view(np.float32)
        return dict(norm=f[0], coef=f[1], skip=int(h[2]), clipped_steps=int(h[3]), nonfinite_steps=int(h[4]), pad=h[5:].tolist())


def _mixed_grads(mags=MAGS):
    g = torch.Generator().manual_seed(11)
    return [(torch.randn(s, generator=g) * m).cuda() for s, m in zip(SIZES, mags)]


def _ref_norm(grads):
    return float(np.sqrt(sum(float((g.double().cpu() ** 2).sum()) for g in grads if g is not None)))


@pytest.fixture(scope="module")
def mixed():
    grads = _mixed_grads()
    return grads, _ref_norm(grads)


def test_norm_within_one_ulp_of_float64_and_independent_of_addresses(mixed):
    grads, ref = mixed
    abi = _Abi()
    rows = grads[:3] + [None] + grads[3:]
    a = abi.norm(rows)
    print(f"\nnorm {a['norm']!r} vs float64 {ref!r}: rel {abs(float(a['norm']) - ref) / ref:.3e} (bound {ULP:.3e})")
    assert a["skip"] == 0 and a["coef"] == np.float32(1) and a["pad"] == [0, 0, 0]
    assert abs(float(a["norm"]) - ref) <= ULP * ref
    # every tensor alone: the small magnitudes are invisible in the total, here each one has to count
    for g, s in zip(grads, SIZES):
        one, r1 = abi.norm([g]), _ref_norm([g])
        assert abs(float(one["norm"]) - r1) <= ULP * r1, (s, one["norm"], r1)
    # squares outside fp32's range in both directions (1e-50 and 1e50) still count in full
    for m in (1e-25, 1e25):
        ext = _mixed_grads([m] * len(SIZES))
        e, r = abi.norm(ext), _ref_norm(ext)
        assert e["skip"] == 0 and abs(float(e["norm"]) - r) <= ULP * r, (m, e["norm"], r)
    # the same call again: the same bits
    b = abi.norm(rows)
    assert _bits(b["norm"]) == _bits(a["norm"])
    # the same values at other addresses: cloned tensors, and one flat buffer in which every tensor starts 4 bytes past a
    # 16-byte boundary (the kernel's 4-byte path)
    clones = [g.clone() if g is not None else None for g in rows]
    assert _bits(abi.norm(clones)["norm"]) == _bits(a["norm"])
    flat = torch.zeros(sum((g.numel() + 7) // 4 * 4 for g in grads) + 4, device="cuda")
    views, off = [], 1
    for g in grads:
        v = flat[off:off + g.numel()]
        v.copy_(g.reshape(-1))
        assert v.data_ptr() % 16 == 4
        views.append(v)
        off += (g.numel() + 7) // 4 * 4
    assert _bits(abi.norm(views[:3] + [None] + views[3:])["norm"]) == _bits(a["norm"])
    for g, c in zip(grads, clones[:3] + clones[4:]):                   # the norm reads only
        assert torch.equal(g, c)


def test_coefficient_is_torchs_formula_in_fp32_and_the_counters_run():
    g = torch.Generator().manual_seed(12)
    grads = [torch.randn(s, generator=g).cuda() for s in ((7,), (4097,), (3, 1000))]
    abi = _Abi()
    norm = float(abi.norm(grads)["norm"])

    def want(mx, nrm):
        return np.minimum(np.float32(1), np.float32(mx) / (np.float32(nrm) + np.float32(1e-6)))

    seen = dict(clipped_steps=0, nonfinite_steps=0)
    for mx, clipped in ((norm / 2, True), (norm / 3.7, True), (1e-3, True), (norm * 2, False), (norm * 1.0000001, False)):
        s = abi.norm(grads, mx)
        seen["clipped_steps"] += int(clipped)
        assert _bits(s["coef"]) == _bits(want(mx, s["norm"])), (mx, s["coef"], want(mx, s["norm"]))
        assert (s["coef"] < 1) == clipped and s["skip"] == 0
        assert {k: s[k] for k in seen} == seen
    for mx in (0.0, float("inf"), -1.0, float("nan")):                 # norm-only mode
        s = abi.norm(grads, mx)
        assert _bits(s["coef"]) == _bits(1.0) and s["skip"] == 0 and {k: s[k] for k in seen} == seen
    for poison in (float("inf"), float("nan")):
        bad = [x.clone() for x in grads]
        bad[1][4096] = poison                                          # the last element, in the second chunk
        s = abi.norm(bad, norm / 2)
        seen["nonfinite_steps"] += 1
        assert s["skip"] == 1 and s["coef"] == 0 and not np.isfinite(s["norm"]) and {k: s[k] for k in seen} == seen
    s = abi.norm(grads, norm / 2)                                      # and a finite step clears skip again
    assert s["skip"] == 0 and s["clipped_steps"] == seen["clipped_steps"] + 1 and s["nonfinite_steps"] == 2
    # argument checks: nothing launched
    tab, cs, count, total = abi.table(grads)
    part = torch.zeros(total, dtype=torch.float64, device="cuda")
    lib, rec = abi.lib, abi.rec.data_ptr()
    assert lib.sgd_grad_norm(None, cs.data_ptr(), count, total, part.data_ptr(), 1.0, rec, None) == 1
    assert lib.sgd_grad_norm(tab.data_ptr(), cs.data_ptr(), count, total, None, 1.0, rec, None) == 1
    assert lib.sgd_grad_norm(tab.data_ptr(), cs.data_ptr(), count, total, part.data_ptr(), 1.0, None, None) == 1
    assert lib.sgd_grad_norm(tab.data_ptr(), cs.data_ptr(), 0, total, part.data_ptr(), 1.0, rec, None) == 1
    assert lib.sgd_grad_scale(tab.data_ptr(), cs.data_ptr(), count, 0, rec, None) == 1
    assert lib.sgd_grad_scale(tab.data_ptr(), cs.data_ptr(), count, total, None, None) == 1


# ------------------------------------------------------------------------------------------------------------------------
# the optimizer: the module of test_fused_adamw_ema_matches_torch_adamw_and_litema (tests/test_hip_train.py)
# ------------------------------------------------------------------------------------------------------------------------
class _M(torch.nn.Module):
    def __init__(self):
        super().__init__()
        nn, g = torch.nn, torch.Generator().manual_seed(3)
        self.a = nn.Parameter(torch.randn(1, generator=g))
        self.b = nn.Parameter(torch.randn(5, 7, generator=g))
        self.c = nn.Parameter(torch.randn(4097, generator=g))
        self.d = nn.Parameter(torch.randn(3, 10000, generator=g))
        self.unused = nn.Parameter(torch.randn(33, generator=g))
        self.frozen = nn.Parameter(torch.randn(9, generator=g), requires_grad=False)


def _two_groups(m):
    return [dict(params=[m.a, m.b, m.unused], lr=3e-3), dict(params=[m.c, m.d], lr=1e-3, weight_decay=0.05)]


def _fused(m, **kw):
    from sgdm_amd.ema import LitEma
    from sgdm_amd.optim import FusedAdamWEma
    ema = LitEma(m).cuda()
    return FusedAdamWEma(_two_groups(m), lr=3e-3, weight_decay=0.01, ema=ema, ema_model=m, **kw), ema


def _grads_for(m, gen, scale):
    return {n: torch.randn(p.shape, generator=gen).cuda() * scale for n, p in m.named_parameters()
            if n not in ("unused", "frozen")}


def _snapshot(m, opt, ema):
    out = {f"p.{n}": p.detach().clone() for n, p in m.named_parameters()}
    shadow = dict(ema.named_buffers())                                 # (the shadows only: num_updates is a host-side count)
    out.update({f"s.{n}": shadow[s].detach().clone() for n, s in ema.m_name2s_name.items()})
    for n, p in m.named_parameters():
        for k in ("exp_avg", "exp_avg_sq"):
            if k in opt.state.get(p, {}):
                out[f"{k}.{n}"] = opt.state[p][k].detach().clone()
    return out


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_clipped_step_is_the_plain_kernel_on_premultiplied_gradients():
    """3 steps over two param groups; step 0 is not clipped (coef == 1: bit-identical to the step without the option), steps 1
    and 2 are.  Control: a twin FusedAdamWEma without max_grad_norm, fed g * coef formed in torch from the record's coef."""
    m1, m2 = _M().cuda(), _M().cuda()
    o1, e1 = _fused(m1, max_grad_norm=5.0)
    o2, e2 = _fused(m2)
    gen = torch.Generator().manual_seed(4)
    coefs = []
    for step in range(3):
        grads = _grads_for(m1, gen, 10.0 ** (step - 2))               # norms ~1.8, ~18, ~180 against max_grad_norm 5
        for n, g in grads.items():
            m1.get_parameter(n).grad = g.clone()
        o1.step()
        st = o1.clip_stats()
        coefs.append(st["coef"])
        ref = float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values())))
        assert abs(st["norm"] - ref) <= ULP * ref and st["skipped"] is False
        assert float(o1.grad_norm) == st["norm"] and o1.grad_norm.is_cuda and o1.grad_norm.dim() == 0
        for n, g in grads.items():
            assert torch.equal(m1.get_parameter(n).grad, g), n          # p.grad bitwise untouched
            m2.get_parameter(n).grad = g * st["coef"]                   # one rounded fp32 product
        o2.step()
        torch.cuda.synchronize()
        bad = _same_bits(_snapshot(m1, o1, e1), _snapshot(m2, o2, e2))
        assert not bad, (step, bad)
        assert m1.unused.grad is None and not o1.state[m1.unused]
    print(f"\ncoefs {coefs}")
    assert coefs[0] == 1.0 and coefs[1] < 1.0 and coefs[2] < coefs[1]
    assert o1.clip_stats()["clipped_steps"] == 2 and o1.clip_stats()["nonfinite_steps"] == 0
    assert int(e1.num_updates) == int(e2.num_updates) == 3
    assert "max_grad_norm" not in o1.state_dict()["param_groups"][0]
    # cleared, the optimizer is the plain one again
    o1.max_grad_norm = None
    for mm, oo in ((m1, o1), (m2, o2)):
        for n, g in _grads_for(mm, torch.Generator().manual_seed(9), 100.0).items():
            mm.get_parameter(n).grad = g
        oo.step()
    assert not _same_bits(_snapshot(m1, o1, e1), _snapshot(m2, o2, e2))
    assert o1.clip_stats()["clipped_steps"] == 2


def test_clipped_step_matches_torch_clip_adamw_and_litema():
    from conftest import max_rel
    from sgdm_amd.ema import LitEma
    m1, m2 = _M().cuda(), _M().cuda()
    e1 = LitEma(m1).cuda()
    o1 = torch.optim.AdamW(_two_groups(m1), lr=3e-3, weight_decay=0.01)
    o2, e2 = _fused(m2, max_grad_norm=5.0)
    gen = torch.Generator().manual_seed(4)
    trainable = [p for p in m1.parameters() if p.requires_grad]
    for step in range(4):
        for n, g in _grads_for(m1, gen, 10.0 ** (step - 2)).items():
            m1.get_parameter(n).grad, m2.get_parameter(n).grad = g.clone(), g.clone()
        tn = torch.nn.utils.clip_grad_norm_(trainable, 5.0)
        o1.step()
        e1(m1)
        o2.step()
        rel = abs(float(o2.grad_norm) - float(tn)) / float(tn)
        print(f"\nstep {step}: norm {float(o2.grad_norm)!r} torch {float(tn)!r} rel {rel:.3e}")
        assert rel <= 2.0 ** -22, (step, rel)
    torch.cuda.synchronize()

    def close(x, ref):          # 2e-6 of the value scale (tests/test_hip_train.py)
        return float((x.double() - ref.double()).abs().max()) <= 2e-6 * max(float(ref.abs().max()), 1.0)

    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert close(p2.detach().cpu(), p1.detach().cpu()), n1
    for (n1, b1), (n2, b2) in zip(e1.named_buffers(), e2.named_buffers()):
        assert close(b2.float().cpu(), b1.float().cpu()), n1
    assert int(e2.num_updates) == 4 and o2.clip_stats()["clipped_steps"] == 3
    for g1, g2 in zip(o1.param_groups, o2.param_groups):
        for p1, p2 in zip(g1["params"], g2["params"]):
            if p1.grad is None:
                assert not o2.state[p2]
                continue
            assert max_rel(o2.state[p2]["exp_avg"].cpu(), o1.state[p1]["exp_avg"].cpu()) < 2e-6
            assert max_rel(o2.state[p2]["exp_avg_sq"].cpu(), o1.state[p1]["exp_avg_sq"].cpu()) < 2e-6


@pytest.mark.parametrize("poison", [float("inf"), float("nan")])
def test_non_finite_norm_voids_the_step_on_the_device(poison):
    """one poisoned element: nothing is written; the next finite step updates as it would have after a step voided by the health
    gate (the twin: the plain optimizer with the gate raised by hand for that step -- st['step'] advances on both)"""
    from sgdm_amd.unet import grad_health
    m1, m2 = _M().cuda(), _M().cuda()
    o1, e1 = _fused(m1, max_grad_norm=float("inf"))                   # measure and guard, never scale
    o2, e2 = _fused(m2)
    gen = torch.Generator().manual_seed(5)
    gate = grad_health(m1.a.device)
    try:
        for mm, oo in ((m1, o1), (m2, o2)):                           # a first ordinary step: moments exist
            for n, g in _grads_for(mm, torch.Generator().manual_seed(6), 1.0).items():
                mm.get_parameter(n).grad = g
            oo.step()
        before = _snapshot(m1, o1, e1)
        assert not _same_bits(before, _snapshot(m2, o2, e2))
        grads = _grads_for(m1, gen, 1.0)
        grads["d"][2, 9999] = poison
        for n, g in grads.items():
            m1.get_parameter(n).grad, m2.get_parameter(n).grad = g.clone(), g.clone()
        o1.step()
        st = o1.clip_stats()
        assert st["skipped"] is True and st["nonfinite_steps"] == 1 and st["coef"] == 0.0 and not np.isfinite(st["norm"])
        assert not np.isfinite(float(o1.grad_norm))
        assert not _same_bits(before, _snapshot(m1, o1, e1))          # parameters, moments, shadows: bitwise unchanged
        gate.fill_(1)
        o2.step()
        gate.zero_()
        assert not _same_bits(before, _snapshot(m2, o2, e2))
        # with the gate up the clipped step writes nothing either, whatever the record says
        m3 = _M().cuda()
        o3, e3 = _fused(m3, max_grad_norm=0.5)
        b3 = _snapshot(m3, o3, e3)
        for n, g in _grads_for(m3, torch.Generator().manual_seed(7), 1.0).items():
            m3.get_parameter(n).grad = g
        gate.fill_(1)
        o3.step()
        gate.zero_()
        after3 = _snapshot(m3, o3, e3)
        assert not [k for k in b3 if not torch.equal(b3[k], after3[k])]
        assert all(bool((after3[k] == 0).all()) for k in after3 if k.startswith("exp_avg"))
        assert o3.clip_stats()["skipped"] is False and o3.clip_stats()["coef"] < 1.0
        # the next finite step updates normally
        for mm, oo in ((m1, o1), (m2, o2)):
            for n, g in _grads_for(mm, torch.Generator().manual_seed(8), 1.0).items():
                mm.get_parameter(n).grad = g
            oo.step()
        after = _snapshot(m1, o1, e1)
        assert not _same_bits(after, _snapshot(m2, o2, e2))
        assert all(not torch.equal(after[k], before[k]) for k in after if k.split(".")[-1] in "abcd")
        st = o1.clip_stats()
        assert st["skipped"] is False and st["nonfinite_steps"] == 1 and np.isfinite(st["norm"])
    finally:
        gate.zero_()


def test_clip_grad_norm_function():
    from sgdm_amd.optim import clip_grad_norm_
    abi = _Abi()
    m = _M().cuda()
    grads = _grads_for(m, torch.Generator().manual_seed(13), 1.0)
    ref = _ref_norm(list(grads.values()))

    def load():
        for n, g in grads.items():
            m.get_parameter(n).grad = g.clone()

    def want_coef(mx, nrm):
        return np.minimum(np.float32(1), np.float32(mx) / (np.float32(nrm) + np.float32(1e-6)))

    # an iterable of parameters (a generator; `unused` and `frozen` have no gradient and are skipped), clipped
    load()
    norm = clip_grad_norm_((p for p in m.parameters()), ref / 3)
    assert norm.is_cuda and norm.dim() == 0 and norm.dtype == torch.float32
    rec_norm = abi.norm(list(grads.values()))["norm"]                   # the C-ABI's norm of the same gradients
    assert _bits(float(norm)) == _bits(rec_norm) and abs(float(norm) - ref) <= ULP * ref
    coef = want_coef(ref / 3, float(norm))
    assert coef < 1
    for n, g in grads.items():
        assert torch.equal(m.get_parameter(n).grad, g * float(coef)), n
    assert m.unused.grad is None and m.frozen.grad is None
    # an optimizer that is not ours, unclipped: bitwise untouched
    load()
    sgd = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.1)
    n2 = clip_grad_norm_(sgd, ref * 2)
    assert _bits(float(n2)) == _bits(rec_norm)
    assert _bits(float(norm)) == _bits(rec_norm)                         # the earlier return value is the caller's own
    for n, g in grads.items():
        assert torch.equal(m.get_parameter(n).grad, g), n
    # non-finite: the gradients are left as they are, the norm says so
    load()
    m.c.grad[17] = float("nan")
    kept = {n: m.get_parameter(n).grad.clone() for n in grads}
    n3 = clip_grad_norm_(m.parameters(), ref / 3)
    assert not np.isfinite(float(n3))
    for n in grads:
        assert torch.equal(m.get_parameter(n).grad.nan_to_num(7.0), kept[n].nan_to_num(7.0)), n
    # refused: a non-contiguous gradient, an fp16 gradient
    load()
    m.d.grad = torch.randn(10000, 3).cuda().t()
    with pytest.raises(RuntimeError):
        clip_grad_norm_(m.parameters(), 1.0)
    load()
    h = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16, device="cuda"))
    h.grad = torch.ones(8, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError):
        clip_grad_norm_([m.a, h], 1.0)


# ------------------------------------------------------------------------------------------------------------------------
# the training loop: the ch-32, 16x16, batch-4 model of tests/test_hip_train.py::_run_loop at f16x3, every step clipped
# ------------------------------------------------------------------------------------------------------------------------
def _clip_loop(kind, max_norm, steps=3, lr=1e-3, name="uf_clusterlayout_c32_s16", prec="f16x3"):
    """kind: 'fused' (FusedAdamWEma(max_grad_norm)) | 'torch' (torch clip_grad_norm_ + torch.optim.AdamW + LitEma.forward)"""
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    from sgdm_amd.ema import LitEma
    from sgdm_amd.optim import FusedAdamWEma
    from test_hip_train import _loop_inputs
    from test_hip_unet import build_model
    m, entry = build_model(name, prec)
    m.dropout = 0.0
    m.train()
    d = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS).train()
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    ema = LitEma(m).cuda()
    params = [p for p in m.parameters() if p.requires_grad]
    if kind == "fused":
        opt = FusedAdamWEma(params, lr=lr, weight_decay=0.01, ema=ema, ema_model=m, max_grad_norm=max_norm)
    else:
        opt = torch.optim.AdamW(params, lr=lr, weight_decay=0.01)
    losses, norms = [], []
    for step in range(steps):
        batch, t, noise, mask = _loop_inputs(entry, step)
        loss, _ = d.p_losses(batch["image"].cuda(), t.cuda(), noise.cuda(), cond=batch["cond"].float().cuda(),
                             layout=batch["layout"].cuda() if "layout" in batch else None, cond_drop_prob=0.5,
                             cond_drop_mask=mask.cuda())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if kind == "torch":
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
        if kind == "torch":
            ema(m)
        else:
            norms.append(float(opt.grad_norm))
        losses.append(loss.item())
        if step == 0:
            params1 = {k: p.detach().cpu().clone() for k, p in m.named_parameters()}
            shadows1 = {k: dict(ema.named_buffers())[s].detach().cpu().clone() for k, s in ema.m_name2s_name.items()}
    batch, t, noise, mask = _loop_inputs(entry, 99)
    m.eval()

    def ev():
        with torch.no_grad():
            return m(batch["image"].cuda(), t.cuda(), cond=batch["cond"].float().cuda(),
                     layout=batch["layout"].cuda() if "layout" in batch else None, cond_drop_prob=0.0,
                     cond_drop_mask=mask.cuda())[0].cpu()
    eps = ev()
    ema.store(m.parameters())
    ema.copy_to(m)
    eps_ema = ev()
    ema.restore(m.parameters())
    return dict(losses=losses, norms=norms, eps=eps, eps_ema=eps_ema, params=params1, shadows=shadows1,
                stats=opt.clip_stats() if kind == "fused" else None)


def test_training_loop_with_every_step_clipped_matches_torch():
    from conftest import max_rel
    probe = _clip_loop("fused", float("inf"), steps=1)                 # one unclipped step: its norm
    assert probe["stats"]["coef"] == 1.0 and probe["stats"]["clipped_steps"] == 0
    max_norm = 0.5 * probe["norms"][0]
    a = _clip_loop("fused", max_norm)
    b = _clip_loop("torch", max_norm)
    print(f"\nmax_grad_norm {max_norm!r}: norms fused {a['norms']} torch {b['norms']}")
    assert a["stats"]["clipped_steps"] == 3 and a["stats"]["nonfinite_steps"] == 0
    assert a["norms"][0] == probe["norms"][0]
    for na, nb in zip(a["norms"], b["norms"]):
        assert abs(na - nb) <= 1e-5 * nb
    # the bounds of test_training_loop_fused_optimizer_updates_the_packed_weights (tests/test_hip_train.py), fused vs torch
    for la, lb in zip(a["losses"], b["losses"]):
        assert abs(la - lb) <= 1e-5 * abs(lb), (a["losses"], b["losses"])
    assert max_rel(a["eps"], b["eps"]) < 1e-5
    assert max_rel(a["eps_ema"], b["eps_ema"]) < 1e-5
    for k in a["params"]:
        assert float((a["params"][k] - b["params"][k]).abs().max()) <= 2e-6 * max(1.0, float(b["params"][k].abs().max())), k
    for k in a["shadows"]:
        assert float((a["shadows"][k] - b["shadows"][k]).abs().max()) <= 2e-6 * max(1.0, float(b["shadows"][k].abs().max())), k
