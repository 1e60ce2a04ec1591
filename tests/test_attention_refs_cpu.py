"""The float64 attention references and the case generator of tests/attention_refs.py, checked without a GPU: the geometry
tests of the HIP cores (tests/test_hip_attention_geometry.py) are only as good as what they compare against."""
import pytest
import torch
import torch.nn.functional as F

import attention_refs as R

# two small shapes per layout: (b, heads, tq, tk, d); the legacy layout has tq == tk
SHAPES = {"legacy": [(2, 3, 7, 7, 16), (1, 2, 33, 33, 32)],
          "separate": [(2, 3, 5, 9, 16), (1, 2, 33, 40, 64)],
          "mq": [(2, 3, 5, 9, 16), (1, 4, 33, 40, 32)]}


def _inputs(layout, shape, seed=0):
    """float64 q, k, v that went through the layout's own row packing and back (the helpers the GPU tests use)"""
    b, heads, tq, tk, d = shape
    g = torch.Generator().manual_seed(seed)
    hk = 1 if layout == "mq" else heads
    q = torch.randn(b, heads, tq, d, generator=g, dtype=torch.float64)
    k = torch.randn(b, hk, tk, d, generator=g, dtype=torch.float64)
    v = torch.randn(b, hk, tk, d, generator=g, dtype=torch.float64)
    if layout == "legacy":
        q2, k2, v2 = R.legacy_split(R.legacy_rows(q, k, v, 3 * heads * d + 4), heads, d)
    else:
        q2 = R.heads_of(R.rows_of(q, heads * d + 12), heads, d)
        kv = torch.cat([R.rows_of(k, hk * d), R.rows_of(v, hk * d + 4)], -1)           # [k | v | pad]
        k2, v2 = R.heads_of(kv, hk, d), R.heads_of(kv[:, :, hk * d:], hk, d)
    assert torch.equal(q2, q) and torch.equal(k2, k) and torch.equal(v2, v)
    return q2, k2, v2


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_forward_reference_equals_sdpa(layout):
    for shape in SHAPES[layout]:
        b, heads, tq, tk, d = shape
        q, k, v = _inputs(layout, shape)
        scale = d ** -0.5
        out, lse = R.ref_attention(q, k, v, scale)
        ke, ve = k.expand(-1, heads, -1, -1), v.expand(-1, heads, -1, -1)
        want = F.scaled_dot_product_attention(q, ke, ve, scale=scale)
        assert out.dtype == torch.float64 and float((out - want).abs().max()) < 1e-12
        s = torch.einsum("bhid,bhjd->bhij", q, ke) * scale
        assert float((lse - torch.logsumexp(s, -1)).abs().max()) < 1e-12
        # masked: the reference's own formulation, masked_fill(~mask, -finfo(float32).max) before the softmax
        mask = torch.rand(b, tk, generator=torch.Generator().manual_seed(1)) > 0.4
        mask[:, 0] = True
        outm, lsem = R.ref_attention(q, k, v, scale, mask)
        sm = s.masked_fill(~mask[:, None, None, :], -torch.finfo(torch.float32).max)
        wantm = torch.einsum("bhij,bhjd->bhid", sm.softmax(-1), ve)
        assert float((outm - wantm).abs().max()) < 1e-12
        assert float((lsem - torch.logsumexp(sm, -1)).abs().max()) < 1e-12
        # ... which is attention over the attended keys alone
        for i in range(b):
            oc, lc = R.ref_attention(q[i:i + 1], k[i:i + 1, :, mask[i]], v[i:i + 1, :, mask[i]], scale)
            assert float((outm[i:i + 1] - oc).abs().max()) < 1e-12 and float((lsem[i:i + 1] - lc).abs().max()) < 1e-12


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("hk", [2, 1])
def test_gradient_reference_equals_finite_differences(hk, masked):
    """central differences of sum(out * dout) in float64 at one tiny shape (d = 16, tq = 3, tk = 5)"""
    b, heads, tq, tk, d = 2, 2, 3, 5, 16
    g = torch.Generator().manual_seed(3)
    q = torch.randn(b, heads, tq, d, generator=g, dtype=torch.float64)
    k = torch.randn(b, hk, tk, d, generator=g, dtype=torch.float64)
    v = torch.randn(b, hk, tk, d, generator=g, dtype=torch.float64)
    dout = torch.randn(b, heads, tq, d, generator=g, dtype=torch.float64)
    mask = torch.tensor([[True, False, True, True, False], [True, True, False, True, True]]) if masked else None
    scale = d ** -0.5
    grads = R.ref_attention_grads(q, k, v, dout, scale, mask)
    assert [t.shape for t in grads] == [q.shape, k.shape, v.shape]

    def loss(qq, kk, vv):
        return float((R.ref_attention(qq, kk, vv, scale, mask)[0] * dout).sum())

    eps = 1e-6
    args = [q, k, v]
    for which, grad in enumerate(grads):
        num = torch.empty_like(grad)
        flat = args[which].reshape(-1)
        for i in range(flat.numel()):
            keep = float(flat[i])
            flat[i] = keep + eps
            up = loss(*args)
            flat[i] = keep - eps
            down = loss(*args)
            flat[i] = keep
            num.reshape(-1)[i] = (up - down) / (2 * eps)
        # truncation eps^2 |f'''| ~ 1e-12 and rounding 1e-16 |f| / eps ~ 1e-9: both far below the bound
        assert float((num - grad).abs().max()) < 1e-7 * max(1.0, float(grad.abs().max())), "qkv"[which]
    if masked:
        assert float(grads[1][~mask[:, None, :].expand(b, hk, tk)].abs().max()) == 0.0
        assert float(grads[2][~mask[:, None, :].expand(b, hk, tk)].abs().max()) == 0.0
    if hk == 1:                 # multi-query: dk / dv are the per-head gradients, summed
        _, dk_h, dv_h = R.ref_attention_grads(q, k.expand(-1, heads, -1, -1), v.expand(-1, heads, -1, -1), dout, scale, mask)
        assert float((grads[1] - dk_h.sum(1, keepdim=True)).abs().max()) < 1e-13
        assert float((grads[2] - dv_h.sum(1, keepdim=True)).abs().max()) < 1e-13


def test_gradient_scales_bound_the_gradients():
    """the absolute-value forms bound |dq|, |dk|, |dv| element by element, and stay positive where one attended key makes dq and
    dk exactly zero (what the GPU sweeps divide by there)"""
    g = torch.Generator().manual_seed(4)
    for hk, tk, mask in ((2, 5, None), (1, 5, torch.tensor([[True, False, True, True, False]])), (2, 1, None),
                         (1, 5, torch.tensor([[True, False, False, False, False]]))):
        q = torch.randn(1, 2, 3, 16, generator=g)
        k, v = torch.randn(1, hk, tk, 16, generator=g), torch.randn(1, hk, tk, 16, generator=g)
        dout = torch.randn(1, 2, 3, 16, generator=g)
        grads = R.ref_attention_grads(q, k, v, dout, 0.25, mask)
        scales = R.ref_attention_grad_scales(q, k, v, dout, 0.25, mask)
        for gr, sc in zip(grads, scales):
            assert gr.shape == sc.shape and bool((gr.abs() <= sc * (1 + 1e-12)).all())
        one_key = tk == 1 or (mask is not None and int(mask.sum()) == 1)
        assert (float(grads[0].abs().max()) == 0.0 and float(grads[1].abs().max()) == 0.0) == one_key
        assert all(float(sc.max()) > 0.0 for sc in scales)


@pytest.mark.parametrize("name", sorted(R.SWEEPS))
def test_generator_invariants(name):
    kw = R.SWEEPS[name]
    cases = R.sweep_cases(name)
    assert len(cases) == kw["n"] == 24
    assert cases == R.sweep_cases(name), "the draw is seeded"
    assert R.stratification_gaps(cases, dims=kw["dims"], masked=kw["masked"]) == []
    for cs in cases:
        b, heads, d, tq, tk = cs["b"], cs["heads"], cs["d"], cs["tq"], cs["tk"]
        assert b in R.BATCHES and heads in R.HEADS and d in kw["dims"] and cs["sharp"] in R.SHARPS
        assert b * heads * tq * tk * d <= 2 * 3 * 257 * 273 * 128
        for key in ("q_ld", "kv_ld", "out_ld", "dout_ld", "q_hs", "kv_hs"):
            assert cs[key] % 4 == 0, (key, cs)
        for key in R.PAD_KEYS:
            assert cs[key] in R.PADS
        assert cs["out_ld"] == heads * d + cs["out_pad"] and cs["dout_ld"] == heads * d + cs["dout_pad"]
        if cs["layout"] == "legacy":
            assert tq == tk and (tq in R.TQS or tq in R.TKS)
            assert cs["q_ld"] == cs["kv_ld"] == 3 * heads * d + cs["q_pad"] and cs["q_hs"] == cs["kv_hs"] == 3 * d
        else:
            assert tq in R.TQS and tk in R.TKS
            assert cs["q_ld"] == heads * d + cs["q_pad"] and cs["q_hs"] == d
            hk = 1 if cs["layout"] == "mq" else heads
            assert cs["kv_ld"] == 2 * hk * d + cs["kv_pad"] and cs["kv_hs"] == (0 if cs["layout"] == "mq" else d)
        mask = R.case_mask(cs)
        t = R.case_tensors(cs)
        assert t["q"].shape == (b, heads, tq, d) and t["dout"].shape == (b, heads, tq, d)
        assert t["k"].shape == t["v"].shape == (b, 1 if cs["layout"] == "mq" else heads, tk, d)
        if not kw["masked"]:
            assert mask is None and "mask_pattern" not in cs
            continue
        assert cs["layout"] != "legacy"
        if kw.get("backward") and cs["layout"] == "mq":
            assert heads == 1
        assert mask.shape == (b, tk) and mask.dtype == torch.bool and bool(mask[:, 0].all()), cs
        pat = cs["mask_pattern"]
        if pat == "only_key0":
            assert int(mask.sum()) == b
        elif pat == "last_masked":
            assert not bool(mask[:, -1].any())
        elif pat == "subtile_then_valid":
            assert not bool(mask[:, 32:64].any()) and bool(mask[:, 64].all())
        elif pat == "valid_then_subtile":
            first = (tk - 1) // 32 * 32
            assert first >= 32 and not bool(mask[:, first:].any()) and bool(mask[:, first - 1].all())
    if kw["masked"] and not kw.get("backward"):
        assert any(cs["layout"] == "mq" and cs["heads"] > 1 for cs in cases), "the masked forward shares K / V among heads"


def test_guarded_buffer_on_the_cpu():
    buf = R.Guarded(3, 8, cols=5, device="cpu")
    assert buf.untouched() and not buf.written()
    buf.tensor()[:, :5] = 1.0
    assert buf.untouched() and buf.written() and torch.equal(buf.owned(), torch.ones(3, 5))
    for spot in ((0, 5), (2, 7)):                       # padding columns
        b2 = R.Guarded(3, 8, cols=5, device="cpu")
        b2.tensor()[spot] = 0.0
        assert not b2.untouched()
    for off in (0, 7, 4 * 8, 5 * 8 - 1):                # the guard rows in front and behind
        b2 = R.Guarded(3, 8, cols=5, device="cpu")
        b2.bits[off] = 0
        assert not b2.untouched()
    b2 = R.Guarded(3, 8, cols=5, device="cpu")
    b2.tensor()[1, 6] = float("nan")                    # another NaN is not the pattern
    assert not b2.untouched()
