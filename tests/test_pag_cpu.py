"""Perturbed-attention guidance (Ahn et al. 2024; sampling kwargs pag_scale / pag_layers / pag_drop_cond) where it needs no GPU:
the option parsing (sgdm_amd/diffusion.py: pag_options -- every refusal is raised before the library is loaded), the
resolution of the layer sets against the oracle's block plan, the binding of the new entry (include/sgdm_hip.h:
sgd_attention_identity) and the reference the GPU tests use: the oracle's forward with ``attention_block`` patched to a = v for
the chosen layers on rows [B, 2B).  The reference project has no such guidance; oracle/ is not touched."""
import os
import re

import pytest
import torch

from conftest import PKG, ROOT, cfg_from_index, load_json

INDEX = load_json("unet_index.json")


# ------------------------------------------------------------------------------------------ the patched oracle (shared)

def patched_attention(U, prefixes, B):
    """``oracle.unet_ref.attention_block`` with the attention map of the layers in ``prefixes`` replaced by the identity on rows
    [B, 2B): a = v there (each query's output is its own value row), the original everywhere else"""
    orig = U.attention_block
    prefixes = frozenset(prefixes)

    def attention_block(sd, p, x, heads, new_order=False):
        out = orig(sd, p, x, heads, new_order)
        if p not in prefixes:
            return out
        import torch.nn.functional as F
        b, c, hh, ww = x.shape
        assert b == 2 * B, (b, B)
        xf = x[B:].reshape(B, c, -1)
        qkv = F.conv1d(U._gn(sd, p + ".norm", xf), sd[p + ".qkv.weight"], sd[p + ".qkv.bias"])
        length, ch = qkv.shape[-1], c // heads
        if new_order:
            v = qkv.chunk(3, dim=1)[2].reshape(B * heads, ch, length)
        else:
            v = qkv.reshape(B * heads, ch * 3, length).split(ch, dim=1)[2]
        h = F.conv1d(v.reshape(B, -1, length), sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"])
        return torch.cat((out[:B], (xf + h).reshape(B, c, hh, ww)), 0)
    return attention_block


def pag_forward(monkeypatch, cfg, sd, x, t, cond, layout, prefixes, drop_cond=False):
    """the doubled evaluation [conditional | perturbed] of the oracle, [2B, C, H, W]"""
    from oracle import unet_ref as U
    B = x.shape[0]
    dbl = lambda a: None if a is None else torch.cat((a, a), 0)
    mask = torch.cat((torch.zeros(B, dtype=torch.bool), torch.full((B,), bool(drop_cond))))
    with monkeypatch.context() as mp:
        mp.setattr(U, "attention_block", patched_attention(U, prefixes, B))
        with torch.no_grad():
            return U.unet_forward(cfg, sd, dbl(x), dbl(t), dbl(cond), dbl(layout), mask)


def _plan_model(name="uf_label_c32_s16"):
    """the drop-in model on the host, as pag_options reads it: its own block plan, kind and attention type (no device)"""
    from sgdm_amd.unet import UNetModel, UNetModelCA
    from test_hip_unet import AttrDict
    entry = INDEX[name]
    cond = AttrDict(scale_type="imagen")
    if entry["layout_dim"]:
        cond[entry["ctor"]["condition_method"]] = AttrDict(layout_dim=entry["layout_dim"])
    return (UNetModel if entry["kind"] == "unet_fast" else UNetModelCA)(condition=cond, **entry["ctor"])


# ------------------------------------------------------------------------------------------------------------- options

def test_defaults_and_off():
    from sgdm_amd.diffusion import pag_options
    m = _plan_model()
    for sk in (None, {}, dict(pag_scale=0), dict(pag_scale=0.0), dict(cfg_rescale=0.5)):
        assert pag_options(sk, True, m) is None
    assert pag_options({}, False, None) is None                                 # off: nothing asked of the step
    assert pag_options(dict(pag_scale=1.5), True, m) == (1.5, ("middle_block.1",), False)
    assert pag_options(dict(pag_scale=2, pag_layers="mid", pag_drop_cond=True), True, m) == (2.0, ("middle_block.1",), True)
    s, layers, drop = pag_options(dict(pag_scale=3.0, cond_scale=7.0), True, m)   # cond_scale is not read
    assert (s, drop) == (3.0, False) and isinstance(s, float) and isinstance(drop, bool)


@pytest.mark.parametrize("name", ["uf_label_c32_s16", "uf_heads8_label_c32_s16", "uf_newattn_label_c32_s16"])
def test_layer_sets_resolve_against_the_oracle_plan(name):
    from oracle import unet_ref as U
    from sgdm_amd.diffusion import pag_options
    from sgdm_amd.unet import attention_prefixes
    m = _plan_model(name)
    inp, mid, out = U.build_plan(cfg_from_index(INDEX[name]))
    want = [f"input_blocks.{i}.{j}" for i, b in enumerate(inp) for j, l in enumerate(b) if l[0] == "attn"]
    want += [f"middle_block.{j}" for j, l in enumerate(mid) if l[0] == "attn"]
    want += [f"output_blocks.{i}.{j}" for i, b in enumerate(out) for j, l in enumerate(b) if l[0] == "attn"]
    assert m.attention_prefixes() == attention_prefixes(m._plan) == want and "middle_block.1" in want and len(want) > 1
    assert pag_options(dict(pag_scale=1.0, pag_layers="all"), True, m)[1] == tuple(sorted(want))
    assert pag_options(dict(pag_scale=1.0, pag_layers="mid"), True, m)[1] == ("middle_block.1",)
    some = [want[-1], want[0], want[0]]                                         # any order, repeats: a sorted set
    assert pag_options(dict(pag_scale=1.0, pag_layers=some), True, m)[1] == tuple(sorted(set(some)))
    assert pag_options(dict(pag_scale=1.0, pag_layers=tuple(want)), True, m)[1] == tuple(sorted(want))
    # every prefix names parameters of an attention block
    from sgdm_amd.synth import weights_from_seed
    sd = weights_from_seed(INDEX[name]["manifest"], INDEX[name]["seed"])
    assert all(p + ".qkv.weight" in sd and p + ".proj_out.weight" in sd for p in want)


def test_refusals():
    from sgdm_amd.diffusion import pag_options
    m = _plan_model()
    bad = [dict(pag_scale=-0.1), dict(pag_scale="1.5"), dict(pag_scale=True), dict(pag_scale=False), dict(pag_scale=None),
           dict(pag_scale=float("nan")), dict(pag_scale=float("inf")), dict(pag_scale=[1.0]),
           dict(pag_layers="mid"), dict(pag_drop_cond=True), dict(pag_drop_cond=False), dict(pag_scale=0, pag_layers="all"),
           dict(pag_scale=0.0, pag_drop_cond=True),
           dict(pag_scale=1.0, cfg_distilled=True),
           dict(pag_scale=1.0, pag_layers="middle"), dict(pag_scale=1.0, pag_layers=["middle_block.0"]),
           dict(pag_scale=1.0, pag_layers=["middle_block.1", "output_blocks.99.1"]), dict(pag_scale=1.0, pag_layers=[]),
           dict(pag_scale=1.0, pag_layers=3), dict(pag_scale=1.0, pag_layers=[1]),
           dict(pag_scale=1.0, pag_drop_cond=1), dict(pag_scale=1.0, pag_drop_cond="yes")]
    for sk in bad:
        with pytest.raises(ValueError):
            pag_options(sk, True, m)
    with pytest.raises(ValueError):
        pag_options(dict(pag_scale=1.0), False, m)                              # not the fused step
    with pytest.raises(ValueError):
        pag_options(dict(pag_scale=1.0), True, None)                            # no drop-in UNet behind the step
    for name in ("ca_stego_c32_s16", "uf_st_label_c32_s16"):                    # Attention_LR / SpatialTransformer
        with pytest.raises(ValueError):
            pag_options(dict(pag_scale=1.0), True, _plan_model(name))
    # a plan without a middle attention: 'mid' selects nothing
    no_mid = _plan_model()
    inp, mid, out = no_mid._plan
    no_mid._plan = (inp, [l for l in mid if l[0] != "attn"], out)
    with pytest.raises(ValueError):
        pag_options(dict(pag_scale=1.0), True, no_mid)
    assert pag_options(dict(pag_scale=1.0, pag_layers="all"), True, no_mid)[1]


def test_step_runner_refuses_before_anything_is_loaded(monkeypatch):
    """a generic denoise_sample_fn, p0 and a tensor cond_scale are not the fused step; the library is never asked for"""
    from sgdm_amd import _lib as L
    from sgdm_amd import diffusion as Dm
    from sgdm_amd.unet import UNetModel
    from test_hip_unet import AttrDict

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    m = UNetModel(condition=AttrDict(scale_type="imagen"), **INDEX["uf_label_c32_s16"]["ctor"])
    fused = m.forward_with_cond_scale
    cases = [(lambda x, t, **kw: x, dict(cond_scale=2.0), dict(pag_scale=1.5)),
             (fused, dict(cond_scale=2.0, p0=torch.zeros(2)), dict(pag_scale=1.5)),
             (fused, dict(cond_scale=torch.ones(2, 1, 1, 1)), dict(pag_scale=1.5)),
             (fused, dict(cond_scale=2.0), dict(pag_scale=1.5, cfg_distilled=True)),
             (fused, dict(cond_scale=2.0), dict(pag_scale=-1.0)),
             (fused, dict(cond_scale=2.0), dict(pag_layers="all")),
             (fused, dict(cond_scale=2.0), dict(pag_scale=1.5, pag_layers=["input_blocks.0.0"]))]
    for fn, kw, sk in cases:
        with pytest.raises(ValueError):
            Dm._StepRunner(fn, kw, sk, "cpu")
    # the engine refuses the same before it builds anything (no device is touched: the check comes first)
    with pytest.raises(ValueError):
        m._pag_set(("middle_block.1",), 3)                                      # an odd UNet batch
    with pytest.raises(ValueError):
        m._pag_set(("middle_block.1", "input_blocks.4.1"), 4)                   # not sorted
    assert m._pag_set(("middle_block.1",), 4) == ("middle_block.1",)


def test_binding_and_header_declare_the_entry():
    from sgdm_amd import _lib as L
    res, args = L.SIGNATURES["sgd_attention_identity"]
    assert res is L.i32 and args == [L.vp, L.i32, L.i32, L.i32, L.i32, L.i32, L.i32, L.vp, L.i32, L.vp]
    hdr = open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()
    m = re.search(r"int sgd_attention_identity\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == len(args)
    assert int(re.search(r"#define SGD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION    # an additive entry
    assert os.path.exists(os.path.join(PKG, "csrc", "pag.hip"))


# ------------------------------------------------------------------------------------ the reference of the GPU tests

def _oracle_case(name, B=2):
    from sgdm_amd.synth import synth_batch, weights_from_seed
    entry = INDEX[name]
    cfg = cfg_from_index(entry)
    sd = weights_from_seed(entry["manifest"], entry["seed"])
    g = torch.Generator().manual_seed(31)
    x, t = torch.randn(B, 3, 16, 16, generator=g), torch.tensor([999, 3][:B])
    cond = synth_batch(cfg["condition_method"], B, 16, cfg["cond_dim"], entry["layout_dim"] or 0, seed=31)["cond"].float()
    return cfg, sd, x, t, cond


@pytest.mark.parametrize("name", ["uf_label_c32_s16", "uf_newattn_label_c32_s16"])
def test_patched_oracle_is_the_oracle_without_layers_and_differs_with_mid(name, monkeypatch):
    from oracle import unet_ref as U
    cfg, sd, x, t, cond = _oracle_case(name)
    B = x.shape[0]
    orig = U.attention_block
    with torch.no_grad():
        plain = U.unet_forward(cfg, sd, torch.cat((x, x)), torch.cat((t, t)), torch.cat((cond, cond)), None,
                               torch.zeros(2 * B, dtype=torch.bool))
    none = pag_forward(monkeypatch, cfg, sd, x, t, cond, None, ())
    assert U.attention_block is orig                                            # the patch is gone with its context
    assert torch.equal(none, plain)
    assert torch.equal(plain[:B], plain[B:])                                    # (0, 0) drop mask: two equal halves
    mid = pag_forward(monkeypatch, cfg, sd, x, t, cond, None, ("middle_block.1",))
    assert torch.equal(mid[:B], plain[:B])                                      # the conditional rows never see the patch
    diff = float((mid[B:] - plain[B:]).abs().max() / plain.abs().max())
    print(f"{name}: patched oracle, 'mid': perturbed half vs conditional half, max abs diff / max |ref| {diff:.2e}")
    assert diff > 1e-3
    from sgdm_amd.unet import attention_prefixes
    allp = pag_forward(monkeypatch, cfg, sd, x, t, cond, None, attention_prefixes(U.build_plan(cfg)))
    assert torch.equal(allp[:B], plain[:B]) and not torch.equal(allp[B:], mid[B:])
    # pag_drop_cond: the perturbed half under the (0, 1) mask is the patched forward of the unconditional rows
    drop = pag_forward(monkeypatch, cfg, sd, x, t, cond, None, ("middle_block.1",), drop_cond=True)
    assert torch.equal(drop[:B], plain[:B]) and not torch.equal(drop[B:], mid[B:])


def test_identity_map_is_what_the_patch_writes():
    """a = v is softmax == I: the oracle's own einsum with the attention weights forced to the identity gives the patch's rows"""
    from oracle import unet_ref as U
    cfg, sd, x, t, cond = _oracle_case("uf_label_c32_s16")
    p, heads = "middle_block.1", U.build_plan(cfg)[1][1][2]
    c = sd[p + ".qkv.weight"].shape[1]
    h = torch.randn(4, c, 4, 4, generator=torch.Generator().manual_seed(5))
    import torch.nn.functional as F
    with torch.no_grad():
        got = patched_attention(U, (p,), 2)(sd, p, h, heads)
        xf = h.reshape(4, c, -1)
        qkv = F.conv1d(U._gn(sd, p + ".norm", xf), sd[p + ".qkv.weight"], sd[p + ".qkv.bias"])
        q, k, v = qkv.reshape(4 * heads, c // heads * 3, 16).split(c // heads, dim=1)
        a = torch.einsum("bts,bcs->bct", torch.eye(16).expand(4 * heads, 16, 16), v).reshape(4, -1, 16)
        want = (xf + F.conv1d(a, sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"])).reshape(h.shape)
    assert torch.equal(got[2:], want[2:]) and torch.equal(got[:2], U.attention_block(sd, p, h, heads)[:2])
    assert float(sd[p + ".proj_out.weight"].abs().max()) > 0                    # the golden weights do project the attention


def test_combine_at_zero_weight_is_the_conditional_half():
    from test_hip_vpred import _guided32
    g = torch.Generator().manual_seed(3)
    out = torch.randn(4, 35, 3, generator=g)
    assert torch.equal(_guided32(out, 2, 0.0, 2), out[:2])                      # (1 + 0) c - 0 p, bit for bit
    w = torch.tensor(1.5)
    assert torch.equal(_guided32(out, 2, 1.5, 2), (1 + w) * out[:2] - w * out[2:])
