"""A channel-changing ResBlock's 1x1 skip conv folded into its 3x3 out conv (sgd_igemm_fused_aux): kernel-level parity through the
C ABI against float64 conv2d on the CPU, next to the unfused pair (sgd_igemm twice, as the training forward launches it), and the
launch program's two variants in whole models.  GPU only.

Bounds: those of the igemm kernel tests per mode (test_hip_kernels.PRECS: 2e-5 f16x3, 1e-4 bf16x3) on rel-L2 and max-abs error,
100 x that on the element-wise relative error of conftest.elem_rel (as test_hip_unet holds its outputs), for the fused launch AND
the pair; and the fused rel-L2 error at most twice the pair's in the same case -- both sit at the fp32 accumulation-order floor and
only the order of one sum differs."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import elem_rel, load_json, load_npz, max_rel, rel_l2

pytestmark = pytest.mark.gpu

TOL = {"f16x3": 2e-5, "bf16x3": 1e-4}
TOL_MODEL = {"f16x3": 5e-5, "bf16x3": 1e-4}            # test_hip_unet.TOL: whole-UNet outputs against the reference's


def _lib():
    from sgdm_amd import _lib as L
    return L, L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return C.c_void_p(t.data_ptr())


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _pack_scaled(ws_ks, prec):
    """the tensors of `ws_ks` = [(weight, ksize)] packed back to back with the scale of ONE amax over all of them"""
    L, lib = _lib()
    cout = ws_ks[0][0].shape[0]
    sizes = [int(lib.sgd_packed_weight_bytes(cout, w.shape[1], ks, prec)) for w, ks in ws_ks]
    buf = torch.empty(sum(sizes) // 4, device="cuda")
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")
    sinv = torch.ones(1, device="cuda")
    for w, _ in ws_ks:
        L.check(lib.sgd_weight_amax(_p(w), w.numel(), _p(amax), _st()), "amax")
    off, dims = 0, []
    for (w, ks), nb in zip(ws_ks, sizes):
        cp, op = C.c_int32(), C.c_int32()
        L.check(lib.sgd_pack_weight_scaled(_p(w), C.c_void_p(buf.data_ptr() + off), cout, w.shape[1], ks, prec, 0, _p(amax), _p(sinv),
                                           C.byref(cp), C.byref(op), _st()), "pack")
        dims.append((cp.value, op.value))
        off += nb
    return buf, sinv, dims, amax


class Case:
    """one ResBlock tail: y = conv3x3(silu(a h + b)) + conv1x1(cat(x0, x1)) + b3 + bs, seeded; the float64 reference is computed once"""

    def __init__(self, n, hw, cout, ac0, ac1, seed=0, skip_scale=1.0, zero_main=False, zero_skip=False):
        g = torch.Generator().manual_seed(100 + seed)
        self.n, self.hw, self.cout, self.ac0, self.ac1 = n, hw, cout, ac0, ac1
        self.h = torch.randn(n, cout, hw, hw, generator=g)
        self.x0 = torch.randn(n, ac0, hw, hw, generator=g)
        self.x1 = torch.randn(n, ac1, hw, hw, generator=g) if ac1 else None
        self.pa = 1 + 0.3 * torch.randn(n, cout, generator=g)
        self.pb = 0.3 * torch.randn(n, cout, generator=g)
        self.w3 = torch.randn(cout, cout, 3, 3, generator=g) / math.sqrt(9 * cout)
        self.w1 = torch.randn(cout, ac0 + ac1, 1, 1, generator=g) / math.sqrt(ac0 + ac1) * skip_scale
        self.b3, self.bs = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
        if zero_main:
            self.w3.zero_()
        if zero_skip:
            self.w1.zero_()
        d = torch.float64
        act = F.silu(self.h.to(d) * self.pa.to(d)[:, :, None, None] + self.pb.to(d)[:, :, None, None])
        xs = self.x0.to(d) if self.x1 is None else torch.cat([self.x0.to(d), self.x1.to(d)], 1)
        self.ref = F.conv2d(act, self.w3.to(d), self.b3.to(d), padding=1) + F.conv2d(xs, self.w1.to(d), self.bs.to(d))
        # device copies shared by every run of the case
        self.hd, self.x0d = _nhwc(self.h).cuda(), _nhwc(self.x0).cuda()
        self.x1d = _nhwc(self.x1).cuda() if ac1 else None
        self.pad, self.pbd = self.pa.cuda(), self.pb.cuda()
        self.w3d, self.w1d = self.w3.cuda(), self.w1.cuda()
        L, lib = _lib()
        self.work = torch.zeros(int(lib.sgd_igemm_work_bytes()) // 4, device="cuda")

    def conv_args(self, prec, y, tune, grid_cap, stats):
        L, lib = _lib()
        a = L.IgemmArgs()
        a.x0, a.c0 = self.hd.data_ptr(), self.cout
        a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride = L.MODE_CONV3, self.n, self.hw, self.hw, self.hw, self.hw, 1
        a.pro, a.pro_silu, a.pa, a.pb = L.PRO_AFFINE_NC, 1, self.pad.data_ptr(), self.pbd.data_ptr()
        a.y, a.cout, a.y_ld, a.prec = y.data_ptr(), self.cout, self.cout, prec
        a.tune, a.grid_cap = tune, grid_cap
        a.work, a.work_bytes = self.work.data_ptr(), self.work.numel() * 4
        if stats is not None:
            a.stats = stats.data_ptr()
        return a

    def aux(self):
        L, lib = _lib()
        return L.IgemmAux(x0=self.x0d.data_ptr(), x1=self.x1d.data_ptr() if self.x1d is not None else 0, c0=self.ac0, c1=self.ac1)

    def _out(self, prec, tune, grid_cap):
        L, lib = _lib()
        y = torch.full((self.n, self.hw, self.hw, self.cout), float("nan"), device="cuda")
        a = self.conv_args(prec, y, tune, grid_cap, None)
        parts = lib.sgd_igemm_stats_parts(C.byref(a))
        assert parts > 0
        st = torch.full((self.n, parts, 2, self.cout), float("nan"), device="cuda")
        a.stats = st.data_ptr()
        return y, st, a

    def run_fused(self, prec_name, tune, grid_cap=0):
        L, lib = _lib()
        prec = L.PREC_BY_NAME[prec_name]
        y, st, a = self._out(prec, tune, grid_cap)
        buf, sinv, dims, _ = _pack_scaled([(self.w3d, 3), (self.w1d.reshape(self.cout, -1), 1)], prec)
        bias = (self.b3 + self.bs).cuda()
        a.w, a.w_scale_inv, (a.cin_p, a.cout_p), a.bias = buf.data_ptr(), sinv.data_ptr(), dims[0], bias.data_ptr()
        xa = self.aux()
        assert lib.sgd_igemm_fused_aux_ok(C.byref(a), C.byref(xa)) == 1
        L.check(lib.sgd_igemm_fused_aux(C.byref(a), C.byref(xa), _st()), "fused")
        torch.cuda.synchronize()
        return y.cpu().permute(0, 3, 1, 2), st.cpu()

    def run_pair(self, prec_name, tune, grid_cap=0):
        """the skip conv into a tensor of its own, then the out conv with that tensor as its residual: what the parent launches"""
        L, lib = _lib()
        prec = L.PREC_BY_NAME[prec_name]
        rows = self.n * self.hw * self.hw
        skip = torch.full((self.n, self.hw, self.hw, self.cout), float("nan"), device="cuda")
        b1, s1, d1, _ = _pack_scaled([(self.w1d.reshape(self.cout, -1), 1)], prec)
        bsd, b3d = self.bs.cuda(), self.b3.cuda()
        q = L.IgemmArgs()
        q.x0, q.c0, q.c1 = self.x0d.data_ptr(), self.ac0, self.ac1
        q.x1 = self.x1d.data_ptr() if self.x1d is not None else 0
        q.mode, q.m, q.rows_per_n, q.stride = L.MODE_FLAT, rows, self.hw * self.hw, 1
        q.w, q.w_scale_inv, (q.cin_p, q.cout_p), q.bias = b1.data_ptr(), s1.data_ptr(), d1[0], bsd.data_ptr()
        q.y, q.cout, q.y_ld, q.prec, q.tune, q.grid_cap = skip.data_ptr(), self.cout, self.cout, prec, tune, grid_cap
        q.work, q.work_bytes = self.work.data_ptr(), self.work.numel() * 4
        L.check(lib.sgd_igemm(C.byref(q), _st()), "skip")
        y, st, a = self._out(prec, tune, grid_cap)
        b3p, s3, d3, _ = _pack_scaled([(self.w3d, 3)], prec)
        a.w, a.w_scale_inv, (a.cin_p, a.cout_p), a.bias = b3p.data_ptr(), s3.data_ptr(), d3[0], b3d.data_ptr()
        a.res, a.res_mode = skip.data_ptr(), L.RS_NONE
        L.check(lib.sgd_igemm(C.byref(a), _st()), "out conv")
        torch.cuda.synchronize()
        return y.cpu().permute(0, 3, 1, 2), st.cpu()


_CASES = {}


def case(*key, **kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _CASES:
        _CASES[k] = Case(*key, **kw)
    return _CASES[k]


def _check(c, prec, tune, grid_cap=0, label=""):
    tol = TOL[prec]
    yf, sf = c.run_fused(prec, tune, grid_cap)
    yu, su = c.run_pair(prec, tune, grid_cap)
    ef, eu = rel_l2(yf, c.ref), rel_l2(yu, c.ref)
    print(f"{label} {prec}: rel-L2 fused {ef:.3e} pair {eu:.3e}  max-rel fused {max_rel(yf, c.ref):.3e} pair {max_rel(yu, c.ref):.3e}  "
          f"elem-rel fused {elem_rel(yf, c.ref):.3e} pair {elem_rel(yu, c.ref):.3e}")
    assert torch.isfinite(yf).all() and torch.isfinite(sf).all()
    for y in (yf, yu):
        assert rel_l2(y, c.ref) < tol and max_rel(y, c.ref) < tol and elem_rel(y, c.ref) < 100 * tol
    assert ef <= 2 * eu, (ef, eu)
    # GroupNorm partial statistics (consumed by the next layer's gn()): the fused epilogue's against the pair's, slot by slot
    assert sf.shape == su.shape
    print(f"{label} {prec}: statistics rel-L2 fused vs pair {rel_l2(sf, su):.3e}")
    assert rel_l2(sf, su) < tol and max_rel(sf, su) < tol
    # ... and against the exact sums of the output the launch wrote
    yy = yf.double().permute(0, 2, 3, 1).reshape(c.n, -1, c.cout)
    exact = torch.stack([yy.sum(1), (yy * yy).sum(1)], 1)
    assert max_rel(sf.double().sum(1), exact) < 2e-6
    return yf, sf


# n, hw, cout, aux c0 | c1, grid_cap.  SGD_TUNE_NO_SMALL throughout: these launches have fewer 128-column tiles than the
# small-launch rule hands to the 32-column tile, which the fused instance (and its query) does not serve.
SHAPES = {
    # two spatial tiles per image, 4 main chunks, the concat seam on a chunk boundary, fewer aux chunks (3) than main chunks
    "two_tiles_64|32": (3, 16, 128, 64, 32, 0),
    "two_tiles_96|0": (3, 16, 128, 96, 0, 0),
    # 16 tiles x 16 main chunks on the whole device: the balanced tail splits (asserted below); 16 aux chunks
    "tail_256|256": (2, 16, 512, 256, 256, 0),
    # two tiles per block (10 tiles on a grid capped at 8): the aux -> next tile seam of both roles; 2 aux chunks (ring remainder)
    "seam_32|32": (5, 16, 128, 32, 32, 8),
    # ... and a single aux chunk
    "seam_32|0": (5, 16, 128, 32, 0, 8),
}


@pytest.mark.parametrize("prec", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fused_vs_float64_and_pair(name, prec):
    L, lib = _lib()
    n, hw, cout, ac0, ac1, cap = SHAPES[name]
    c = case(n, hw, cout, ac0, ac1)
    if name.startswith("tail"):
        cus = min(256, torch.cuda.get_device_properties(0).multi_processor_count & ~7)
        out = (C.c_int32 * (4 * cus))()
        assert lib.sgd_igemm_tail_layout(n * (hw * hw // 128) * (cout // 128), cout // 32, 9, cus, out) == 0
        assert any(out[4 * b] >= 2 for b in range(cus)), "this launch is meant to split its last round along K"
    y1, s1 = _check(c, prec, L.TUNE_NO_SMALL, cap, name)
    # two fused runs are bit-identical (the balanced tail adds its parts in a fixed order)
    y2, s2 = c.run_fused(prec, L.TUNE_NO_SMALL, cap)
    assert torch.equal(y1, y2) and torch.equal(s1, s2)
    if name.startswith("tail"):                       # the plain schedule computes the same tiles whole
        y3, _ = c.run_fused(prec, L.TUNE_NO_SMALL | L.TUNE_PLAIN_SCHEDULE, cap)
        assert rel_l2(y3, c.ref) < TOL[prec] and rel_l2(y3, y1) < 2e-6


@pytest.mark.parametrize("prec", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("variant", ["skip_2^-8", "skip_2^8", "main_zero", "both_zero"])
def test_shared_scale(variant, prec):
    """both weight tensors carry ONE power-of-two scale: a skip weight 2^8 smaller / larger than the main weight, and the
    zero_module initial state of out_layers.3 (all-zero main weights; all zero both: the output is the summed bias exactly)"""
    L, lib = _lib()
    kw = {"skip_2^-8": dict(skip_scale=2.0 ** -8), "skip_2^8": dict(skip_scale=2.0 ** 8), "main_zero": dict(zero_main=True),
          "both_zero": dict(zero_main=True, zero_skip=True)}[variant]
    c = case(3, 16, 128, 64, 32, seed=1, **kw)
    if variant == "both_zero":
        yf, sf = c.run_fused(prec, L.TUNE_NO_SMALL)
        assert torch.isfinite(yf).all() and torch.isfinite(sf).all()
        assert torch.equal(yf, (c.b3 + c.bs)[None, :, None, None].expand_as(yf))
        return
    _check(c, prec, L.TUNE_NO_SMALL, 0, variant)


def _query(prec="f16x3", n=3, hw=16, cout=128, ac0=64, ac1=32, drop_p=0.0, tune=None, res=0):
    L, lib = _lib()
    q = L.IgemmArgs()
    q.mode, q.n, q.hi, q.wi, q.ho, q.wo, q.stride = L.MODE_CONV3, n, hw, hw, hw, hw, 1
    q.c0, q.cout, q.y_ld, q.prec = cout, cout, cout, L.PREC_BY_NAME[prec]
    q.pro, q.pro_silu, q.drop_p, q.res = L.PRO_AFFINE_NC, 1, drop_p, res
    q.tune = L.TUNE_NO_SMALL if tune is None else tune
    xa = L.IgemmAux(c0=ac0, c1=ac1)
    return lib.sgd_igemm_fused_aux_ok(C.byref(q), C.byref(xa)), q, xa


def test_refusals():
    L, lib = _lib()
    assert _query()[0] == 1
    assert _query(hw=8)[0] == 0                        # two images per tile (g.nb > 1)
    assert _query(ac0=48, ac1=48)[0] == 0              # a source that is not whole 32-channel chunks
    assert _query(drop_p=0.1)[0] == 0
    assert _query(res=1)[0] == 0                       # a residual present
    for prec in ("f32", "f16", "bf16"):                # modes without the instance
        assert _query(prec=prec)[0] == 0
    assert _query(tune=0)[0] == 0                      # 6 tiles: the launcher would take the 32-column tile
    assert _query(cout=96, ac0=64, ac1=0)[0] == 0      # cout % 128
    # the launch refuses what the query refuses, before any launch, with no error state left behind
    ok, q, xa = _query(hw=8)
    assert lib.sgd_igemm_fused_aux(C.byref(q), C.byref(xa), _st()) == 1
    assert lib.sgd_igemm_fused_aux(None, None, _st()) == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ whole models
class AD(dict):
    __getattr__ = dict.__getitem__


INDEX = load_json("unet_index.json")


def _golden_model(name, prec):
    from sgdm_amd.synth import weights_from_seed
    from sgdm_amd.unet import UNetModel
    entry = INDEX[name]
    kw = dict(entry["ctor"])
    cond = AD(scale_type="imagen")
    if entry["layout_dim"]:
        cond[kw["condition_method"]] = AD(layout_dim=entry["layout_dim"])
    m = UNetModel(condition=cond, **kw)
    m.load_state_dict(weights_from_seed(entry["manifest"], entry["seed"]))
    m = m.cuda().eval()
    m.hip_precision = prec
    return m


def _golden_inputs(name):
    v = load_npz(f"unet_{name}.npz")
    cond = torch.from_numpy(v["cond"]).cuda() if "cond" in v else None
    layout = torch.from_numpy(v["layout"]).float().cuda() if "layout" in v else None
    return v, torch.from_numpy(v["x"]).cuda(), torch.from_numpy(v["t"]).cuda(), cond, layout


def _tags(eng, train):
    return [op[0] for op in eng.program(train).ops]


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("name", sorted(n for n in INDEX if n.startswith("uf_") and "c32_s16" in n))
def test_small_golden_models_either_setting(name, fuse, monkeypatch):
    """the ch=32 16x16 fixtures with SGDM_FUSE_SKIP 1 and 0: every ResBlock of these models is refused (64-channel outputs, maps
    below 128 pixels, the small-launch tile), so _res builds the pair in both variants and the outputs meet the fixture"""
    monkeypatch.setenv("SGDM_FUSE_SKIP", fuse)
    m = _golden_model(name, "f16x3")
    v, x, t, cond, layout = _golden_inputs(name)
    with torch.no_grad():
        eps = m(x, t, cond=cond, layout=layout, cond_drop_prob=torch.zeros(x.shape[0]).cuda())[0]
    assert max_rel(eps.cpu(), v["eps_keep"]) < TOL_MODEL["f16x3"] and rel_l2(eps.cpu(), v["eps_keep"]) < TOL_MODEL["f16x3"]
    eng = next(iter(m._engines.values()))
    assert not eng.fused_packs
    assert any(".skip_connection" in tg for tg in _tags(eng, False)) and _tags(eng, False) == _tags(eng, True)


@pytest.mark.parametrize("prec", ["f16x3", "bf16x3"])
def test_s64_golden_model_fused_and_pair(prec, monkeypatch):
    """ch=256 at 64x64, CFG evaluation (UNet batch 2): the three 64x64 decoder ResBlocks fuse; with SGDM_FUSE_SKIP 1 and 0 the
    guided output meets the fixture, and the fused program has no skip_connection launch for the fused blocks"""
    name = "uf_s64_c256"
    v, x, t, cond, layout = _golden_inputs(name)
    outs = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("SGDM_FUSE_SKIP", fuse)
        m = _golden_model(name, prec)
        with torch.no_grad():
            e = m.forward_with_cond_scale(x, t, cond_scale=2.0, cond=cond, layout=layout)
        err = (max_rel(e.cpu(), v["cfg_imagen_2.0"]), rel_l2(e.cpu(), v["cfg_imagen_2.0"]))
        print(f"SGDM_FUSE_SKIP={fuse} {prec}: max-rel {err[0]:.3e} rel-L2 {err[1]:.3e}")
        assert max(err) < TOL_MODEL[prec]
        eng = next(iter(m._engines.values()))
        outs[fuse] = (len(eng.fused_packs), _tags(eng, False), _tags(eng, True))
    nf, infer, train = outs["1"]
    assert nf == 3 and outs["0"][0] == 0
    fused = [tg[:-len(".skip_connection")] for tg in train if tg.endswith(".skip_connection") and tg not in infer]
    assert len(fused) == nf and all(b.startswith("output_blocks.") for b in fused)
    assert len(train) == len(infer) + nf and train == outs["0"][1] == outs["0"][2]
    for b in fused:                                     # one entry tagged out_layers.3 in place of the pair
        assert infer.count(b + ".out_layers.3") == 1 and train.count(b + ".out_layers.3") == 1


def _wide_model(dropout, image_size=16, prec="f16x3"):
    """128 -> 256 channels at 16 x 16 / 8 x 8: at UNet batch 40 the two 16 x 16 decoder ResBlocks (384 -> 128, 256 -> 128) fuse"""
    from sgdm_amd.synth import weights_from_seed
    from sgdm_amd.unet import UNetModel
    kw = dict(image_size=image_size, in_channels=3, out_channels=3, model_channels=128, num_res_blocks=1, channel_mult=[1, 2],
              attention_resolutions=[], num_heads=4, use_scale_shift_norm=True, resblock_updown=True, dropout=dropout,
              cond_dim=10, condition_method="label")
    m = UNetModel(condition=AD(scale_type="imagen"), **kw)
    m.load_state_dict(weights_from_seed([(k, tuple(p.shape)) for k, p in m.state_dict().items()], 5))
    m = m.cuda()
    m.hip_precision = prec
    return m


def _wide_batch(B=40, hw=16):
    g = torch.Generator().manual_seed(8)
    return (torch.randn(B, 3, hw, hw, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda(),
            F.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float().cuda())


def test_program_variants_and_training_step(monkeypatch):
    """fusion on: the inference program has no skip_connection launch for the fused blocks, the training program has the pair;
    the inference outputs of both settings agree to the kernel bound; a training step (dropout on: loss, every gradient) is bit-equal
    between SGDM_FUSE_SKIP 1 and 0, before and after inference evaluations on the same engine"""
    x, t, cond = _wide_batch()
    got = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("SGDM_FUSE_SKIP", fuse)
        m = _wide_model(0.1)
        m.eval()
        with torch.no_grad():
            e0 = m(x, t, cond=cond, cond_drop_prob=torch.zeros(40).cuda())[0]
        m.train()
        torch.manual_seed(11)                           # dropout seeds of the step
        eps = m(x, t, cond=cond, cond_drop_prob=torch.zeros(40).cuda())[0]
        loss = (eps - x).square().mean()
        loss.backward()
        grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        m.eval()
        with torch.no_grad():
            e1 = m(x, t, cond=cond, cond_drop_prob=torch.zeros(40).cuda())[0]
        assert torch.equal(e0, e1)                      # the inference variant is back, its packs unchanged
        eng = next(iter(m._engines.values()))
        got[fuse] = (e0.cpu(), float(loss), grads, len(eng.fused_packs), _tags(eng, False), _tags(eng, True))
    e_f, loss_f, g_f, nf, infer, train = got["1"]
    e_u, loss_u, g_u, nu, infer_u, train_u = got["0"]
    assert nf == 2 and nu == 0
    assert [tg for tg in train if tg not in infer] == ["output_blocks.2.0.skip_connection", "output_blocks.3.0.skip_connection"]
    assert train == train_u == infer_u
    print(f"inference output, fused vs pair: rel-L2 {rel_l2(e_f, e_u):.3e}")
    assert rel_l2(e_f, e_u) < TOL["f16x3"]
    assert loss_f == loss_u and g_f.keys() == g_u.keys() and len(g_f) > 20
    for k in g_f:
        assert torch.equal(g_f[k], g_u[k]), k


@pytest.mark.parametrize("why", ["f32", "f16", "8x8"])
def test_refused_blocks_build_the_pair(why):
    """the model whose 16 x 16 decoder blocks fuse in f16x3, in a mode without the instance and at 8 x 8 (two images per tile):
    sgd_igemm_fused_aux_ok says no for every block, _res builds the pair into both variants and no fused pack exists.  (The
    query's other refusals -- a source of 48 channels, drop_p > 0 -- cannot be reached through _res: channel counts of a plan are
    multiples of 32 where cout % 128 == 0, and the training forward, the only one with dropout, always launches the pair.)"""
    hw = 8 if why == "8x8" else 16
    m = _wide_model(0.0, image_size=hw, prec="f16x3" if why == "8x8" else why)
    m.eval()
    x, t, cond = _wide_batch(40, hw)
    with torch.no_grad():
        e = m(x, t, cond=cond, cond_drop_prob=torch.zeros(40).cuda())[0]
    assert torch.isfinite(e).all()
    eng = next(iter(m._engines.values()))
    assert not eng.fused_packs and not eng.train_bufs
    infer, train = _tags(eng, False), _tags(eng, True)
    assert infer == train and all(w is None for w in eng.prog.when)
    for b in ("output_blocks.2.0", "output_blocks.3.0"):
        assert infer.count(b + ".skip_connection") == 1 and infer.count(b + ".out_layers.3") == 1
        q = eng._fuse_skip_ok(128, (40, hw, hw, hw, hw, 1, 0), 256 if b.endswith("2.0") else 128, 128)
        assert q is False


def test_fused_pack_follows_weight_updates(monkeypatch):
    """the fused pack (3x3 + 1x1 weights under one scale, summed bias) is refreshed in front of inference evaluations only: after
    in-place weight updates -- with a training forward, which does not refresh it, in between -- the next inference evaluation
    must use the new weights: compared with the same sequence under SGDM_FUSE_SKIP=0"""
    x, t, cond = _wide_batch()
    z = torch.zeros(40).cuda()
    outs = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("SGDM_FUSE_SKIP", fuse)
        m = _wide_model(0.0)
        m.eval()
        seq = []
        with torch.no_grad():
            seq.append(m(x, t, cond=cond, cond_drop_prob=z)[0].cpu())
            for p in m.parameters():
                p.mul_(1.03125)                          # every weight AND bias of the fused blocks changes, versions bumped
            seq.append(m(x, t, cond=cond, cond_drop_prob=z)[0].cpu())
        m.train()
        m(x, t, cond=cond, cond_drop_prob=z)[0].square().mean().backward()       # training forward: the pair's packs only
        m.eval()
        with torch.no_grad():
            for n_, p in m.named_parameters():
                if "skip_connection" in n_ or "out_layers.3" in n_:
                    p.mul_(0.75)                         # ... then only the fused blocks' own tensors change
            seq.append(m(x, t, cond=cond, cond_drop_prob=z)[0].cpu())
        eng = next(iter(m._engines.values()))
        assert len(eng.fused_packs) == (2 if fuse == "1" else 0)
        outs[fuse] = seq
    for i, (f, u) in enumerate(zip(outs["1"], outs["0"])):
        print(f"evaluation {i}: fused vs pair rel-L2 {rel_l2(f, u):.3e}")
        assert rel_l2(f, u) < TOL["f16x3"]
    assert rel_l2(outs["1"][1], outs["1"][0]) > 1e-3 and rel_l2(outs["1"][2], outs["1"][1]) > 1e-3


def test_captured_step_equals_eager_small_golden_model():
    """the captured sampling step (hipGraph) against the eager one, bit for bit: the ch=32 16x16 golden model at batch 4"""
    _captured_equals_eager(_golden_model("uf_label_c32_s16", "f16x3"), 4, 10, expect_fused=False)


def test_captured_step_equals_eager_fused():
    """... and on a model whose program holds fused launches (UNet batch 40)"""
    m = _wide_model(0.0)
    m.eval()
    _captured_equals_eager(m, 20, 10, expect_fused=True)


def _captured_equals_eager(m, B, ncls, expect_fused):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 3, 16, 16, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    cond = F.one_hot(torch.randint(0, ncls, (B,), generator=g), ncls).float().cuda()
    with torch.no_grad():
        eager = m.forward_with_cond_scale(x, t, cond_scale=2.0, cond=cond).clone()
        eng = next(iter(m._engines.values()))
        assert bool(eng.fused_packs) == expect_fused
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                eng.launch(torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().wait_stream(side)
        ref = eng.eps_nhwc.clone()
        eng.eps_nhwc.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(eng.eps_nhwc, ref)
        again = m.forward_with_cond_scale(x, t, cond_scale=2.0, cond=cond)
        assert torch.equal(again, eager)
