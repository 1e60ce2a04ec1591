"""Training step of the drop-in denoisers: backward program + autograd glue.

The reference gets its backward from torch.autograd through the UNet (PL calls ``loss.backward()``,
lightning_module.py:215-245; AttentionBlock recomputes its forward under a custom checkpoint,
openaimodel.py:359-362, util.py:119-148).  Here the backward is a second static launch program
walking the forward tape in reverse:

  * input gradients of every conv / linear = the FORWARD implicit-GEMM kernel on adjoint-packed weights
    (``sgd_pack_weight_dgrad``), in the model's arithmetic mode;
  * weight gradients = ``sgd_wgrad`` (exact-fp32 MFMA, the activated input recomputed by the same fused
    prologue as the forward: nothing but the raw feature maps is kept) + ``sgd_wgrad_reduce`` into the
    reference OIHW layout;
  * GroupNorm(+FiLM)+SiLU backward = ``sgd_gn_bwd_reduce/coef/apply`` (resample adjoints of the up/down
    ResBlocks and the identity-skip gradient folded into the apply pass);
  * attention backward = ``sgd_attention_bwd`` with the forward's log-sum-exp (no score matrix stored).

The tape holds ONE record per forward GEMM (``unet._Layer``: descriptor, pack, parameter names, bias padding) and the walk
derives both adjoints from it: ``gemm_geometry`` reads (cout, cin, taps, rows), the input-gradient geometry and the strided
adjoint's zero-upsampling off the descriptor; ``Backward.dx(layer, gy, dst)`` is the input gradient, ``Backward.dw(layer, gy)``
the weight / bias gradient, zero-padded operators (padded attention heads) included.  The per-kind methods (``_res``, ``_attn``,
...) are the chain rule of their block in those two calls; only the FiLM projection calls ``dgrad`` / ``wgrad`` itself.

The losses whose ``backward()`` starts this program -- q_sample, the fused loss kernels, ``p_losses_hip`` -- are ``losses.py``;
``distill_teacher_from`` is re-exported here, the name the documentation and the error messages give it, and so are the
names callers took from this module before the move.  ``progressive_next_stage`` (progressive distillation: the student becomes
the next teacher, the step count is halved) lives here, next to the name it builds the teacher with.

``loss.backward()`` works because the UNet evaluation is a ``torch.autograd.Function`` whose inputs are the
trainable parameters; it returns one gradient tensor per parameter in the reference layout.
Both operators are covered: ``unet_fast`` and ``unetca_fast`` (LayerNorm, multi-query attention with context / null
keys, strided-conv Downsample and nearest+conv Upsample adjoints).

One engine (workspace + tape) exists per (UNet batch, H, W, precision), so the activations a backward reads are those of
the LAST forward on that engine: ``_UNetTrainFn.backward`` checks a forward-generation counter and raises if another
forward ran in between (two losses on one model need two backward-before-next-forward passes, as here, or two batches
of different size).
"""
import collections
import ctypes as C
import math
import os

import torch

from . import _lib as L
from .losses import distill_teacher_from  # noqa: F401  (sgdm_amd.train.distill_teacher_from: INTEGRATION.md)
# the names callers took from this module while the loss code lived here keep resolving; new code imports them from losses.py
from .losses import (_LOSS_KIND, _LOSS_PAR, _MSEFn, _lv_tables, lv_decoder_bits, lv_kl_bits, lv_loss, lv_terms,  # noqa: F401
                     lv_vlb_torch, p_losses_hip, refuse_inference_only, simple_loss_torch as _simple_torch)
from .packs import Derived, PackBatch, Packed, _ptr
from .unet import GN_EPS, GN_GROUPS, _Program, grad_health


def progressive_next_stage(diff, ema=None, hip_precision=None):
    """the next stage of progressive distillation (hparam progressive_steps = K; Salimans & Ho 2022, Algorithm 2): a frozen
    copy of the current student (``distill_teacher_from``: the drop-in UNet behind ``diff.denoise_fn``, its EMA shadows when
    ``ema`` is given, optionally another arithmetic mode) becomes the teacher and K is halved.  The new teacher is a distilled
    model already, so ``distill_guidance`` / ``distill_rescale`` are cleared (each of its evaluations is ONE conditional one)
    and ``guidance_distilled`` is set; the cached row table and teacher runner are dropped.  Returns the new K.  ValueError,
    nothing changed: progressive_steps is off or 1, or num_timesteps % (2 * (K // 2)) != 0 (the next teacher's midpoints would
    fall between timesteps)."""
    K, T = getattr(diff, "progressive", None), diff.hparams.num_timesteps
    if K is None:
        raise ValueError("progressive_next_stage: progressive_steps is not set")
    if K == 1:
        raise ValueError("progressive_next_stage: progressive_steps is 1, there is no stage after a one-step student")
    if K % 2 != 0 or T % K != 0:
        raise ValueError(f"progressive_next_stage: progressive_steps={K} cannot be halved: num_timesteps % (2 * (K / 2)) == 0 "
                         f"with an integer K / 2 is needed (num_timesteps is {T})")
    student = getattr(diff.denoise_fn, "__self__", diff.denoise_fn)
    teacher = distill_teacher_from(student, ema=ema, hip_precision=hip_precision)
    h = diff.hparams
    h.progressive_steps, h.distill_guidance, h.distill_rescale, h.guidance_distilled = K // 2, None, None, True
    diff.progressive, diff.distill = K // 2, None
    diff.__dict__.pop("_pd_rows", None)
    diff.set_distill_teacher(teacher)                   # (drops the teacher runner)
    return K // 2


def wgrad_ksplit(taps, cout, cin, rows):
    """K split of a weight-gradient launch (sgd_wgrad's grid = co tiles x ci tiles x ksplit).  3x3 convs run as ONE
    512-thread block per CU (csrc/backward.hip: wgrad_conv_ws_kernel, 32 input channels per block): the split is chosen
    so that the grid is as close as possible to a whole number of rounds of the 256 CUs with at least ~8 K tiles per
    block; 1x1 / linear launches (256-thread blocks, two per CU, 128 input channels per block) keep the round-2 rule."""
    ktiles = (rows + 63) // 64
    # stem / head (csrc/backward.hip, wgrad_impl: wgrad_narrow_kernel): 3 / 4 channels on one side and, on the other, a
    # whole number of waves of lanes that divides (or equals) the 256-thread block -- the SAME predicate as the launcher's
    # (`lanes_co` / `lanes_ci`); other widths (the ch = 224 plans) fall through to the generic kernels and their rules
    lanes = lambda c: c % 64 == 0 and (c == 256 or (c < 256 and 256 % c == 0))
    if taps == 9 and ((3 <= cin <= 4 and lanes(cout)) or (cout == 3 and lanes(cin))):
        # HBM-bound row walks, one 256-thread block per slab in chunks of 128 rows -- two blocks per CU at bs 80 (~640
        # rows each)
        return max(1, min(ktiles, 1024, -(-rows // 640)))
    if taps == 9:
        per_k = ((cout + 127) // 128) * ((cin + 31) // 32)
        best, best_cost = 1, None
        for ks in range(1, min(ktiles, 512) + 1):
            grid = per_k * ks
            rounds = -(-grid // 256)
            tiles = -(-ktiles // ks)
            cost = rounds * (tiles + 3.0)              # + ~3 tile periods of prologue / slab store per block
            if tiles >= 4 and (best_cost is None or cost < best_cost - 1e-9):
                best, best_cost = ks, cost
        return best
    base = taps * ((cout + 127) // 128) * ((cin + 127) // 128)
    return max(1, min(ktiles, 1024 // base))


GemmGeometry = collections.namedtuple("GemmGeometry", "cout cin taps rows conv zero_up")


def gemm_geometry(a):
    """what the adjoints of one forward GEMM need, read off its descriptor (an IgemmArgs): the GEMM's (cout, cin, taps, rows);
    conv: the geometry (n, h, w) of the input-gradient launch, None for a flat (1x1 / linear) launch; zero_up: the adjoint of a
    strided conv reads gy zero-upsampled x2.  A stride-1 conv with a resample in its loader (RS_AVGPOOL2, RS_UP2) runs its
    input gradient at the OUTPUT resolution, like any other: the resample's adjoint is the caller's (gn_bwd's gu_mode,
    sgd_resample_bwd)."""
    if a.mode == L.MODE_FLAT:
        return GemmGeometry(a.cout, a.c0 + a.c1, 1, a.m, None, False)
    return GemmGeometry(a.cout, a.c0 + a.c1, 9, a.n * a.ho * a.wo, (a.n, a.ho, a.wo), a.stride == 2)


def _tag(layer):
    """program tag of a layer's launches: the name of its (one) weight parameter less the ".weight" suffix"""
    wname, = layer.wnames
    return wname[:-len(".weight")]


class Backward:
    """backward launch program of one engine (unet_fast)"""

    def __init__(self, eng, arena=None, reducer=None):
        """arena / reducer (sgdm_amd.ddp): parameter gradients are views of one flat buffer cut into buckets and
        each bucket's all-reduce is enqueued on a side stream as soon as the launches filling it are issued."""
        self.e, self.lib, self.n, self.dev, self.prec = eng, eng.lib, eng.n, eng.dev, eng.prec
        self.m = eng.m
        if self.prec in (L.PREC_F16, L.PREC_BF16):
            raise ValueError("hip_precision 'f16' / 'bf16' is inference only: no backward program exists for a single-product engine")
        self.prog = _Program()
        self.packs, self.late, self.late_at = [], [], []
        self.arena, self.reducer = arena, reducer
        self.world = reducer.world if reducer is not None else 1
        # Gradients run through the program multiplied by a power of two so that the split-f16 operands of the
        # dgrad launches stay in fp16's normal range (d loss / d eps ~ 1/(B*C*H*W) would land in the subnormals
        # and lose the lo part); every parameter-gradient reduction multiplies by 1/scale again.  Exact in fp32.
        numel = eng.n * self.m.out_channels * eng.h * eng.w
        self.gscale = float(2 ** int(math.ceil(math.log2(max(2, numel)))))
        self.unscale = 1.0 / (self.gscale * self.world)      # + the 1/world of the gradient average (SUM all-reduce)
        self.G = {}                      # activation data_ptr -> [grad tensor, written?]
        self.pgrad = {}                  # parameter name -> gradient tensor (reference shape)
        self.keep = []
        self.CW = 256                    # row chunks of the two-stage column sums
        self.cwork = torch.empty(self.CW, 8192, dtype=torch.float32, device=self.dev)
        self.wscratch_bytes, self._wscratch_buf = 0, None      # pre-split operand planes of the 3x3 weight gradients (wgrad)
        self._pack_batch = self._flag = self._windows = None
        self._build()

    # ---------------------------------------------------------------- helpers
    def attention_bwd_fn(self, d):
        """the attention backward in the engine's arithmetic: split-precision MFMA for f16x3 at head widths up to 64 (the
        forward's choice, unet._Engine.attention_fn), exact fp32 otherwise -- 128-wide heads (config/dynamic/unet_fast_s64.yaml:
        1024 channels / 8 heads) included"""
        if self.prec == L.PREC_F16X3 and d <= 64 and os.environ.get("SGDM_ATTN_BWD_SPLIT", "1") != "0":
            return self.lib.sgd_attention_bwd_split
        return self.lib.sgd_attention_bwd

    def buf(self, *shape):
        t = torch.empty(*shape, dtype=torch.float32, device=self.dev)
        self.keep.append(t)
        return t

    def gact(self, t):
        """(grad buffer of activation tensor t, accumulate flag for the next writer)"""
        ent = self.G.get(t.data_ptr())
        if ent is None:
            ent = [self.buf(*t.shape), False]
            self.G[t.data_ptr()] = ent
        acc = ent[1]
        ent[1] = True
        return ent[0], int(acc)

    def gread(self, t):
        ent = self.G[t.data_ptr()]
        assert ent[1], "gradient read before any producer wrote it"
        return ent[0]

    def pg(self, name):
        if name not in self.pgrad:
            self.pgrad[name] = self.arena.grad(name) if self.arena is not None else self.buf(*self.m.P(name).shape)
        return self.pgrad[name]

    def wrote(self, name):
        """program point right after the launch that completes parameter `name`: overlapped bucket send"""
        if self.reducer is None or not self.reducer.active:
            return
        bi = self.arena.bucket_of[name]
        # (the last bucket is flushed by reducer.finish(), after the step's health flag has been written into its tail slot)
        if self.arena.buckets[bi][2] == name and bi != len(self.arena.buckets) - 1:
            red = self.reducer

            def bucket_ready(stream, bi=bi):
                red.bucket_ready(bi)
                return 0
            self.prog.add(f"bucket{bi}.allreduce", bucket_ready)

    def dgrad(self, tag, gy, cin_of_gy, y, cout_of_y, deps, src_fn, cout_fwd, cin_fwd, ksize, conv=None, m=0,
              y_ld=None, zero_up=False, acc=False, pad=None, donor=None):
        """y (+)= adjoint(W) applied to gy (gy has cout_fwd channels, y gets cin_fwd channels).  W [cout_fwd, cin_fwd(, k, k)]:
        the parameters `deps` (zero-padded: pad), or what src_fn returns of them; donor: packs.Packed.
        zero_up: adjoint of a stride-2 conv (gy is zero-upsampled x2 inside the loader); acc: add into y."""
        # the head (a conv with 3 / 4 OUTPUT channels): its input gradient is the stem's kernel on the flipped, transposed
        # parameter (csrc/narrow.hip, adjoint mode) -- fp32 FMA straight from the weight, no adjoint pack
        if (conv is not None and ksize == 3 and not zero_up and not acc and cin_of_gy in (3, 4) and cout_fwd == cin_of_gy
                and cout_of_y % 4 == 0 and cout_of_y <= 1024 and len(deps) == 1 and deps[0].dtype == torch.float32
                and deps[0].is_contiguous() and gy.shape[-1] == cin_of_gy and os.environ.get("SGDM_NARROW_CONV", "1") != "0"):
            nimg, hh, ww = conv
            wsrc, fn, gy_p, y_p, ld = deps[0], self.lib.sgd_conv3_narrow_in, C.c_void_p(gy.data_ptr()), C.c_void_p(y.data_ptr()), y_ld or cout_of_y

            def sgd_conv3_narrow_in(stream):          # (the parameter's address is read at launch time)
                return fn(gy_p, C.c_void_p(wsrc.data_ptr()), C.c_void_p(0), y_p, C.c_void_p(0), nimg, hh, ww, cin_of_gy, cout_of_y,
                          ld, 1, stream)
            self.prog.add(tag, sgd_conv3_narrow_in, flops=2.0 * nimg * hh * ww * cout_of_y * 9 * cin_of_gy)
            return
        pk = Packed(deps, ksize, self.prec, L.PACK_DGRAD, pad, src_fn, (cout_fwd, cin_fwd), donor, self.dev)
        self.packs.append(pk)
        a = L.IgemmArgs()
        a.x0, a.c0 = gy.data_ptr(), cin_of_gy
        if conv is not None:
            nimg, hh, ww = conv                    # dims of gy
            if zero_up:
                a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride, a.resample = (L.MODE_CONV3, nimg, hh, ww, 2 * hh, 2 * ww, 1,
                                                                          L.RS_ZEROUP2)
            else:
                a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride = L.MODE_CONV3, nimg, hh, ww, hh, ww, 1
        else:
            a.mode, a.m, a.stride = L.MODE_FLAT, m, 1
        a.w, a.cin_p, a.cout_p = pk.buf.data_ptr(), pk.cin_p, pk.cout_p
        a.w_scale_inv = pk.scale_ptr
        a.y, a.cout, a.y_ld, a.prec = y.data_ptr(), cout_of_y, (y_ld or cout_of_y), self.prec
        if acc:
            a.res, a.res_mode = y.data_ptr(), L.RS_NONE
        if self.e.work_bytes:                # the forward engine's balanced-tail scratch (same stream: launches are ordered)
            a.work, a.work_bytes = self.e.work.data_ptr(), self.e.work_bytes
        a.grid_cap = getattr(self.e, "_grid_cap", 0)
        self.late_at.append(len(self.prog.ops))          # program position of this launch (reserve windows)
        self.late.append((a, pk))
        self.keep.append(a)
        rows = (a.n * a.ho * a.wo) if conv is not None else m
        self.prog.add(tag, self.lib.sgd_igemm, C.byref(a), flops=2.0 * rows * cout_of_y * (9 if conv is not None else 1) * cin_of_gy)

    def wgrad(self, tag, fwd_args, gy, gy_ld, cout, cin, taps, rows, wname, bias_name=None, dw_view=None):
        ksplit = wgrad_ksplit(taps, cout, cin, rows)
        slabs = self.buf(ksplit, taps, cout, cin)
        xt = os.environ.get("SGDM_WGRAD_TUNE")      # A/B switch of tools/profile_train_layers.py: "<SGD_TUNE_WGRAD_* bits>[:max cin*cout]"
        if xt and taps == 9 and cin * cout <= int((xt.split(":") + ["1000000000"])[1]):
            fwd_args.tune |= int(xt.split(":")[0])
        # 3x3 convs: operands pre-split once into 16-bit planes (scratch shared by every launch of the program, grown to
        # the largest request before the first run: sgd_wgrad_scratch)
        need = int(self.lib.sgd_wgrad_scratch_bytes(C.byref(fwd_args), cout)) if taps == 9 else 0
        self.wscratch_bytes = max(self.wscratch_bytes, need)
        # the bias gradient (column sums of gy) comes out of the same launch: the kernel (or its pre-pass) stages the gy
        # rows anyway; as many partial rows as that launch writes
        brows = int(self.lib.sgd_wgrad_bias_rows(C.byref(fwd_args), cout, gy_ld, ksplit, need)) if bias_name is not None else 0
        bslab = self.buf(brows, cout) if bias_name is not None else None
        box = self

        def wgrad_launch(stream, fwd_args=fwd_args, gy=gy, slabs=slabs, bslab=bslab):
            ws = box._wscratch()
            return box.lib.sgd_wgrad_scratch(C.byref(fwd_args), _ptr(gy), gy_ld, cout, _ptr(slabs), ksplit,
                                             _ptr(bslab) if bslab is not None else None, _ptr(ws), ws.numel() * 4, stream)
        wgrad_launch.__name__ = "sgd_wgrad"
        self.prog.add(tag + ".wgrad", wgrad_launch, flops=2.0 * rows * cout * cin * taps)
        dw = dw_view if dw_view is not None else self.pg(wname)
        if bias_name is not None:
            # weight and bias gradient of the layer folded by one launch
            self.prog.add(tag + ".wred", self.lib.sgd_wgrad_reduce_bias, _ptr(slabs), ksplit, taps, cout, cin, _ptr(dw), 0,
                          self.unscale, _ptr(bslab), brows, _ptr(self.pg(bias_name)))
        else:
            self.prog.add(tag + ".wred", self.lib.sgd_wgrad_reduce, _ptr(slabs), ksplit, taps, cout, cin, _ptr(dw), 0,
                          self.unscale)
        if dw_view is None:
            self.wrote(wname)
        if bias_name is not None:
            self.wrote(bias_name)

    def _wscratch(self):
        if self._wscratch_buf is None or self._wscratch_buf.numel() * 4 < self.wscratch_bytes:
            self._wscratch_buf = torch.empty(max(4, self.wscratch_bytes) // 4 + 4, dtype=torch.float32, device=self.dev)
        return self._wscratch_buf

    # The two adjoints of one forward GEMM, derived from its record (unet._Layer): geometry from the descriptor
    # (gemm_geometry), the weight and its zero-padded re-layout from the pack, the parameter names from the record.  Tags are
    # the weight's name without ".weight".  Two calls, not one: the call sites' order is the program order and the
    # first-use order of pg(name) -- the order of the DDP arena's slots and buckets.
    def dx(self, layer, gy, dst, acc=False, tag=None):
        """dst (+)= the gradient of the layer's input, from the gradient gy of its output"""
        g, pk = gemm_geometry(layer.a), layer.pk
        assert len(pk.srcs) == 1
        self.dgrad(tag or _tag(layer) + ".dgrad", gy, g.cout, dst, g.cin, pk.srcs, None, g.cout, g.cin,
                   pk.ksize, conv=g.conv, m=0 if g.conv else g.rows, zero_up=g.zero_up, acc=acc, pad=pk.pad, donor=pk)

    def dw(self, layer, gy):
        """the layer's weight (and bias) gradient.  A zero-padded operator (packs._Pad; the descriptor's widths are the PADDED
        ones): the padded gradient is gathered back into the parameter's own shape -- the padding rows / columns receive
        gradients that belong to no parameter -- and the bias gradient is the column sums of gy, gathered like the weight's
        rows where the bias is padded too."""
        g, pad = gemm_geometry(layer.a), layer.pk.pad
        (wname,), tag = layer.wnames, _tag(layer)
        if pad is None:
            return self.wgrad(tag, layer.a, gy, g.cout, g.cout, g.cin, g.taps, g.rows, wname, layer.bias)
        tmp = self.buf(g.cout, g.cin)
        self.wgrad(tag, layer.a, gy, g.cout, g.cout, g.cin, g.taps, g.rows, wname, dw_view=tmp)
        self.gather_op(tag + ".unpad", wname, tmp, pad)
        if layer.bias is None:
            return
        if layer.bias_pad is None:
            return self.colsum(tag + ".bias", _ptr(gy), g.rows, g.cout, g.cout, layer.bias)
        tb = self.buf(1, g.cout)
        self.prog.add(tag + ".bias", self.lib.sgd_colsum, _ptr(gy), g.rows, g.cout, g.cout, _ptr(tb), 0, self.unscale,
                      _ptr(self.cwork), self.CW)
        self.gather_op(tag + ".bias.unpad", layer.bias, tb, layer.bias_pad)

    def colsum(self, tag, g_ptr, rows, c, ld, pname):
        self.prog.add(tag, self.lib.sgd_colsum, g_ptr, rows, c, ld, _ptr(self.pg(pname)), 0, self.unscale,
                      _ptr(self.cwork), self.CW)
        self.wrote(pname)

    def ln_bwd(self, tag, x, g, rows, c, gamma_name, dst, acc, beta_name=None, gres=None):
        """LayerNorm backward: dst (+)= dx (+ gres); dgamma (and dbeta when the norm has a trainable bias)"""
        gxh = self.buf(rows, c)
        self.prog.add(tag, self.lib.sgd_ln_bwd, _ptr(x), _ptr(g), _ptr(self.m.P(gamma_name)), rows, c, 1e-5, _ptr(dst),
                      int(acc), _ptr(gxh), _ptr(gres) if gres is not None else None)
        self.colsum(tag + ".dgamma", _ptr(gxh), rows, c, c, gamma_name)
        if beta_name is not None:
            self.colsum(tag + ".dbeta", _ptr(g), rows, c, c, beta_name)

    def gather_op(self, tag, pname, padded, pad):
        """parameter gradient <- the entries of a zero-padded gradient that belong to the parameter (packs._Pad.gather)"""
        dst = self.pg(pname)

        def op(stream):
            dst.copy_(pad.gather(padded.reshape(-1, padded.shape[-1])).reshape(dst.shape))
            return 0
        self.prog.add(tag, op)
        self.wrote(pname)

    def copy_op(self, tag, dst, src_view):
        def op(stream):
            dst.copy_(src_view)
            return 0
        self.prog.add(tag, op)

    def gn_bwd(self, tag, srcs, hw, a, b, sums, gname, silu, gu, gu_ld, gu_mode, gres, gres_ld, gres_mode,
               film_ptr=0, film_ld=0, dfilm_ptr=0, drop=(0.0, 0)):
        """GroupNorm(+FiLM)[+SiLU] backward over a (virtual concat of) source tensor(s); writes/accumulates the
        input gradients into the sources' gradient buffers."""
        n, lib = self.n, self.lib
        h, w = hw
        ct = sum(c for _, c in srcs)
        # Row-stream reduce (round 6, csrc/backward.hip): same-resolution gradient, every source a power-of-two channel count whose
        # image (>= 32 x 32) is a whole number of 32 KiB windows.  It writes per-chunk partial sums (one table for all sources:
        # the smallest of their chunk counts) that the coefficient launch folds itself.
        rows_ok = gu_mode == L.RS_NONE and os.environ.get("SGDM_GN_BWD_ROWS", "1") != "0"
        ks = [int(lib.sgd_gn_bwd_rows_chunks(n, h, w, c)) for _, c in srcs] if rows_ok else [0]
        chunks = min(ks) if min(ks) > 0 and all(k % min(ks) == 0 for k in ks) else 0
        S = self.buf(n, max(1, chunks), ct, 2)
        off = 0
        for t, c in srcs:
            if chunks:
                self.prog.add(tag + ".reduce", lib.sgd_gn_bwd_reduce_rows, _ptr(t), n, h, w, c, ct, off, _ptr(a), _ptr(b), silu,
                              _ptr(gu), gu_ld, drop[0], drop[1], chunks, _ptr(S), nbytes=8.0 * n * h * w * c)
            else:
                self.prog.add(tag + ".reduce", lib.sgd_gn_bwd_reduce, _ptr(t), n, h, w, c, ct, off, _ptr(a), _ptr(b), silu,
                              _ptr(gu), gu_ld, gu_mode, drop[0], drop[1], _ptr(S), nbytes=8.0 * n * h * w * c)
            off += c
        sch = max(1, chunks)
        A, B, Cc = (self.buf(n, ct) for _ in range(3))
        gamma, beta = self.m.P(gname + ".weight"), self.m.P(gname + ".bias")
        # (the launcher's bound: dynamic table + the kernel's 2 KB of static reduction scratch inside the 64 KB default limit)
        fused = (n <= 256 and (16 if chunks else 8) * n * (ct // GN_GROUPS) + 32 * n + 4 + 2048 <= 64 * 1024
                 and os.environ.get("SGDM_GN_BWD_FOLD", "1") != "0")
        coef = (_ptr(S), sch, _ptr(sums), _ptr(gamma), _ptr(beta), C.c_void_p(film_ptr), film_ld, n, ct, GN_GROUPS, h * w,
                GN_EPS, _ptr(A), _ptr(B), _ptr(Cc))
        dgamma, dbeta, dfilm = _ptr(self.pg(gname + ".weight")), _ptr(self.pg(gname + ".bias")), C.c_void_p(dfilm_ptr)
        dg, db = (None, None) if fused else (self.buf(n, ct), self.buf(n, ct))       # per-sample tables of the unfused forms
        if fused:                # coefficients + dgamma / dbeta column sums in ONE launch (bit-identical to the two below)
            self.prog.add(tag + ".coef", lib.sgd_gn_bwd_coef_fold, *coef, dfilm, dgamma, dbeta, 0, self.unscale)
        elif n <= 256:           # dgamma and dbeta from the per-sample tables in one launch
            self.prog.add(tag + ".coef", lib.sgd_gn_bwd_coef, *coef, _ptr(dg), _ptr(db), dfilm)
            self.prog.add(tag + ".dgamma_dbeta", lib.sgd_colsum_pair, _ptr(dg), _ptr(db), n, ct, ct, dgamma, dbeta, 0,
                          self.unscale)
        else:
            self.prog.add(tag + ".coef", lib.sgd_gn_bwd_coef, *coef, _ptr(dg), _ptr(db), dfilm)
            self.prog.add(tag + ".dgamma", lib.sgd_colsum, _ptr(dg), n, ct, ct, dgamma, 0, self.unscale, _ptr(self.cwork),
                          self.CW)
            self.prog.add(tag + ".dbeta", lib.sgd_colsum, _ptr(db), n, ct, ct, dbeta, 0, self.unscale, _ptr(self.cwork),
                          self.CW)
        self.wrote(gname + ".weight")
        self.wrote(gname + ".bias")
        off = 0
        for t, c in srcs:
            dst, acc = self.gact(t)
            nb = 4.0 * n * h * w * c * (3 + (1 if gres is not None else 0) + (1 if acc else 0))
            self.prog.add(tag + ".apply", lib.sgd_gn_bwd_apply, _ptr(t), n, h, w, c, ct, off, _ptr(a), _ptr(b), silu,
                          _ptr(gu), gu_ld, gu_mode, drop[0], drop[1], _ptr(A), _ptr(B), _ptr(Cc),
                          _ptr(gres) if gres is not None else None,
                          gres_ld, gres_mode, _ptr(dst), c, 0, acc, nbytes=nb)
            off += c

    # ---------------------------------------------------------------- program
    def _build(self):
        e, n = self.e, self.n
        self.geps = self.buf(*e.eps_nhwc.shape)           # filled by the autograd Function before the program runs
        film_rec = [r for r in e.tape if r["kind"] == "film"][0]
        self.gfilm = self.buf(n, film_rec["film_w"])
        self._film_plan(film_rec)
        for rec in reversed(e.tape):
            step = getattr(self, "_" + rec["kind"], None)
            if step is None:
                raise NotImplementedError(rec["kind"])
            step(rec)

    def _conv_in(self, rec):
        """the stem: its input is the image, no gradient wanted"""
        self.dw(rec["a"], self.gread(rec["y"]))

    def _linear(self, rec):
        """to_cond_tokens.0: its input is the guidance, no gradient wanted"""
        self.dw(rec["a"], self.gread(rec["y"]))

    def _head(self, rec):
        x = rec["x"]
        n, h, w, c = x.shape
        gu = self.buf(n, h, w, c)
        self.dx(rec["conv"], self.geps, gu)
        self.dw(rec["conv"], self.geps)
        self.gn_bwd("out.0", [(x, c)], (h, w), rec["a"], rec["b"], rec["sums"], "out.0", 1, gu, c, L.RS_NONE, None, 0, 0)

    def _res(self, rec):
        p, e = rec["p"], self.e
        (hh, ww), rs = rec["hw_in"], rec["rs"]
        n, ho, wo, cout = rec["h1"].shape
        cin = sum(c for _, c in rec["srcs"])
        gy = self.gread(rec["y"])
        # conv2 (out_layers.3)
        gu2 = self.buf(n, ho, wo, cout)
        self.dx(rec["conv2"], gy, gu2)
        self.dw(rec["conv2"], gy)
        # GN2 + FiLM + SiLU -> gradient of h1 and of this block's FiLM slice
        self.G[rec["h1"].data_ptr()] = [self.buf(*rec["h1"].shape), False]
        if rec["ss"]:
            self.gn_bwd(p + ".out_layers.0", [(rec["h1"], cout)], (ho, wo), rec["a2"], rec["b2"], rec["sums2"],
                        p + ".out_layers.0", 1, gu2, cout, L.RS_NONE, None, 0, 0,
                        film_ptr=e.film.data_ptr() + 4 * rec["film_off"], film_ld=e.film_ld,
                        dfilm_ptr=self.gfilm.data_ptr() + 4 * rec["film_off"], drop=(rec["drop_p"], rec["drop_seed"]))
            gh1 = self.gread(rec["h1"])
        else:
            # additive embedding (openaimodel.py:317-319): h1 holds h + emb_out; the gradient of emb_out[n, c] is the pixel sum of
            # the gradient of h1 -- the (sum, .) column of a statistics pass over it -- and lands in this block's slice of the
            # embedding-projection gradient like the FiLM form's (dscale, dshift)
            self.gn_bwd(p + ".out_layers.0", [(rec["h1"], cout)], (ho, wo), rec["a2"], rec["b2"], rec["sums2"],
                        p + ".out_layers.0", 1, gu2, cout, L.RS_NONE, None, 0, 0, drop=(rec["drop_p"], rec["drop_seed"]))
            gh1 = self.gread(rec["h1"])
            st = self.buf(n, cout, 2)
            self.prog.add(p + ".emb_add.bwd", self.lib.sgd_chan_stats, _ptr(gh1), n, ho * wo, cout, _ptr(st), cout, 0)
            self.copy_op(p + ".emb_add.gfilm", self.gfilm[:, rec["film_off"]:rec["film_off"] + cout], st[:, :, 0])
        self._film_group_done(p)
        # conv1 (in_layers.2): its input gradient at the OUTPUT resolution, the resample's adjoint in GN1's backward below
        gu1 = self.buf(n, ho, wo, cin)
        self.dx(rec["conv1"], gh1, gu1)
        self.dw(rec["conv1"], gh1)
        # skip path
        if rec["skip"] is not None:
            gsk = self.buf(n, hh, ww, cin)
            self.dx(rec["skip"], gy, gsk, tag=p + ".skip.dgrad")
            self.dw(rec["skip"], gy)
            gres, gres_ld, gres_mode = gsk, cin, L.RS_NONE
        else:
            gres, gres_ld, gres_mode = gy, cout, rs            # identity skip through the same resample
        # GN1 + SiLU (+ resample adjoint of the activated tensor) -> gradients of the block inputs
        self.gn_bwd(p + ".in_layers.0", rec["srcs"], (hh, ww), rec["a1"], rec["b1"], rec["sums1"], p + ".in_layers.0",
                    1, gu1, cin, rs, gres, gres_ld, gres_mode)

    def _attn(self, rec):
        """AttentionBlock backward (autograd of openaimodel.py:365-371, 403-420 / 427-451); with zero-padded heads (dp > d) every
        tensor between qkv and proj_out is dp wide per head, as in _attn_lr"""
        n, p, ch, heads, d, dp, T = self.n, rec["p"], rec["ch"], rec["heads"], rec["d"], rec["dp"], rec["T"]
        inner = heads * dp
        gy = self.gread(rec["y"])
        gatt = self.buf(n, T, inner)
        self.dx(rec["proj_args"], gy, gatt)
        self.dw(rec["proj_args"], gy)
        qkv, gqkv = rec["qkv"], self.buf(n, T, 3 * inner)
        dvec = self.buf(n, heads, T)
        off = lambda t, k: C.c_void_p(t.data_ptr() + 4 * k)
        hs, ko, vo = rec["qkv_layout"]                     # head stride, k / v offsets: legacy or new attention order
        self.prog.add(p + ".attn_bwd", self.attention_bwd_fn(dp), _ptr(qkv), 3 * inner, hs, off(qkv, ko), off(qkv, vo),
                      3 * inner, hs, _ptr(rec["att"]), inner, _ptr(gatt), inner, _ptr(rec["lse"]), _ptr(dvec), n, heads, T, T,
                      dp, 1.0 / math.sqrt(d), _ptr(gqkv), off(gqkv, ko), off(gqkv, vo))
        gxn = self.buf(n, T, ch)
        self.dx(rec["qkv_args"], gqkv, gxn)
        self.dw(rec["qkv_args"], gqkv)
        self.gn_bwd(p + ".norm", [(rec["x"], ch)], rec["hw"], rec["a"], rec["b"], rec["sums"], p + ".norm", 0, gxn, ch,
                    L.RS_NONE, gy, ch, L.RS_NONE)                       # residual: x + proj(...)

    def _down(self, rec):
        """Downsample = conv3x3 stride 2 (openaimodel_ca.py:167-174)"""
        gy = self.gread(rec["y"])
        dst, acc = self.gact(rec["x"])
        self.dx(rec["a"], gy, dst, acc=bool(acc))
        self.dw(rec["a"], gy)

    def _up(self, rec):
        """Upsample = nearest x2 + conv3x3 (openaimodel_ca.py:128-131)"""
        n, hh, ww, c = rec["x"].shape
        gy = self.gread(rec["y"])
        gu = self.buf(n, 2 * hh, 2 * ww, c)
        self.dx(rec["a"], gy, gu)
        dst, acc = self.gact(rec["x"])
        self.prog.add(rec["p"] + ".up_adj", self.lib.sgd_resample_bwd, _ptr(gu), n, hh, ww, c, L.RS_UP2, _ptr(dst), acc)
        self.dw(rec["a"], gy)

    def _attn_lr(self, rec):
        """Attention_LR backward (autograd of crossattetion_lr.py:81-142).  With zero-padded heads (dp > d: head widths the
        attention core has no instance for) every tensor between the projections is dp wide per head; dx / dw build the
        adjoint operators from the padded weights and gather each padded weight gradient back into the parameter's shape."""
        n, p, ch, heads, d, dp, T, J, ntok = (self.n, rec["p"], rec["ch"], rec["heads"], rec["d"], rec["dp"], rec["T"],
                                              rec["J"], rec["ntok"])
        x, gy = rec["x"], self.gread(rec["y"])
        rows = n * T
        inner = heads * dp
        # y = x + LN_out(o):  LN_out backward (gamma trainable, beta is a buffer)
        go = self.buf(n, T, ch)
        self.ln_bwd(p + ".to_out.1", rec["o"], gy, rows, ch, p + ".to_out.1.gamma", go, 0)
        gatt = self.buf(n, T, inner)
        self.dx(rec["aout"], go, gatt)
        self.dw(rec["aout"], go)
        # multi-query attention core
        q, kv = rec["q"], rec["kv"]
        gq, gkv = self.buf(n, T, inner), self.buf(n, J, 2 * dp)
        dvec = self.buf(n, heads, T)
        self.prog.add(p + ".attn_bwd", self.attention_bwd_fn(dp), _ptr(q), inner, dp, _ptr(kv),
                      C.c_void_p(kv.data_ptr() + 4 * dp), 2 * dp, 0, _ptr(rec["att"]), inner, _ptr(gatt), inner,
                      _ptr(rec["lse"]), _ptr(dvec), n, heads, T, J, dp, d ** -0.5, _ptr(gq), _ptr(gkv),
                      C.c_void_p(gkv.data_ptr() + 4 * dp))
        # to_q / to_kv share LN(x): gradient of the normalised input is the sum of both adjoints
        gxn = self.buf(n, T, ch)
        self.dx(rec["aq"], gq, gxn)
        self.dw(rec["aq"], gq)
        gkv_self = self.buf(n, T, 2 * dp)
        self.copy_op(p + ".gkv_self", gkv_self, gkv[:, ntok + 1:, :])
        self.dx(rec["akv"], gkv_self, gxn, acc=True)
        self.dw(rec["akv"], gkv_self)
        # null key/value: summed over the batch
        gnull = C.c_void_p(gkv.data_ptr() + 4 * ntok * 2 * dp)
        if rec["null_pad"] is None:
            self.colsum(p + ".null_kv", gnull, n, 2 * dp, J * 2 * dp, p + ".null_kv")
        else:
            tn = self.buf(2, dp)
            self.prog.add(p + ".null_kv", self.lib.sgd_colsum, gnull, n, 2 * dp, J * 2 * dp, _ptr(tn), 0, self.unscale,
                          _ptr(self.cwork), self.CW)
            self.gather_op(p + ".null_kv.unpad", p + ".null_kv", tn, rec["null_pad"])
        # context keys/values -> to_context.1 (Linear) -> to_context.0 (LayerNorm) -> shared context tokens
        context = rec["context"]
        ctx = context.shape[-1]
        gckv = self.buf(n, ntok, 2 * dp)
        self.copy_op(p + ".gkv_ctx", gckv, gkv[:, :ntok, :])
        self.dw(rec["actx"], gckv)
        gcn = self.buf(n, ntok, ctx)
        self.dx(rec["actx"], gckv, gcn)
        cdst, cacc = self.gact(context)
        self.ln_bwd(p + ".to_context.0", context, gcn, n * ntok, ctx, p + ".to_context.0.weight", cdst, cacc,
                    beta_name=p + ".to_context.0.bias")
        # input LayerNorm (gamma trainable, beta buffer) + the residual path
        dst, acc = self.gact(x)
        self.ln_bwd(p + ".norm", x, gxn, rows, ch, p + ".norm.gamma", dst, acc, gres=gy)

    def _norm_cond(self, rec):
        """context = LayerNorm(cat(time tokens, cond tokens)) (openaimodel_ca.py:973,1017)"""
        n, ntok, ctx, wt = self.n, rec["ntok"], rec["ctx"], rec["wt"]
        gctx = self.gread(rec["context"])
        graw = self.buf(n, ntok, ctx)
        self.ln_bwd("norm_cond", rec["raw"], gctx, n * ntok, ctx, "norm_cond.weight", graw, 0, beta_name="norm_cond.bias")
        g2 = graw.view(n, ntok * ctx)
        gt = self.buf(n, wt)
        self.copy_op("norm_cond.split_t", gt, g2[:, :wt])
        self.G[rec["raw_t"].data_ptr()] = [gt, True]
        if rec["raw_c"] is not None:
            gc = self.buf(n, ntok * ctx - wt)
            self.copy_op("norm_cond.split_c", gc, g2[:, wt:])
            self.G[rec["raw_c"].data_ptr()] = [gc, True]

    def _film(self, rec):
        """emb_layers of all ResBlocks (one GEMM forward): weight/bias grads split back per block; gradient of
        SiLU(emb) through the adjoint, then through the SiLU, into the (virtual concat) emb parts."""
        n, m = self.n, self.m
        fw = rec["film_w"]
        ted = rec["emb_t"].shape[1]
        cc = rec["emb_c"].shape[1] if rec["emb_c"] is not None else 0
        ech = ted + cc
        names = rec["names"]
        wparams = [m.P(p + ".emb_layers.1.weight") for p in names]
        # (the weight / bias gradients of the FiLM projections were produced stage by stage inside the walk: _film_group_done)
        assert not self._film_open, self._film_open
        cat = lambda: torch.cat([w.detach() for w in wparams], 0)
        parts = [(rec["emb_t"], 0, ted)] + ([(rec["emb_c"], ted, cc)] if cc else [])
        # few rows (the batch), a very long reduction (all FiLM outputs, 13,824 at C2): split-K on the concatenated weight as
        # stored -- the conv kernel walked it with 4 tiles (0.75 ms per step); the concatenation follows the parameters
        skinny = n <= 256 and fw >= 2048 and os.environ.get("SGDM_SKINNY_DGRAD", "1") != "0"
        if skinny:
            wcat = self.buf(fw, ech)

            def refresh_wcat(stream, wcat=wcat):
                torch.cat([w.detach().float() for w in wparams], 0, out=wcat)
            self.prog.add("emb_layers.wcat", Derived(wparams, refresh_wcat))
            # y[n, ech] = sum_k gfilm[n, k] wcat[k, ech] IS a weight gradient seen from the other side: "rows" = the fw FiLM
            # outputs, "gy" = gfilm transposed (fw x n), "a" = wcat.  The split 1x1 weight-gradient kernel (MFMA, split K over
            # the rows) replaces the fp32-FMA sgd_linear_splitk_t (LDS-bound: 0.25 ms per step at C2 for 1.7 GFLOP)
            gfT, gall = self.buf(fw, n), self.buf(n, ech)
            self.copy_op("emb_layers.gfilm_t", gfT, self.gfilm.view(n, fw).t())
            wa = L.IgemmArgs()
            wa.x0, wa.c0, wa.mode, wa.m, wa.stride, wa.prec = wcat.data_ptr(), ech, L.MODE_FLAT, fw, 1, self.prec
            self.keep.append(wa)
            ksplit = max(1, min((fw + 63) // 64 // 4, 512 // ((ech + 127) // 128)))
            slabs = self.buf(ksplit, 1, n, ech)
            lib = self.lib

            def sgd_wgrad(stream):
                ws = self._wscratch()
                return lib.sgd_wgrad_scratch(C.byref(wa), _ptr(gfT), n, n, _ptr(slabs), ksplit, None, _ptr(ws), ws.numel() * 4,
                                             stream)
            self.prog.add("emb_layers.dgrad", sgd_wgrad, flops=2.0 * n * ech * fw)
            self.prog.add("emb_layers.dgrad.fold", lib.sgd_wgrad_reduce, _ptr(slabs), ksplit, 1, n, ech, _ptr(gall), 0, 1.0)
        for t, o, c in parts:
            gact = self.buf(n, c)
            if skinny:
                self.copy_op(f"emb_layers.dgrad.part{o}", gact, gall[:, o:o + c])
            else:
                self.dgrad(f"emb_layers.dgrad{o}", self.gfilm, fw, gact, c, wparams, lambda o=o, c=c: cat()[:, o:o + c], fw, c,
                           1, m=n)
            g = self.buf(n, c)
            self.prog.add(f"emb.silu_bwd{o}", self.lib.sgd_silu_bwd, _ptr(t), _ptr(gact), n * c, _ptr(g))
            self.G[t.data_ptr()] = [g, True]

    # FiLM projections (emb_layers of all ResBlocks: ONE GEMM in the forward, its 42 MB of weight gradients the largest single
    # tensor group of the model).  As one launch at the end of the walk -- its gradient rows are complete only when the LAST
    # ResBlock's GroupNorm backward has written its slice -- it was the last gradient of the backward: on 8 GPUs the part of the
    # exchange nothing hides (round 5: bucket 4 + tail, ~80 MB, complete 0.4 ms before the end).  The walk visits the
    # ResBlocks in reverse forward order and a block's slice of the FiLM gradient is final after its out_layers.0 backward,
    # so the columns are cut into STAGES of consecutive blocks (>= FILM_STAGE_BYTES of weight gradient each) and every
    # stage's weight / bias gradient is launched as soon as its first (in forward order) block is through.
    FILM_STAGE_BYTES = 6 << 20

    def _film_plan(self, rec):
        names, couts = rec["names"], rec["couts"]
        fw = rec["film_w"]
        ech = rec["emb_t"].shape[1] + (rec["emb_c"].shape[1] if rec["emb_c"] is not None else 0)
        offs, off = [], 0
        fm = self.m._film_mult                     # 2: FiLM (scale, shift); 1: additive embedding (use_scale_shift_norm=False)
        for co in couts:
            offs.append(off)
            off += fm * co
        self._film_ctx = dict(rec=rec, ech=ech, fw=fw, dwcat=self.buf(fw, ech), dbcat=self.buf(fw))
        # stages in WALK order (last ResBlock of the forward first); a stage closes at block i when it holds enough bytes
        self._film_close = {}                       # block name -> (first block index, one past the last) of the stage it closes
        hi = len(names)
        acc = 0
        for i in range(len(names) - 1, -1, -1):
            acc += fm * couts[i] * ech * 4
            if acc >= self.FILM_STAGE_BYTES or i == 0:
                self._film_close[names[i]] = (i, hi)
                hi, acc = i, 0
        self._film_offs = offs + [fw]
        self._film_open = set(self._film_close)

    def _film_group_done(self, p):
        """called from the walk right after ResBlock `p`'s out_layers.0 backward has written its FiLM-gradient slice"""
        grp = self._film_close.get(p)
        if grp is None:
            return
        self._film_open.discard(p)
        i0, i1 = grp
        f, n = self._film_ctx, self.n
        rec, ech, fw, dwcat, dbcat = f["rec"], f["ech"], f["fw"], f["dwcat"], f["dbcat"]
        names, couts = rec["names"], rec["couts"]
        c0, c1 = self._film_offs[i0], self._film_offs[i1]
        tag = f"emb_layers.s{i0}"
        gsl = self.gfilm[:, c0:c1]                  # columns of this stage (row stride fw)
        dw_dst, db_dst = dwcat[c0:c1], dbcat[c0:c1]
        if self.arena is None:
            # single process: the per-block gradients ARE row slices of the concatenated result (contiguous), no copies.
            # (first-use order = the arena's order in a data-parallel build: the stage's weights, then its biases)
            for i in range(i0, i1):
                self.pgrad[names[i] + ".emb_layers.1.weight"] = dwcat[self._film_offs[i]:self._film_offs[i + 1]]
            for i in range(i0, i1):
                self.pgrad[names[i] + ".emb_layers.1.bias"] = dbcat[self._film_offs[i]:self._film_offs[i + 1]]
        else:
            # data parallel: the stage's weights, then its biases, take CONSECUTIVE arena slots (first-use order; every slot a
            # whole number of quads), so the stage's rows of the concatenated gradient ARE one arena range each: the reduce and
            # the column sums write there directly (round 6: 44 device-side slice copies per step fewer)
            wv = [self.pg(names[i] + ".emb_layers.1.weight") for i in range(i0, i1)]
            bv = [self.pg(names[i] + ".emb_layers.1.bias") for i in range(i0, i1)]
            flat = self.arena.flat

            def span(views, rows, cols):
                o0 = (views[0].data_ptr() - flat.data_ptr()) // flat.element_size()
                t = flat[o0:o0 + rows * cols].view(rows, cols) if cols > 1 else flat[o0:o0 + rows]
                off = 0
                for v in views:                     # consecutive, unpadded: each view starts where the one before it ended
                    assert v.data_ptr() == t.data_ptr() + off * flat.element_size(), "FiLM stage is not one arena range"
                    off += v.numel()
                return t
            dw_dst, db_dst = span(wv, c1 - c0, ech), span(bv, c1 - c0, 1)
        self.wgrad(tag, rec["a"].a, gsl, fw, c1 - c0, ech, 1, n, None, None, dw_view=dw_dst)
        self.prog.add(tag + ".bias", self.lib.sgd_colsum, _ptr(gsl), n, c1 - c0, fw, _ptr(db_dst), 0, self.unscale,
                      _ptr(self.cwork), self.CW)
        for i in range(i1 - 1, i0 - 1, -1):
            self.wrote(names[i] + ".emb_layers.1.weight")
            self.wrote(names[i] + ".emb_layers.1.bias")

    def _mlp2(self, rec):
        """Linear -> SiLU -> Linear (time_embed / mlp_cond / to_time_tokens / cond_mlp); the first layer's input is no activation"""
        gy = self.gread(rec["y"])
        n, mid = rec["h"].shape
        self.dw(rec["a2"], gy)
        gh_act = self.buf(n, mid)
        self.dx(rec["a2"], gy, gh_act)
        gh = self.buf(n, mid)
        self.prog.add(rec["name"] + ".silu_bwd", self.lib.sgd_silu_bwd, _ptr(rec["h"]), _ptr(gh_act), n * mid, _ptr(gh))
        self.dw(rec["a0"], gh)

    def _mlp_chain(self, rec):
        """to_cond_tokens_2d (openaimodel_ca.py:606-614): Linear -> SiLU -> Linear -> SiLU -> Linear -> SiLU -> Linear over
        the n*T token rows; every SiLU was the next GEMM's prologue, so each layer's input tensor is pre-activation"""
        g = self.gread(rec["y"])                          # [n, T*ctx] == [n*T, ctx] rows of the last layer's output
        for li, (x, layer) in reversed(list(enumerate(rec["layers"]))):
            self.dw(layer, g)
            if li == 0:
                break                                      # the layer input is the guidance itself: no gradient wanted
            gact, gpre = self.buf(*x.shape), self.buf(*x.shape)
            self.dx(layer, g, gact)
            self.prog.add(_tag(layer) + ".silu_bwd", self.lib.sgd_silu_bwd, _ptr(x), _ptr(gact), x.numel(), _ptr(gpre))
            g = gpre

    # ---------------------------------------------------------------- execution
    def run(self, geps_nchw):
        lib = self.lib
        stream = torch.cuda.current_stream().cuda_stream
        if self._pack_batch is None or len(self._pack_batch.packs) != len(self.packs):
            self._pack_batch = PackBatch(self.packs, self.prec, self.dev)
        self._pack_batch.refresh(stream)
        n, c = self.n, self.m.out_channels
        h, w = self.e.h, self.e.w
        g = (geps_nchw.float() * self.gscale).contiguous()
        L.check(lib.sgd_pack_input(_ptr(g), None, None, None, n, n, c, 0, h, w, _ptr(self.geps), stream), "geps")
        if self.reducer is not None:
            self.reducer.start()
        self.prog.run(stream)
        # Health of this step's gradients: 1.0 iff the engine's balanced-tail health word is up.  With an arena
        # the flag is the arena's last slot and travels with the LAST bucket (SUM over the ranks: every rank sees > 0 when any
        # rank failed); it is added to the device's sticky gate, which the fused optimizer takes as skip_if_nonzero -- a
        # poisoned step is never applied -- and copied to pinned host memory for the next step's poll_health() to raise on.
        word, flag = self.e.health_word(), None
        if word is not None:
            flag = self.arena.health if self.arena is not None else self._own_flag()
            flag.copy_(word.ne(0))
        if self.reducer is not None:
            self.reducer.backward_done()     # (overlap record: everything the exchange could hide behind is issued)
            self.reducer.finish()            # flush the tail bucket (it holds the flag), join the side stream
        if flag is not None:
            grad_health(self.dev).add_(flag)
        self.e.note_health(flag)
        return self.pgrad

    # ---- CU reserve only while a collective is in flight.  The persistent conv grid leaves
    # `reserve` compute units to RCCL's kernels on the side stream (tests/test_hip_contention.py: a launch whose blocks do
    # not all fit next to them takes up to 1.7x).  Taken from every launch of the backward the reserve cost ~1.1 ms of a
    # 63 ms step; RCCL needs it only between a bucket's enqueue and its completion.  The host knows where in the PROGRAM each
    # collective starts (the bucket hooks) and how many bytes it moves: a launch keeps the whole device unless it falls into
    # the window [hook, hook + bytes / RESERVE_GBPS + 0.2 ms) of estimated launch time (algorithmic flops at 300 TF/s, 40 us
    # for the memory-bound launches in between).  RESERVE_GBPS = 50 GB/s of all-reduced bytes (SGDM_RESERVE_GBPS) is about
    # half of what an 8-GPU xGMI ring delivers on 16 channels: a 64 MB bucket holds its window for 1.5 ms.  A STATIC rule on
    # purpose: windows sized by measured completion times would make the grid of a launch -- and with it the K split of its
    # balanced tail, i.e. the rounding of its sums -- depend on timing; this way a given program always runs the same grids.
    RESERVE_GBPS = 50.0

    def apply_grid_cap(self):
        cap = getattr(self.e, "_grid_cap", 0)
        if cap <= 0 or self.reducer is None or not self.reducer.active or os.environ.get("SGDM_RESERVE_WINDOWS", "1") == "0":
            for a, _ in self.late:
                a.grid_cap = cap
            self._windows = None
            return
        gbps = float(os.environ.get("SGDM_RESERVE_GBPS", self.RESERVE_GBPS))
        esz = self.arena.flat.element_size()
        hooks = [(i, int(op[0][len("bucket"):].split(".")[0])) for i, op in enumerate(self.prog.ops)
                 if op[0].startswith("bucket") and op[0].endswith(".allreduce")]
        est = [(mt[1] / 300e12 * 1e3 if mt[1] > 0 else 0.04) for mt in self.prog.meta]       # ms per program entry
        inside = [False] * len(self.prog.ops)
        for pos, bi in hooks:
            s0, e0, _ = self.arena.buckets[bi]
            budget = (e0 - s0) * esz / (gbps * 1e9) * 1e3 + 0.2
            j = pos
            while j < len(inside) and budget > 0:
                inside[j] = True
                budget -= est[j]
                j += 1
        for (a, _), at in zip(self.late, self.late_at):
            a.grid_cap = cap if inside[at] else 0
        self._windows = (sum(inside), len(inside))

    def _own_flag(self):
        if self._flag is None:
            self._flag = torch.zeros(1, dtype=torch.float32, device=self.dev)
        return self._flag


class _UNetTrainFn(torch.autograd.Function):
    """eps = UNet(x, t, ...) with gradients for the trainable parameters"""

    @staticmethod
    def forward(ctx, model, eng, args, *params):
        x, t, cond, layout, mask = args
        eng.run(x, t, cond, layout, mask, train=True)
        eng.generation = getattr(eng, "generation", 0) + 1
        ctx.model, ctx.eng, ctx.generation = model, eng, eng.generation
        ctx.names = [n for n, p in model.named_parameters() if p.requires_grad]
        ctx.params = params
        return model._to_nchw(eng)

    @staticmethod
    def backward(ctx, geps):
        eng = ctx.eng
        if eng.generation != ctx.generation:
            raise RuntimeError("sgdm_amd: backward through a stale forward -- another training forward ran on this "
                               "model (same batch/resolution) after the one being differentiated and overwrote its "
                               "activations; call backward() before the next forward")
        model = ctx.model
        _check_torch_ddp(model)
        if getattr(eng, "backward", None) is None:
            eng.backward = make_backward(eng)
            eng.backward.apply_grid_cap()        # the CU reserve of a data-parallel step, inside its windows only
        # The program writes every parameter gradient into a persistent buffer (a view of the DDP arena when there is one).
        # Handing those to autograd made AccumulateGrad clone each of them -- ~390 device copies per step (it cannot steal a
        # tensor somebody else still references).  A parameter whose .grad is None gets the buffer itself as .grad (what
        # DDP's gradient_as_bucket_view does); one whose .grad already IS the buffer from an earlier backward (zero_grad(
        # set_to_none=False), gradient accumulation) is un-aliased first, so accumulation keeps torch's semantics.
        held = eng.backward.pgrad
        for name, p in zip(ctx.names, ctx.params):
            g = held.get(name)
            if g is not None and p.grad is not None and p.grad.data_ptr() == g.data_ptr():
                p.grad = p.grad.clone()
        grads = eng.backward.run(geps)
        out = []
        with torch.no_grad():
            for name, p in zip(ctx.names, ctx.params):
                g = grads.get(name)          # None: parameter not on the path (e.g. to_cond_tokens_2d, README.md:90-94)
                # alias fast path only when nobody observes the gradient through autograd: tensor hooks / post-accumulate
                # hooks (gradient clipping callbacks, optimizer-in-backward, torch DDP's reducer) need AccumulateGrad to run
                alias = getattr(model, "hip_grad_alias", True) and not p._backward_hooks \
                    and not getattr(p, "_post_accumulate_grad_hooks", None)
                if g is not None and alias and p.grad is None and g.shape == p.shape:
                    p.grad = g
                    g = None
                out.append(g)
        return (None, None, None) + tuple(out)


def _check_torch_ddp(model):
    """once per model: the reference's own multi-GPU command wraps the LightningModule in torch DDP
    (pl.trainer.strategy=ddp): then torch's reducer owns the exchange -- this path must hand it the gradients through
    autograd (its hooks sit on the AccumulateGrad nodes) and must NOT all-reduce them a second time, nor broadcast the
    parameters the wrapper's constructor has already broadcast"""
    if getattr(model, "_torch_ddp_checked", False):
        return
    from .ddp import find_torch_ddp_wrapper, torch_ddp_ignores
    model._torch_ddp_checked = True
    wrapper = find_torch_ddp_wrapper(model)
    if wrapper is not None and not torch_ddp_ignores(wrapper, model):
        import warnings
        model.hip_ddp = False
        model.hip_grad_alias = False
        warnings.warn("sgdm_amd: the model is wrapped in torch DistributedDataParallel -- gradients are handed to "
                      "torch's reducer (one all-reduce, torch's buckets) and the HIP path's own overlapped RCCL "
                      "exchange is off.  For the native exchange run one process per GPU WITHOUT the wrapper "
                      "(sgdm_amd.pl_strategy.HipDDPStrategy) or call sgdm_amd.ddp.exclude_from_torch_ddp(root, "
                      "unet, ema) before wrapping (INTEGRATION.md).")


def make_backward(eng):
    """single process: plain gradient buffers.  torch.distributed initialised with world > 1: a dry build learns the
    order in which the backward produces the parameter gradients, then the real program writes them into a flat
    arena in that order and overlaps the bucketed RCCL all-reduce with the remaining launches."""
    from .ddp import BucketReducer, GradArena, exchange_active, exchange_forced, exchange_group
    if not exchange_active(eng.m):
        return Backward(eng)
    dry = Backward(eng)
    order = [(name, tuple(g.shape)) for name, g in dry.pgrad.items()]
    del dry
    arena = GradArena(order, eng.dev, bucket_bytes=getattr(eng.m, "hip_bucket_bytes", 64 << 20))
    # RCCL: a communicator of the exchange's own, capped at the CU reserve (collective over all ranks: every rank builds
    # its backward program at its first training step)
    return Backward(eng, arena, BucketReducer(arena, group=exchange_group(), average=False, force=exchange_forced(eng.m)))


def forward_train(model, x, t, cond, layout, mask, n):
    """autograd-capable UNet evaluation (called from UNetModelBase._run when grads are required)"""
    refuse_inference_only(model)
    B, cx, H, W = x.shape
    if getattr(model, "use_spatial_transformer", False):
        # the reference cannot train this variant either: BasicTransformerBlock checkpoints _forward(x, context) with
        # context=None (openaimodel.py:915, attention.py:213-214) and CheckpointFunction.backward calls None.detach()
        # (diffusionmodules/util.py:132 -> AttributeError); tests/golden/make_golden_train_tokens.py documents the run
        raise NotImplementedError("training through the SpatialTransformer path is not built: the reference raises "
                                  "AttributeError in its backward for this variant (checkpoint with context=None)")
    prec = L.PREC_BY_NAME[model.hip_precision]
    if not getattr(model, "_hip_ddp_synced", False) and getattr(model, "hip_ddp", True):
        # torch DDP broadcasts rank 0's parameters and buffers when it wraps a module; nothing else on this path would, and
        # replicas that start from different weights (rank-dependent init, a missing seed_everything, per-rank
        # checkpoints) would train silently diverged: once per model, before its first exchanged training step.  Every
        # rank enters its first training forward together (it is a collective).  Under torch's own wrapper
        # (strategy=ddp unchanged) the wrapper's constructor has done this already: look for it FIRST.  A LitEma built
        # before this point holds the old values: sync the root module early instead -- HipDDPStrategy and bench.py do;
        # this late call warns on a rank whose values it had to change.
        from .ddp import exchange_active, sync_initial_state
        if exchange_active(model):
            _check_torch_ddp(model)
        if getattr(model, "hip_ddp", True):
            sync_initial_state(model, late=True)
    eng = model._engine(n, H, W, prec)
    params = [p for p in model.parameters() if p.requires_grad]
    eps = _UNetTrainFn.apply(model, eng, (x, t, cond, layout, mask), *params)
    return eps, 0.0, dict()
