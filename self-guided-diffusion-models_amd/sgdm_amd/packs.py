"""Device copies that follow the parameters: the staleness rule, the packed igemm weights and their batched re-pack.

Everything a launch reads in place of a parameter -- its weight in the igemm layout (forward, adjoint, sub-pixel, fused
3x3+1x1), a zero-padded head layout, a concatenation -- is derived state and goes stale when an optimizer step, an EMA swap,
``load_state_dict`` or ``.to()`` touches the parameter.  ``Stale`` is the one statement of "touched"; ``Derived`` redoes an
arbitrary update under it, ``Packed`` / ``FusedPacked`` a weight pack, ``PackBatch`` many packs in one call.
"""
import ctypes as C
import os

import torch

from . import _lib as L


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Stale:
    """have the source tensors changed since ``mark()``?  Changed: another address (``.to()``, a re-materialised or replaced
    tensor) or, unless versions=False, a bumped version counter (in-place ops, the fused optimizer's explicit bump).  ``srcs``: a
    sequence, read at every ask, or a callable returning one.  Never marked: changed."""

    def __init__(self, srcs, versions=True):
        self.srcs, self.versions, self.seen = srcs, versions, None

    def key(self):
        srcs = self.srcs() if callable(self.srcs) else self.srcs
        if self.versions:
            return tuple((s.data_ptr(), s._version) for s in srcs)
        return tuple(s.data_ptr() for s in srcs)

    def changed(self):
        return self.key() != self.seen

    def mark(self):
        self.seen = self.key()


class Derived:
    """device state that ``update(stream)`` derives from ``srcs``, redone when they changed.  Callable, so it serves as a refresh
    hook and as a program entry (under ``update``'s name)."""

    def __init__(self, srcs, update):
        self.stale, self.update, self.__name__ = Stale(srcs), update, update.__name__

    def refresh(self, stream):
        if self.stale.changed():
            self.update(stream)
            self.stale.mark()
        return 0

    __call__ = refresh


class _Pad:
    """zero-padded re-layout of a 2-D weight (or a vector / [2, d] table along its last dim): source row r lands at row
    rows[r], source column c at column cols[c] of an [n_rows, n_cols] zero matrix.  ``gather`` is the adjoint (the
    gradient of the padded tensor read back at the positions of the real entries)."""

    def __init__(self, rows=None, n_rows=None, cols=None, n_cols=None):
        self.rows = None if rows is None else torch.as_tensor(rows, dtype=torch.int64)
        self.cols = None if cols is None else torch.as_tensor(cols, dtype=torch.int64)
        self.n_rows, self.n_cols = n_rows, n_cols

    def _idx(self, dev):
        if self.rows is not None and self.rows.device != dev:
            self.rows = self.rows.to(dev)
        if self.cols is not None and self.cols.device != dev:
            self.cols = self.cols.to(dev)

    def apply(self, w):
        self._idx(w.device)
        w2 = w.reshape(w.shape[0], -1)
        out = w2.new_zeros(self.n_rows if self.rows is not None else w2.shape[0],
                           self.n_cols if self.cols is not None else w2.shape[1])
        if self.rows is not None and self.cols is not None:
            out[self.rows[:, None], self.cols[None, :]] = w2
        elif self.rows is not None:
            out[self.rows] = w2
        else:
            out[:, self.cols] = w2
        return out

    def gather(self, wp):
        self._idx(wp.device)
        if self.rows is not None:
            wp = wp[self.rows]
        if self.cols is not None:
            wp = wp[:, self.cols]
        return wp


class Packed:
    """device buffer holding one conv / linear weight in the igemm layout, refreshed when the source parameter(s) change.

    kind: the library's job kind.  L.PACK_FORWARD: the operator itself; L.PACK_DGRAD: its adjoint (the input-gradient
    operator); L.PACK_SUBPIXEL: the 16 summed 2x2 kernels of a nearest-x2-upsample 3x3 conv (include/sgdm_hip.h:
    SGD_RS_UP2_SUBPIXEL; split modes only, its scale is that of max |V|).
    srcs: the parameters, concatenated along dim 0;  pad: the packed operator is the zero-padded re-layout (_Pad) of that;
    src_fn: returns the weight where it is a slice / concat of ``srcs`` that those two do not describe, ``dims`` = its
    (cout, cin).  cout / cin are always the FORWARD weight's, cin_p / cout_p the padded dims of the packed operator.
    donor: the forward pack of the same parameter, whose max |w| an adjoint pack reads instead of reducing its own.
    idle: ``refresh`` leaves the pack stale (_Engine.refresh: a pack only the training forward launches, while the engine
    serves inference)."""

    def __init__(self, srcs, ksize, prec, kind=L.PACK_FORWARD, pad=None, src_fn=None, dims=None, donor=None, device=None):
        self.srcs, self.names, self.ksize, self.prec, self.kind = srcs, (), ksize, prec, kind
        self.pad, self.src_fn, self.donor, self.idle = pad, src_fn, donor, False
        self.subpixel = kind == L.PACK_SUBPIXEL
        assert not self.subpixel or (ksize == 3 and pad is None and prec != L.PREC_F32)
        self.cout, self.cin = dims if dims is not None else (sum(s.shape[0] for s in srcs), srcs[0].shape[1])
        if pad is not None:
            assert ksize == 1
            self.cout = pad.n_rows if pad.rows is not None else self.cout
            self.cin = pad.n_cols if pad.cols is not None else self.cin
        lib, dev = L.load(), device if device is not None else srcs[0].device
        self.buf = torch.empty(self._bytes(lib) // 4, dtype=torch.float32, device=dev)
        ab, pb, cp, op = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        L.check(lib.sgd_pack_job_blocks(self.cout, self.cin, ksize, prec, kind, C.byref(ab), C.byref(pb), C.byref(cp), C.byref(op)),
                "sgd_pack_job_blocks")
        self.amax_blocks, self.pack_blocks, self.cin_p, self.cout_p = ab.value, pb.value, cp.value, op.value
        self.stale = Stale(srcs)
        # split precisions: per-tensor power-of-two scale so hi AND lo halves stay in fp16's normal range whatever the
        # tensor's magnitude (include/sgdm_hip.h: sgd_igemm_args.w_scale_inv); formed on the device, no host round trip
        self.scaled = prec != L.PREC_F32
        if self.scaled:
            self.amax = torch.zeros(1, dtype=torch.int32, device=dev)
            self.scale_inv = torch.ones(1, dtype=torch.float32, device=dev)

    def _bytes(self, lib):
        if self.subpixel:
            return int(lib.sgd_packed_weight_subpixel_bytes(self.cout, self.cin, self.prec))
        if self.kind == L.PACK_DGRAD:                                      # the adjoint's outputs are the forward's inputs
            return int(lib.sgd_packed_weight_bytes(self.cin, self.cout, self.ksize, self.prec))
        return int(lib.sgd_packed_weight_bytes(self.cout, self.cin, self.ksize, self.prec))

    @property
    def scale_ptr(self):
        return self.scale_inv.data_ptr() if self.scaled else 0

    def due(self):
        return not self.idle and self.stale.changed()

    def mark(self):
        """the buffer holds the sources as they are now (PackBatch, after its batched call)"""
        self.stale.mark()

    def refresh(self, stream):
        if self.due():
            self._pack(L.load(), stream)
            self.stale.mark()

    def _source(self):
        if self.src_fn is not None:
            src = self.src_fn().detach()
        else:
            src = self.srcs[0].detach() if len(self.srcs) == 1 else torch.cat([s.detach() for s in self.srcs], 0)
        src = src.contiguous().float()
        return src if self.pad is None else self.pad.apply(src).contiguous()

    def _whole(self, src):
        """is ``src`` the one source parameter, whole?"""
        return len(self.srcs) == 1 and src.data_ptr() == self.srcs[0].data_ptr() and src.numel() == self.srcs[0].numel()

    def batch_job(self):
        """the L.PackJob that re-packs this buffer from a device-side table (PackBatch) -- the source is one whole contiguous
        fp32 parameter -- else None: concatenated, zero-padded and sliced sources keep their own refresh"""
        p = self.srcs[0]
        if (len(self.srcs) != 1 or self.pad is not None or (self.src_fn is not None and not self._whole(self.src_fn()))
                or p.dtype != torch.float32 or not p.is_contiguous() or p.numel() != self.cout * self.cin * self.ksize ** 2):
            return None
        return L.PackJob(src=p.data_ptr(), dst=self.buf.data_ptr(), amax_bits=self.amax.data_ptr() if self.scaled else 0,
                         scale_inv=self.scale_ptr, cout=self.cout, cin=self.cin, ksize=self.ksize, transpose=self.kind,
                         own_amax=1 if self.scaled else 0)

    def _lent_amax(self, src):
        """the donor's max |w|: it reduced this very tensor (one whole unpadded parameter, not the sub-pixel sums) and was
        refreshed at the parameter's current version -- on the same stream, earlier"""
        d = self.donor
        if (d is not None and d.scaled and d.kind == L.PACK_FORWARD and d.pad is None and d.src_fn is None and len(d.srcs) == 1
                and d.srcs[0] is self.srcs[0] and self.pad is None and self._whole(src) and not d.stale.changed()):
            return d.amax
        return None

    def _pack(self, lib, stream):
        src = self._source()
        cin_p, cout_p = C.c_int32(0), C.c_int32(0)
        dims = (C.byref(cin_p), C.byref(cout_p), stream)
        if not self.scaled:
            pack = lib.sgd_pack_weight_dgrad if self.kind == L.PACK_DGRAD else lib.sgd_pack_weight
            L.check(pack(_ptr(src), _ptr(self.buf), self.cout, self.cin, self.ksize, self.prec, *dims), "sgd_pack_weight")
        else:
            amax = self._lent_amax(src) if self.kind == L.PACK_DGRAD else None
            if amax is None:
                amax = self.amax
                amax.zero_()
                if self.subpixel:
                    L.check(lib.sgd_weight_amax_subpixel(_ptr(src), self.cout, self.cin, _ptr(amax), stream), "sgd_weight_amax_subpixel")
                else:
                    L.check(lib.sgd_weight_amax(_ptr(src), src.numel(), _ptr(amax), stream), "sgd_weight_amax")
            if self.subpixel:
                L.check(lib.sgd_pack_weight_subpixel_scaled(_ptr(src), _ptr(self.buf), self.cout, self.cin, self.prec, _ptr(amax),
                                                            _ptr(self.scale_inv), *dims), "sgd_pack_weight_subpixel_scaled")
            else:
                L.check(lib.sgd_pack_weight_scaled(_ptr(src), _ptr(self.buf), self.cout, self.cin, self.ksize, self.prec, self.kind,
                                                   _ptr(amax), _ptr(self.scale_inv), *dims), "sgd_pack_weight_scaled")
        assert (cin_p.value, cout_p.value) == (self.cin_p, self.cout_p)
        self._keep = src


class FusedPacked(Packed):
    """A channel-changing ResBlock's out_layers.3 (3x3) and skip_connection (1x1) weights packed back to back for
    sgd_igemm_fused_aux: the two products share their accumulators, so both tensors carry the scale of ONE amax folded over
    both; the launch's bias is the sum of the two biases.  Follows all four parameters' versions; refreshed only in front of an
    inference evaluation (the training forward launches the pair from their own packs).  Dims are the 3x3 operator's."""

    def __init__(self, w3, w1, b3, b1, prec):
        assert w1.shape[0] == w3.shape[0] and prec != L.PREC_F32
        self.caux = w1.shape[1]
        super().__init__([w3], 3, prec)
        self.srcs = [w3, w1, b3, b1]
        self.stale = Stale(self.srcs)
        self.bias = torch.empty(self.cout, dtype=torch.float32, device=w3.device)

    def _bytes(self, lib):
        self.off1 = super()._bytes(lib)                                    # the 1x1 units follow the 3x3 ones
        return self.off1 + int(lib.sgd_packed_weight_bytes(self.cout, self.caux, 1, self.prec))

    def _pack(self, lib, stream):
        w3, w1 = (s.detach().contiguous().float() for s in self.srcs[:2])
        self.amax.zero_()
        for w in (w3, w1):
            L.check(lib.sgd_weight_amax(_ptr(w), w.numel(), _ptr(self.amax), stream), "sgd_weight_amax")
        cin_p, cout_p, cx_p = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.check(lib.sgd_pack_weight_scaled(_ptr(w3), _ptr(self.buf), self.cout, self.cin, 3, self.prec, 0, _ptr(self.amax),
                                           _ptr(self.scale_inv), C.byref(cin_p), C.byref(cout_p), stream), "sgd_pack_weight_scaled")
        L.check(lib.sgd_pack_weight_scaled(_ptr(w1), C.c_void_p(self.buf.data_ptr() + self.off1), self.cout, self.caux, 1,
                                           self.prec, 0, _ptr(self.amax), _ptr(self.scale_inv), C.byref(cx_p), C.byref(cout_p),
                                           stream), "sgd_pack_weight_scaled")
        torch.add(self.srcs[2].detach().float(), self.srcs[3].detach().float(), out=self.bias)
        self._keep = (w3, w1)


class PackBatch:
    """the weight packs of one launch program refreshed together: when (almost) all of them are stale -- every step of a
    training loop -- ONE sgd_pack_weights_batched call (zero + amax + pack kernels over a device-side job table) replaces
    two launches per tensor (142 pack + 74 amax launches of ~6 us per step at C2).  Members are the packs that answer
    ``batch_job()``; the others keep their own refresh."""

    MIN_STALE = 8           # fewer stale packs than this: refresh them one by one

    def __init__(self, packs, prec, dev):
        self.packs, self.prec, self.dev = list(packs), prec, dev
        self.lib = L.load()
        self.members = None

    def _build(self):
        members, jobs, a_job, a_first, p_job, p_first = [], [], [], [0], [], [0]
        for pk in self.packs:
            job = pk.batch_job()
            if job is None:
                continue
            a_job += [len(members)] * (pk.amax_blocks if pk.scaled else 0)
            a_first.append(len(a_job))
            p_job += [len(members)] * pk.pack_blocks
            p_first.append(len(p_job))
            members.append(pk)
            jobs.append(job)
        self.members = members
        self.table = Stale([pk.srcs[0] for pk in members], versions=False)
        self.table.mark()
        if not members:
            return
        arr = (L.PackJob * len(jobs))(*jobs)
        self.jobs = torch.frombuffer(bytearray(C.string_at(C.addressof(arr), C.sizeof(arr))), dtype=torch.uint8).to(self.dev)
        i32t = lambda v: torch.tensor(v if v else [0], dtype=torch.int32, device=self.dev)
        self.a_job, self.a_first, self.p_job, self.p_first = i32t(a_job), i32t(a_first), i32t(p_job), i32t(p_first)
        self.n_a, self.n_p = len(a_job), len(p_job)

    def refresh(self, stream):
        if self.members is None or self.table.changed():
            self._build()                                          # first use, or a parameter moved (.to(), re-materialised)
        if (sum(pk.due() for pk in self.members) >= self.MIN_STALE and os.environ.get("SGDM_BATCHED_PACK", "1") != "0"):
            L.check(self.lib.sgd_pack_weights_batched(_ptr(self.jobs), len(self.members), _ptr(self.a_job), _ptr(self.a_first),
                                                      self.n_a, _ptr(self.p_job), _ptr(self.p_first), self.n_p, self.prec,
                                                      stream), "sgd_pack_weights_batched")
            for pk in self.members:                                # (fresh and idle members were re-packed too: same bytes)
                pk.mark()
        for pk in self.packs:                                      # the rest, and small stale sets, one by one
            pk.refresh(stream)
