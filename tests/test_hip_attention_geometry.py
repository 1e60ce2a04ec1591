"""The six softmax attention cores over seeded random geometry, against float64 (tests/attention_refs.py): every tq / tk around
the wave, block and key-tile boundaries, the three q / k / v layouts, padded row strides on every tensor, logits sharp enough for
the online-softmax rescale, key masks that empty whole sub-tiles -- and, around every output, guard rows and padding columns that
must come back untouched.  One sweep = one test of 24 launches (tests/test_hip_kernels.py does the same for the convolutions)."""
import ctypes as C
import functools

import pytest
import torch

import attention_refs as R
from conftest import max_rel
from test_hip_kernels import ATTN_CORES

pytestmark = pytest.mark.gpu

# forward: the project's own tolerances (test_hip_kernels.ATTN_CORES); the masked core is the exact core with a mask
FWD = {"exact": ("sgd_attention", dict(ATTN_CORES)["sgd_attention"]),
       "split": ("sgd_attention_split", dict(ATTN_CORES)["sgd_attention_split"]),
       "masked": ("sgd_attention_masked", dict(ATTN_CORES)["sgd_attention"])}
LSE_TOL = 2e-5                   # absolute, test_hip_kernels.test_attention_legacy
COMPACT_TOL = 2e-6               # test_hip_attention_ldm.test_masked_attention_core_equals_dropping_the_keys
# backward: test_hip_backward.test_attention_backward, test_hip_attention_ldm.test_masked_attention_backward_vs_autograd
BWD = {"exact": ("sgd_attention_bwd", "exact", 1e-5), "split": ("sgd_attention_bwd_split", "split", 1e-5),
       "masked": ("sgd_attention_masked_bwd", "masked", 5e-6)}
FWD_SWEEP = {"exact": "plain", "split": "plain", "masked": "masked"}
BWD_SWEEP = {"exact": "plain", "split": "plain_to_64", "masked": "masked_backward"}


def _lib():
    from sgdm_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _reference(sweep):
    """cases, inputs and float64 results of a sweep, computed once and shared by the tests that use it (never modified)"""
    out = []
    for cs in R.sweep_cases(sweep):
        t = R.case_tensors(cs)
        o, lse = R.ref_attention(t["q"], t["k"], t["v"], t["scale"], t["mask"])
        dq, dk, dv = R.ref_attention_grads(t["q"], t["k"], t["v"], t["dout"], t["scale"], t["mask"])
        floor = [float(x.max()) for x in R.ref_attention_grad_scales(t["q"], t["k"], t["v"], t["dout"], t["scale"], t["mask"])]
        out.append((cs, t, dict(out=o, lse=lse, dq=dq, dk=dk, dv=dv, floor=dict(zip(("dq", "dk", "dv"), floor)))))
    return out


class _Staged:
    """the inputs of a case on the device in the case's layout, NaN in every padding column"""

    def __init__(self, cs, t):
        heads, d = cs["heads"], cs["d"]
        self.hk = hk = 1 if cs["layout"] == "mq" else heads
        if cs["layout"] == "legacy":
            self.qkv = R.legacy_rows(t["q"], t["k"], t["v"], cs["q_ld"]).cuda()
            self.q, self.k, self.v = (self.qkv.data_ptr() + 4 * d * i for i in range(3))
        else:
            self.qd = R.rows_of(t["q"], cs["q_ld"]).cuda()
            self.kvd = torch.cat([R.rows_of(t["k"], hk * d), R.rows_of(t["v"], cs["kv_ld"] - hk * d)], -1).cuda()
            self.q, self.k, self.v = self.qd.data_ptr(), self.kvd.data_ptr(), self.kvd.data_ptr() + 4 * hk * d
        self.dout = R.rows_of(t["dout"], cs["dout_ld"]).cuda()
        self.mask = t["mask"].to(torch.uint8).cuda() if t["mask"] is not None else None
        self.geom = (cs["b"], heads, cs["tq"], cs["tk"], d, t["scale"])


def _own_max_rel(got, ref, floor):
    """max |got - ref| / max |ref|, each gradient against ITS OWN maximum (test_hip_backward.test_attention_backward).  Where that
    maximum is exactly zero -- every row attends to one key alone: dq = dk = 0, attention_refs.ref_attention_grad_scales -- the
    error is counted in units of the largest term of the sum that cancels instead."""
    den = float(ref.abs().max())
    return float((got.double() - ref).abs().max()) / (den if den > 0.0 else floor)


def _raise(failures):
    """every failing case with its index, findings and whole dict (raised by hand: pytest shortens a rewritten assert's message)"""
    if failures:
        raise AssertionError("\n".join(f"case {ci}: {bad}\n    {cs}" for ci, cs, bad in failures))


def _launch_forward(lib, L, core, cs, sg, tag):
    b, heads, tq = cs["b"], cs["heads"], cs["tq"]
    out = R.Guarded(b * tq, cs["out_ld"], heads * cs["d"])
    lse = R.Guarded(b * heads, tq)
    args = [sg.q, cs["q_ld"], cs["q_hs"], sg.k, sg.v, cs["kv_ld"], cs["kv_hs"]]
    if core == "sgd_attention_masked":
        args.append(sg.mask.data_ptr())
    L.check(getattr(lib, core)(*args, *sg.geom, out.ptr, cs["out_ld"], lse.ptr, _stream()), f"{core} {tag}")
    torch.cuda.synchronize()
    return out, lse


def _compacted(lib, L, cs, t, sg):
    """sgd_attention on the attended keys alone, batch element by batch element -> [b, heads, tq, d]"""
    b, heads, tq, tk, d, scale = sg.geom
    res = []
    for i in range(b):
        keep = t["mask"][i]
        kv = torch.cat([R.rows_of(t["k"][i:i + 1, :, keep], sg.hk * d), R.rows_of(t["v"][i:i + 1, :, keep], sg.hk * d)], -1).cuda()
        out = torch.empty(1, tq, heads * d, device="cuda")
        L.check(lib.sgd_attention(sg.q + 4 * i * tq * cs["q_ld"], cs["q_ld"], cs["q_hs"], kv.data_ptr(),
                                  kv.data_ptr() + 4 * sg.hk * d, 2 * sg.hk * d, cs["kv_hs"], 1, heads, tq, int(keep.sum()), d,
                                  scale, out.data_ptr(), heads * d, None, _stream()), "sgd_attention on the compacted keys")
        res.append(R.heads_of(out.cpu(), heads, d))
    return torch.cat(res)


def run_forward_sweep(kind, report=None):
    """one forward core over its 24 cases -> ({d: worst max_rel of out}, failures); `report` (a list) receives one line per case"""
    L, lib = _lib()
    core, tol = FWD[kind]
    worst, failures = {}, []
    for ci, (cs, t, ref) in enumerate(_reference(FWD_SWEEP[kind])):
        b, heads, tq, tk, d = cs["b"], cs["heads"], cs["tq"], cs["tk"], cs["d"]
        sg = _Staged(cs, t)
        out, lse = _launch_forward(lib, L, core, cs, sg, f"case {ci}: {cs}")
        got = R.heads_of(out.owned().view(b, tq, heads * d), heads, d)
        got_lse = lse.owned().view(b, heads, tq)
        err = max_rel(got, ref["out"])
        err_lse = float((got_lse.double() - ref["lse"]).abs().max())
        worst[d] = max(worst.get(d, 0.0), err)
        if report is not None:
            report.append(f"{core} case {ci:2d} d {d:3d} tq {tq:3d} tk {tk:3d} {cs['layout']:8s} out {err:.2e} lse {err_lse:.2e}")
        bad = []
        if not err < tol:
            bad.append(("out", err))
        if not err_lse < LSE_TOL:
            bad.append(("lse", err_lse))
        if not (out.written() and lse.written()):
            bad.append("an owned element was not written")
        if not out.untouched():
            bad.append("a write outside the rows and columns of out")
        if not lse.untouched():
            bad.append("a write outside lse")
        if tk == 1:
            # one key: P = exp(s - s) is exactly 1, l and 1 / l are exactly 1, and 1 * v plus exact zeros is v: the exact cores
            # return V's row bit for bit.  The split core carries P times 2^14 as exp2(fma(s, log2 e, 14 - s log2 e)), which is
            # 2^14 only up to the rounding of the two products, and then splits it into f16 halves: held to its tolerance (above).
            want = t["v"].expand(-1, heads, -1, -1).expand(-1, -1, tq, -1)
            if kind != "split" and not torch.equal(got, want):
                bad.append("tk == 1 must return V's row bit for bit")
        if kind == "masked":
            err_c = max_rel(got, _compacted(lib, L, cs, t, sg))
            if not err_c < COMPACT_TOL:
                bad.append(("vs sgd_attention on the compacted keys", err_c))
        if bad:
            failures.append((ci, cs, bad))
    return worst, failures


def run_backward_sweep(kind, report=None):
    """one backward core over its 24 cases -> ({d: worst max_rel over dq, dk, dv, each against its own maximum}, failures)"""
    L, lib = _lib()
    core, fwd_kind, tol = BWD[kind]
    worst, failures = {}, []
    for ci, (cs, t, ref) in enumerate(_reference(BWD_SWEEP[kind])):
        b, heads, tq, tk, d = cs["b"], cs["heads"], cs["tq"], cs["tk"], cs["d"]
        sg = _Staged(cs, t)
        hk = sg.hk
        # o and lse from the matching forward launch, on the same padded buffers (forward: o_ld is out_ld)
        out, lse = _launch_forward(lib, L, FWD[fwd_kind][0], cs, sg, f"forward of case {ci}: {cs}")
        dvec = R.Guarded(b * heads, tq)
        if cs["layout"] == "legacy":         # three windows of one gqkv buffer
            gqkv = R.Guarded(b * tq, cs["q_ld"], 3 * heads * d)
            dq_p, dk_p, dv_p = (gqkv.ptr + 4 * d * i for i in range(3))
            outs = {"gqkv": gqkv}
        else:
            gq, gkv = R.Guarded(b * tq, cs["q_ld"], heads * d), R.Guarded(b * tk, cs["kv_ld"], 2 * hk * d)
            dq_p, dk_p, dv_p = gq.ptr, gkv.ptr, gkv.ptr + 4 * hk * d
            outs = {"dq": gq, "dkv": gkv}
        args = [sg.q, cs["q_ld"], cs["q_hs"], sg.k, sg.v, cs["kv_ld"], cs["kv_hs"]]
        if kind == "masked":
            args.append(sg.mask.data_ptr())
        L.check(getattr(lib, core)(*args, out.ptr, cs["out_ld"], sg.dout.data_ptr(), cs["dout_ld"], lse.ptr, dvec.ptr, *sg.geom,
                                   dq_p, dk_p, dv_p, _stream()), f"{core} case {ci}: {cs}")
        torch.cuda.synchronize()
        if cs["layout"] == "legacy":
            got = dict(zip(("dq", "dk", "dv"), R.legacy_split(gqkv.owned().view(b, tq, 3 * heads * d), heads, d)))
        else:
            rows = gkv.owned().view(b, tk, 2 * hk * d)
            got = dict(dq=R.heads_of(gq.owned().view(b, tq, heads * d), heads, d), dk=R.heads_of(rows, hk, d),
                       dv=R.heads_of(rows[:, :, hk * d:], hk, d))
        # (multi-query: the reference's dk / dv are the head sums)
        errs = {nm: _own_max_rel(got[nm], ref[nm], ref["floor"][nm]) for nm in ("dq", "dk", "dv")}
        worst[d] = max(worst.get(d, 0.0), *errs.values())
        if report is not None:
            report.append(f"{core} case {ci:2d} d {d:3d} tq {tq:3d} tk {tk:3d} {cs['layout']:8s} "
                          + " ".join(f"{nm} {e:.2e}" for nm, e in errs.items()))
        bad = [(nm, e) for nm, e in errs.items() if not e < tol]
        outs["dvec"] = dvec
        for nm, buf in outs.items():
            if not buf.written():
                bad.append(f"an owned element of {nm} was not written")
            if not buf.untouched():
                bad.append(f"a write outside the rows and columns of {nm}")
        if not (out.untouched() and lse.untouched()):
            bad.append("the backward wrote next to its inputs o / lse")
        if kind == "masked":
            dead = ~t["mask"][:, None, :].expand(b, hk, tk)
            if float(got["dk"][dead].abs().sum()) != 0.0 or float(got["dv"][dead].abs().sum()) != 0.0:
                bad.append("a masked key's dk / dv row is not exactly zero")
        if bad:
            failures.append((ci, cs, bad))
    return worst, failures


@pytest.mark.parametrize("kind", ["exact", "split", "masked"])
def test_forward_random_geometry(kind):
    _raise(run_forward_sweep(kind)[1])


@pytest.mark.parametrize("kind", ["exact", "split", "masked"])
def test_backward_random_geometry(kind):
    """[exact], case 15 of sweep "plain" (legacy layout, b 2, heads 2, d 64, tq = tk = 2, sharpness 4) is the case that decides how
    the exact backward forms dS = P (dP - D).  With two keys and logits of standard deviation 4 every row is saturated (the
    smaller weight P2 is 1e-4 .. 3e-2), dP - D = +-P2 (dP1 - dP2) is a difference of two nearly equal numbers, and with two queries
    dk's own maximum is 1 / 72 of its absolute-value form (attention_refs.ref_attention_grad_scales).  With D summed in fp32 and
    subtracted from a dP accumulated from zero the kernel left dk at 1.23e-5 of its own maximum, outside the 1e-5 bound; with D
    summed in double and the dP accumulator started at -D it is at 6.1e-6 (profiles/attention_geometry_errors.txt)."""
    _raise(run_backward_sweep(kind)[1])


def test_refusals():
    """contract checks (include/sgdm_hip.h, "Attention cores"): each call changes one thing in a launch the sweeps above accept,
    must return non-zero and launches nothing.  Every pointer lies inside one large buffer all the same."""
    L, lib = _lib()
    arena = torch.zeros(10 * 8192, device="cuda")
    at = lambda i: arena.data_ptr() + 4 * 8192 * i
    b, heads, tq, tk, d = 1, 2, 8, 8, 16
    base = dict(q=at(0), q_ld=heads * d, q_hs=d, k=at(1), v=at(1) + 4 * heads * d, kv_ld=2 * heads * d, kv_hs=d, kmask=at(2),
                o=at(3), o_ld=heads * d, dout=at(4), dout_ld=heads * d, lse=at(5), dvec=at(6), b=b, heads=heads, tq=tq, tk=tk,
                d=d, scale=d ** -0.5, dq=at(7), dk=at(8), dv=at(8) + 4 * heads * d)

    def call(core, **change):
        a = dict(base, **change)
        mask = [a["kmask"]] if "masked" in core else []
        head = [a["q"], a["q_ld"], a["q_hs"], a["k"], a["v"], a["kv_ld"], a["kv_hs"], *mask]
        geom = [a["b"], a["heads"], a["tq"], a["tk"], a["d"], a["scale"]]
        if "bwd" in core:
            return getattr(lib, core)(*head, a["o"], a["o_ld"], a["dout"], a["dout_ld"], a["lse"], a["dvec"], *geom, a["dq"],
                                      a["dk"], a["dv"], _stream())
        return getattr(lib, core)(*head, *geom, a["o"], a["o_ld"], a["lse"], _stream())

    forward = [core for core, _ in FWD.values()]
    backward = [core for core, _, _ in BWD.values()]
    for core in forward + backward:
        assert call(core, d=24) != 0, (core, "d = 24")
        for key in ("q_ld", "kv_ld", "q_hs", "kv_hs"):
            assert call(core, **{key: base[key] + 2}) != 0, (core, key, "not a multiple of 4")
        assert call(core, q=base["q"] + 4) != 0, (core, "q misaligned by 4 bytes")
    for core in backward:
        for key in ("o_ld", "dout_ld"):
            assert call(core, **{key: base[key] + 2}) != 0, (core, key, "not a multiple of 4")
    assert call("sgd_attention_split", o_ld=base["o_ld"] + 2) != 0 and call("sgd_attention_split", o=base["o"] + 4) != 0
    assert call("sgd_attention_bwd_split", d=128, q_ld=256, q_hs=128, kv_ld=512, kv_hs=128, o_ld=256, dout_ld=256,
                v=base["k"] + 4 * 256, dv=base["dk"] + 4 * 256) != 0, "the split backward has no 128-wide instance"
    assert call("sgd_attention_masked_bwd", kv_hs=0, kv_ld=2 * d, v=base["k"] + 4 * d, dv=base["dk"] + 4 * d) != 0, \
        "the masked backward sums no heads: kv_hs == 0 only with one head"
    torch.cuda.synchronize()
    assert float(arena.abs().max()) == 0.0, "a refused call launched"
