#!/usr/bin/env python3
"""A/B of a channel-changing ResBlock's tail IN ONE PROCESS, interleaved (as tools/ab_conv.py): the pair the training forward
launches -- skip_connection (1x1, sgd_igemm) into a tensor of its own, then out_layers.3 (3x3, sgd_igemm) with that tensor as its
residual -- against the one fused launch of the inference forward (sgd_igemm_fused_aux).  Shapes: the eleven such blocks of the
flagship model (ch = 128, mult 1/2/4, 64 x 64) at UNet batch 80, one line per distinct shape with its count per evaluation.

    python tools/ab_fused_skip.py [--n 80] [--rounds 7] [--reps 20] [--prec f16x3|bf16x3]"""
import argparse, ctypes as C, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import torch
from sgdm_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=80); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--prec", default="f16x3")
a = ap.parse_args()
lib = L.load()
prec = L.PREC_BY_NAME[a.prec]
st = torch.cuda.current_stream().cuda_stream
p = lambda t: C.c_void_p(t.data_ptr())
# (aux c0, aux c1, cout, hw, blocks per evaluation)
SHAPES = [(128, 0, 256, 32, 1), (256, 0, 512, 16, 1), (512, 512, 512, 16, 2), (512, 256, 512, 16, 1), (512, 256, 256, 32, 1),
          (256, 256, 256, 32, 1), (256, 128, 256, 32, 1), (256, 128, 128, 64, 1), (128, 128, 128, 64, 2)]
work = torch.zeros(int(lib.sgd_igemm_work_bytes()) // 4, device="cuda")


def pack(ws_ks, cout):
    sizes = [int(lib.sgd_packed_weight_bytes(cout, w.shape[1], ks, prec)) for w, ks in ws_ks]
    buf = torch.empty(sum(sizes) // 4, device="cuda")
    amax, sinv = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, device="cuda")
    for w, _ in ws_ks:
        L.check(lib.sgd_weight_amax(p(w), w.numel(), p(amax), st), "amax")
    off, dims = 0, None
    for (w, ks), nb in zip(ws_ks, sizes):
        cp, op = C.c_int32(), C.c_int32()
        L.check(lib.sgd_pack_weight_scaled(p(w), C.c_void_p(buf.data_ptr() + off), cout, w.shape[1], ks, prec, 0, p(amax), p(sinv),
                                           C.byref(cp), C.byref(op), st), "pack")
        dims = dims or (cp.value, op.value)
        off += nb
    return buf, sinv, dims


tot_pair = tot_fused = tot_skip = 0.0
n = a.n
for ac0, ac1, cout, hw, count in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    h, x0 = r(n, hw, hw, cout), r(n, hw, hw, ac0)
    x1 = r(n, hw, hw, ac1) if ac1 else None
    pa, pb = 1 + 0.3 * r(n, cout), 0.3 * r(n, cout)
    w3, w1 = r(cout, cout, 3, 3) / (9 * cout) ** 0.5, r(cout, ac0 + ac1) / (ac0 + ac1) ** 0.5
    b3, bs = r(cout), r(cout)
    bsum = b3 + bs
    skip = torch.empty(n, hw, hw, cout, device="cuda")
    y_pair, y_fused = torch.full_like(skip, float("nan")), torch.full_like(skip, float("nan"))

    def conv(y, w, sinv, dims, bias, res):
        q = L.IgemmArgs()
        q.x0, q.c0 = h.data_ptr(), cout
        q.mode, q.n, q.hi, q.wi, q.ho, q.wo, q.stride = L.MODE_CONV3, n, hw, hw, hw, hw, 1
        q.pro, q.pro_silu, q.pa, q.pb = L.PRO_AFFINE_NC, 1, pa.data_ptr(), pb.data_ptr()
        q.w, q.w_scale_inv, (q.cin_p, q.cout_p), q.bias = w.data_ptr(), sinv.data_ptr(), dims, bias.data_ptr()
        q.res = res.data_ptr() if res is not None else 0
        q.y, q.cout, q.y_ld, q.prec = y.data_ptr(), cout, cout, prec
        q.work, q.work_bytes = work.data_ptr(), work.numel() * 4
        parts = lib.sgd_igemm_stats_parts(C.byref(q))
        stats = torch.empty(n, parts, 2, cout, device="cuda")
        q.stats = stats.data_ptr()
        return q, stats

    k1 = pack([(w1, 1)], cout)
    k3 = pack([(w3, 3)], cout)
    kf = pack([(w3, 3), (w1, 1)], cout)
    qs = L.IgemmArgs()
    qs.x0, qs.c0, qs.c1, qs.x1 = x0.data_ptr(), ac0, ac1, (x1.data_ptr() if ac1 else 0)
    qs.mode, qs.m, qs.rows_per_n, qs.stride = L.MODE_FLAT, n * hw * hw, hw * hw, 1
    qs.w, qs.w_scale_inv, (qs.cin_p, qs.cout_p), qs.bias = k1[0].data_ptr(), k1[1].data_ptr(), k1[2], bs.data_ptr()
    qs.y, qs.cout, qs.y_ld, qs.prec = skip.data_ptr(), cout, cout, prec
    qs.work, qs.work_bytes = work.data_ptr(), work.numel() * 4
    qc, keep_c = conv(y_pair, k3[0], k3[1], k3[2], b3, skip)
    qf, keep_f = conv(y_fused, kf[0], kf[1], kf[2], bsum, None)
    xa = L.IgemmAux(x0=x0.data_ptr(), x1=x1.data_ptr() if ac1 else 0, c0=ac0, c1=ac1)
    if not lib.sgd_igemm_fused_aux_ok(C.byref(qf), C.byref(xa)):
        print(f"aux {ac0}|{ac1} -> {cout} @{hw}^2: refused by sgd_igemm_fused_aux_ok", flush=True)
        continue

    def run_skip(): return lib.sgd_igemm(C.byref(qs), st)
    def run_conv(): return lib.sgd_igemm(C.byref(qc), st)
    def run_pair(): return run_skip() or run_conv()
    def run_fused(): return lib.sgd_igemm_fused_aux(C.byref(qf), C.byref(xa), st)
    runs = [("skip", run_skip, []), ("conv+res", run_conv, []), ("pair", run_pair, []), ("fused", run_fused, [])]
    for nm, fn, ts in runs:
        for _ in range(3):
            L.check(fn(), nm)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for nm, fn, ts in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / a.reps)
    med = {nm: statistics.median(ts) for nm, fn, ts in runs}
    mn = {nm: min(ts) for nm, fn, ts in runs}
    d = float((y_fused - y_pair).abs().max() / y_pair.abs().max())
    fl = 2.0 * n * hw * hw * cout * (9 * cout + ac0 + ac1)
    print(f"aux {ac0}|{ac1} -> {cout} @{hw}^2 x{count}:  skip {med['skip']:.4f}  conv+res {med['conv+res']:.4f}  pair {med['pair']:.4f} ms "
          f"(min {mn['pair']:.4f}, {fl / med['pair'] / 1e9:.0f} TF)  fused {med['fused']:.4f} ms (min {mn['fused']:.4f}, {fl / med['fused'] / 1e9:.0f} TF)  "
          f"saved {med['pair'] - med['fused']:+.4f} ms  d={d:.1e}", flush=True)
    tot_pair += count * med["pair"]; tot_fused += count * med["fused"]; tot_skip += count * med["skip"]
print(f"per evaluation (11 blocks): skip launches {tot_skip:.3f} ms, pairs {tot_pair:.3f} ms, fused {tot_fused:.3f} ms, saved {tot_pair - tot_fused:+.3f} ms")
