#!/usr/bin/env python3
"""A/B of the fused conv kernel across builds / launch modes IN ONE PROCESS (cdna_hip_programming.md rule 24): every
variant is a (library path, per-call overrides) pair -- `tune=<SGD_TUNE_* bits>` / `grid_cap=<n>` set the fields of
sgd_igemm_args (the library reads no environment), anything else is put into the environment for libraries older than
ABI 15; rounds are interleaved, median and min reported, outputs of all variants compared with the first.

    python tools/ab_conv.py --variants base=lib/libsgdm_hip_base.so new=lib/libsgdm_hip.so new256=lib/libsgdm_hip.so:tune=2 \
        --shapes 80,256,256,64 80,512,512,32 ... [--rounds 7] [--reps 20] [--prec f32|f16x3|bf16x3|f16|bf16] [--plain] [--stats] [--res-mode same|avgpool|up]
--stats: the launches also write their GroupNorm statistic slots (where the shape has any); every variant's output and slots are
compared with the first variant's BIT FOR BIT (`bits=same` / `bits=DIFF`, `stats=same` / `stats=DIFF`) next to the relative difference.
shape = n,cin,cout,hw[,ks[,up]]: up = 1 -- the nearest-x2-upsample conv of a hw x hw input (ResBlock up / Upsample, no
residual); a variant with `subpixel=1` runs it as the sub-pixel conv (SGD_RS_UP2_SUBPIXEL) on the sub-pixel pack:
    --variants direct=lib/libsgdm_hip.so sub128=lib/libsgdm_hip.so:subpixel=1:tune=1 sub256=lib/libsgdm_hip.so:subpixel=1:tune=2 \
    --shapes 80,512,512,16,3,1 80,256,256,32,3,1"""
import argparse, ctypes as C, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import torch
from sgdm_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--variants", nargs="+", required=True)
ap.add_argument("--shapes", nargs="+", required=True)
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--prec", default="f16x3"); ap.add_argument("--plain", action="store_true")
ap.add_argument("--stats", action="store_true")
ap.add_argument("--res-mode", default="same", choices=["same", "avgpool", "up"],
                help="3x3 launches: the residual is a map of the output's size, the 2x2 average of one at twice the resolution "
                     "(ResBlock down) or the nearest pixel of one at half the resolution (ResBlock up)")
a = ap.parse_args()
LIBDIR = os.path.dirname(L.LIB_PATH)


def load(path):
    lib = C.CDLL(path if os.path.isabs(path) else os.path.join(os.path.dirname(LIBDIR), path))
    for name, (res, args) in L.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    return lib


variants = []
for v in a.variants:
    name, rest = v.split("=", 1)
    path, *envs = rest.split(":")
    variants.append((name, load(path), dict(e.split("=") for e in envs)))
prec = L.PREC_BY_NAME[a.prec]
st = torch.cuda.current_stream().cuda_stream
WORK = {}
for shp in a.shapes:
    f = [int(x) for x in shp.split(",")]
    n, cin, cout, hw = f[:4]; ks = f[4] if len(f) > 4 else 3
    up = len(f) > 5 and f[5] == 1
    ho = 2 * hw if up else hw
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(n, hw, hw, cin, device="cuda", generator=g)
    w = torch.randn(cout, cin, ks, ks, device="cuda", generator=g) / (cin * ks * ks) ** 0.5
    rhw = hw if ks != 3 or a.res_mode == "same" else (2 * hw if a.res_mode == "avgpool" else hw // 2)
    bias = torch.randn(cout, device="cuda", generator=g); res = torch.randn(n, rhw, rhw, cout, device="cuda", generator=g)
    pa, pb = 1 + 0.3 * torch.randn(n, cin, device="cuda", generator=g), 0.3 * torch.randn(n, cin, device="cuda", generator=g)
    runs = []
    for name, lib, env in variants:
        sub = up and env.get("subpixel") == "1"
        cp, op = C.c_int32(), C.c_int32()
        sinv = torch.ones(1, device="cuda")
        if sub:                                              # the 16 summed kernels, scaled by max |V|
            amax = torch.zeros(1, dtype=torch.int32, device="cuda")
            buf = torch.empty(lib.sgd_packed_weight_subpixel_bytes(cout, cin, prec) // 4, device="cuda")
            L.check(lib.sgd_weight_amax_subpixel(C.c_void_p(w.data_ptr()), cout, cin, C.c_void_p(amax.data_ptr()), st), "amax")
            L.check(lib.sgd_pack_weight_subpixel_scaled(C.c_void_p(w.data_ptr()), C.c_void_p(buf.data_ptr()), cout, cin, prec,
                                                        C.c_void_p(amax.data_ptr()), C.c_void_p(sinv.data_ptr()), C.byref(cp),
                                                        C.byref(op), st), "pack")
        else:
            buf = torch.empty(lib.sgd_packed_weight_bytes(cout, cin, ks, prec) // 4, device="cuda")
            L.check(lib.sgd_pack_weight(C.c_void_p(w.data_ptr()), C.c_void_p(buf.data_ptr()), cout, cin, ks, prec, C.byref(cp), C.byref(op), st), "pack")
        y = torch.full((n, ho, ho, cout), float("nan"), device="cuda")
        q = L.IgemmArgs()
        q.x0, q.c0 = x.data_ptr(), cin
        if ks == 3:
            q.mode, q.n, q.hi, q.wi, q.ho, q.wo, q.stride = L.MODE_CONV3, n, hw, hw, ho, ho, 1
            q.resample = (L.RS_UP2_SUBPIXEL if sub else L.RS_UP2) if up else L.RS_NONE
            q.w_scale_inv = sinv.data_ptr()
        else:
            q.mode, q.m, q.rows_per_n, q.stride = L.MODE_FLAT, n * hw * hw, hw * hw, 1
        if not a.plain:
            q.pro, q.pro_silu, q.pa, q.pb = L.PRO_AFFINE_NC, 1, pa.data_ptr(), pb.data_ptr()
            q.res = 0 if up else res.data_ptr()
            if ks == 3 and not up:
                q.res_mode = {"same": L.RS_NONE, "avgpool": L.RS_AVGPOOL2, "up": L.RS_UP2}[a.res_mode]
        q.w, q.cin_p, q.cout_p, q.bias = buf.data_ptr(), cp.value, op.value, bias.data_ptr()
        q.y, q.cout, q.y_ld, q.prec = y.data_ptr(), cout, cout, prec
        q.tune, q.grid_cap = int(env.get("tune", 0)), int(env.get("grid_cap", 0))
        env = {k: v for k, v in env.items() if k not in ("tune", "grid_cap", "subpixel")}     # (a copy: the variant serves every shape)
        if hasattr(lib, "sgd_igemm_work_bytes"):            # balanced tail (tune=16 turns it off)
            wb = int(lib.sgd_igemm_work_bytes())
            if name not in WORK:
                WORK[name] = torch.zeros(wb // 4, device="cuda")
            q.work, q.work_bytes = WORK[name].data_ptr(), wb
        stt = None
        if a.stats and hasattr(lib, "sgd_igemm_stats_parts"):
            parts = int(lib.sgd_igemm_stats_parts(C.byref(q)))
            if parts > 0:
                stt = torch.full((n, parts, 2, cout), float("nan"), device="cuda")
                q.stats = stt.data_ptr()
        runs.append((name, lib, env, q, y, (buf, sinv, stt), []))

    def launch(lib, env, q, reps):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        for _ in range(reps):
            rc = lib.sgd_igemm(C.byref(q), st)
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
        return rc

    for name, lib, env, q, y, buf, ts in runs:
        L.check(launch(lib, env, q, 3), name)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, lib, env, q, y, buf, ts in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); launch(lib, env, q, a.reps); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / a.reps)
    fl = 2.0 * n * ho * ho * cout * cin * ks * ks          # (up: the direct conv's work -- fp32-equivalent for the sub-pixel form)
    ref = runs[0][4]
    line = f"n={n} cin={cin} cout={cout} hw={hw} ks={ks}{' up' if up else ''}:"
    for name, lib, env, q, y, buf, ts in runs:
        med, mn = statistics.median(ts), min(ts)
        diff = float((y - ref).abs().max() / ref.abs().max())
        same = lambda u, v: u.shape == v.shape and bool(torch.equal(u.view(torch.int32), v.view(torch.int32)))
        bits = "same" if same(y, ref) else "DIFF"
        if buf[2] is not None and runs[0][5][2] is not None:
            bits += " stats=" + ("same" if same(buf[2], runs[0][5][2]) else "DIFF")
        line += f"  {name} {med:.4f} ms ({fl / med / 1e9:.0f} TF, min {mn:.4f}, d={diff:.1e} bits={bits})"
    print(line, flush=True)
