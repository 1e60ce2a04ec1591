#!/usr/bin/env python3
"""C2 training step (forward + backward + fused AdamW + EMA, synthetic data) with and without global-norm gradient clipping, the
four paths ALTERNATING in one process on one model and one optimizer, so that all see the same device state and the same
neighbours on the host:
  (a) none     no clipping (max_grad_norm absent: the launches of before)
  (b) fused    FusedAdamWEma(max_grad_norm): sgd_grad_norm + sgd_adamw_ema_clip_step, gradients not rewritten
  (c) torch    torch.nn.utils.clip_grad_norm_ on the parameters, then the plain step
  (d) ours     sgdm_amd.optim.clip_grad_norm_ (sgd_grad_norm + sgd_grad_scale in place), then the plain step
Prints per-path best / median / worst over the rounds, the differences to (a), and the norm launches timed alone.
    python tools/bench_grad_clip.py [--batch 40] [--prec f16x3] [--rounds 7] [--steps 5] [--max-norm 0.01] [--out FILE]"""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import torch
import bench
from sgdm_amd import _lib as L
from sgdm_amd import optim as O
from sgdm_amd.diffusion import LatentDiffusion
from sgdm_amd.ema import LitEma

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=40); ap.add_argument("--prec", default="f16x3")
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--max-norm", type=float, default=0.01, help="far below the gradient norm of this workload (~0.2): every step clips")
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about a step time"
dev = torch.device("cuda", 0)
m, sd, data = bench.build_model(bench.WORKLOADS["c2"], dev, a.prec, a.batch)
m.train()
d = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS).train()
d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
params = [p for p in m.parameters() if p.requires_grad]
ema = LitEma(m).to(dev)
opt = O.FusedAdamWEma(params, lr=1e-4, weight_decay=0.01, ema=ema, ema_model=m)
x, cond = data["image"].to(dev), data["cond"].to(dev)
PATHS = ("none", "fused", "torch", "ours")
LABEL = dict(none="(a) no clipping", fused="(b) fused max_grad_norm", torch="(c) torch clip_grad_norm_ + plain step",
             ours="(d) sgdm clip_grad_norm_ + plain step")


def step(kind):
    loss, _ = d.forward_tao(x, cond=cond, cond_drop_prob=0.1)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.max_grad_norm = a.max_norm if kind == "fused" else None
    if kind == "torch":
        torch.nn.utils.clip_grad_norm_(params, a.max_norm)
    elif kind == "ours":
        O.clip_grad_norm_(params, a.max_norm)
    opt.step()
    return loss


for k in PATHS:
    for _ in range(a.warmup):
        step(k)
ms = {k: [] for k in PATHS}
for r in range(a.rounds):
    order = PATHS[r % 4:] + PATHS[:r % 4]
    for k in (order if r % 2 == 0 else order[::-1]):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            step(k)
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
step("fused")
st = opt.clip_stats()
n_el = sum(p.grad.numel() for p in params if p.grad is not None)
lines = [f"C2 training step, bs={a.batch} prec={a.prec}, FusedAdamWEma + EMA, max_norm={a.max_norm}, {a.rounds} rounds x {a.steps} steps "
         f"per path, alternating",
         f"gradients: {sum(1 for p in params if p.grad is not None)} tensors, {n_el * 4 / 1e6:.1f} MB; last fused step: norm {st['norm']:.6g} "
         f"coef {st['coef']:.6g} (clipped steps so far {st['clipped_steps']}, non-finite {st['nonfinite_steps']})"]
for k, v in ms.items():
    best, med = min(v), statistics.median(v)
    lines.append(f"{LABEL[k]:40s}: best {best:.2f} ms  median {med:.2f} ms  worst {max(v):.2f} ms  "
                 f"best-to-median spread {(med - best) / best * 100:.2f} %")
base = statistics.median(ms["none"])
for k in PATHS[1:]:
    dm = statistics.median(ms[k]) - base
    lines.append(f"{k:5s} - none: {dm:+.3f} ms on the medians ({dm / base * 100:+.2f} %), {min(ms[k]) - min(ms['none']):+.3f} ms on the bests")
dm = statistics.median(ms["fused"]) - statistics.median(ms["torch"])
lines.append(f"fused - torch: {dm:+.3f} ms on the medians, {min(ms['fused']) - min(ms['torch']):+.3f} ms on the bests")

# the norm alone (sgd_grad_norm: both launches, table already on the device) and the in-place scale, by device events
lib = L.load()
grads = [p.grad for p in params if p.grad is not None]
rows = [(0, g.data_ptr(), 0, 0, 0, g.numel()) for g in grads]
start = O.chunk_table([r[5] for r in rows])
table = torch.tensor(rows, dtype=torch.int64).to(dev)
cstart = torch.tensor(start, dtype=torch.int32).to(dev)
part = torch.empty(start[-1], dtype=torch.float64, device=dev)
rec = torch.zeros(8, dtype=torch.int32, device=dev)
s = torch.cuda.current_stream().cuda_stream


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return min(out), statistics.median(out)


def norm(mx):
    L.check(lib.sgd_grad_norm(table.data_ptr(), cstart.data_ptr(), len(rows), start[-1], part.data_ptr(), mx, rec.data_ptr(), s), "norm")


def scale():
    L.check(lib.sgd_grad_scale(table.data_ptr(), cstart.data_ptr(), len(rows), start[-1], rec.data_ptr(), s), "scale")


b, md = timed(lambda: norm(float("inf")))
lines.append(f"sgd_grad_norm alone ({start[-1]} chunks): best {b:.1f} us  median {md:.1f} us  = {n_el * 4 / md / 1e6:.2f} TB/s of gradient bytes "
             f"on the median")
b, md = timed(scale)
lines.append(f"sgd_grad_scale, coef == 1 (every block returns): best {b:.1f} us  median {md:.1f} us")
keep = [g.clone() for g in grads]                   # a record with coef 0.999 written by hand; the gradients are put back below
rec[:2] = torch.tensor([1.0, 0.999], dtype=torch.float32).view(torch.int32).to(dev)
b, md = timed(scale)
for g, k in zip(grads, keep):
    g.copy_(k)
lines.append(f"sgd_grad_scale, coef < 1 (read + write): best {b:.1f} us  median {md:.1f} us  = {2 * n_el * 4 / md / 1e6:.2f} TB/s on the median")
report = "\n".join(lines)
print(report)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(report + "\n")
