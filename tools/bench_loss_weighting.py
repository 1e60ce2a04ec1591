#!/usr/bin/env python3
"""C2 training step (forward + backward + AdamW + EMA, synthetic data) with the weighted loss path (hparam loss_weighting:
sgd_loss_fwd / sgd_loss_bwd) and the default path (torch op chain) ALTERNATING in one process on one model, so that both see
the same device state and the same neighbours on the host.  Prints per-path best / median / worst over the rounds.
    python tools/bench_loss_weighting.py [--batch 40] [--prec f16x3] [--rounds 7] [--steps 5] [--par v] [--scheme min_snr] [--out FILE]"""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import torch
import bench
from sgdm_amd.diffusion import LatentDiffusion
from sgdm_amd.ema import LitEma

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=40); ap.add_argument("--prec", default="f16x3")
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--par", default="v"); ap.add_argument("--scheme", default="min_snr")
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about a step time"
dev = torch.device("cuda", 0)
m, sd, data = bench.build_model(bench.WORKLOADS["c2"], dev, a.prec, a.batch)
m.train()
params = dict(bench.MODEL_PARAMS, parameterization=a.par)
paths = {"default": LatentDiffusion(device="cuda", **params).train(),
         "weighted": LatentDiffusion(device="cuda", **dict(params, loss_weighting=a.scheme)).train()}
for d in paths.values():
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
ema = LitEma(m)
x, cond = data["image"].to(dev), data["cond"].to(dev)


def step(d):
    loss, _ = d.forward_tao(x, cond=cond, cond_drop_prob=0.1)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    ema(m)
    return loss


for d in paths.values():
    for _ in range(a.warmup):
        step(d)
ms = {k: [] for k in paths}
for r in range(a.rounds):
    for k in (("default", "weighted") if r % 2 == 0 else ("weighted", "default")):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            l = step(paths[k])
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
lines = [f"C2 training step, bs={a.batch} prec={a.prec} parameterization={a.par}, {a.rounds} rounds x {a.steps} steps per path, alternating"]
for k, v in ms.items():
    best, med = min(v), statistics.median(v)
    lines.append(f"{k:9s} ({'loss_weighting=' + a.scheme if k == 'weighted' else 'hparam absent'}): best {best:.2f} ms  median {med:.2f} ms  "
                 f"worst {max(v):.2f} ms  best-to-median spread {(med - best) / best * 100:.2f} %")
dm = statistics.median(ms["weighted"]) - statistics.median(ms["default"])
lines.append(f"weighted - default: {dm:+.3f} ms on the medians ({dm / statistics.median(ms['default']) * 100:+.2f} %), "
             f"{min(ms['weighted']) - min(ms['default']):+.3f} ms on the bests")
report = "\n".join(lines)
print(report)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(report + "\n")
