#!/usr/bin/env python3
"""Progressive distillation at C2 (unet_fast ch128, 64x64), one process, the variants of each part ALTERNATING within every round
so that drift hits all of them alike; writes profiles/progressive_c2.txt.

(a) the training step (forward + backward + AdamW + EMA, synthetic data, bs 40), the student in --prec:
      plain        the hparam absent: the plain training step
      pd_guided    progressive_steps = 4 and distill_guidance = 2 (stages 1 and 2 in one): two inference evaluations of the teacher
                   at 2B, sgd_pd_half_step between them, sgd_pd_loss_fwd / sgd_pd_loss_bwd
      pd_one       progressive_steps = 4 alone: the teacher is a distilled model already, two evaluations at B
      *_f16        the same with an 'f16' teacher (single-product inference mode)
    and, with --prec f32 as well (the exact-fp32 student, --prec2), the same five.
(b) whole trajectories through p_sample_loop on the captured step (bs 40):
      ddim50       DDIM-50, cond_scale = 2: the UNet at 2B per step
      k4           a model with progressive_steps = 4 and no step kwargs: 4 trailing DDIM steps, the UNet at B per step
      k8           8 trailing cfg_distilled DDIM steps by sampling kwargs (1000 % 16 != 0: K = 8 is no admissible progressive_steps
                   on the 1000-step schedule; a student of 800 or 1600 timesteps would walk this grid by default)
No trained model exists here: the numbers are step times, the sample quality of a student has NOT been measured.

    python tools/bench_progressive.py [--batch 40] [--prec f16x3] [--prec2 f32] [--rounds 5] [--steps 5]
                                      [--out profiles/progressive_c2.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
from sgdm_amd.diffusion import LatentDiffusion  # noqa: E402
from sgdm_amd.ema import LitEma  # noqa: E402
from sgdm_amd.losses import distill_teacher_from  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=40)
ap.add_argument("--prec", default="f16x3")
ap.add_argument("--prec2", default="f32", help="a second student / teacher arithmetic mode for part (a); '' skips it")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive_c2.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about a step time"
dev = torch.device("cuda", 0)
W, K = 2.0, 4
wl = bench.WORKLOADS["c2"]
B, S = a.batch, wl["image"]


def row(name, note, v):
    best, med = min(v), statistics.median(v)
    return f"{name:14s} {note:58s} best {best:9.2f} ms  median {med:9.2f} ms  best-to-median spread {(med - best) / best * 100:5.2f} %"


def timed(fn, arg, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn(arg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


lines = [f"# tools/bench_progressive.py: C2 = {wl['desc'].split(',')[0]}, bs {B}, guidance weight {W}, progressive_steps {K}; device "
         f"{torch.cuda.get_device_name(0)}",
         f"# one process; {a.rounds} rounds, the variants of a part alternating within each round (order reversed every other "
         "round), synchronised wall clock",
         "# sample quality of a progressively distilled student has NOT been measured: there is no trained model here"]


# ------------------------------------------------------------------------------------------------------------- (a) training
def training(prec):
    m, sd, data = bench.build_model(wl, dev, prec, B)
    m.train()
    teachers = {"": distill_teacher_from(m), "_f16": distill_teacher_from(m, hip_precision="f16")}
    paths = {"plain": LatentDiffusion(device="cuda", **bench.MODEL_PARAMS).train()}
    for suffix, t in teachers.items():
        for name, hp in (("pd_guided", dict(distill_guidance=W)), ("pd_one", {})):
            d = paths[name + suffix] = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, progressive_steps=K, **hp)).train()
            d.set_distill_teacher(t)
    for d in paths.values():
        d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
    ema = LitEma(m)
    x, cond = data["image"].to(dev), data["cond"].to(dev)

    def step(name):
        loss = paths[name].forward_tao(x, cond=cond, cond_drop_prob=0.1)[0]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        ema(m)
        return loss

    names = list(paths)
    for k in names:
        timed(step, k, a.warmup)
    ms = {k: [] for k in names}
    for r in range(a.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms[k].append(timed(step, k, a.steps))
    notes = dict(plain="hparam absent")
    for suffix, t in teachers.items():
        notes["pd_guided" + suffix] = f"progressive_steps={K}, distill_guidance={W}, teacher {t.hip_precision}: 2 x 2B"
        notes["pd_one" + suffix] = f"progressive_steps={K}, teacher {t.hip_precision}: 2 x B"
    out = [f"# (a) training step, student {prec}, {a.steps} steps per timing"]
    out += [row(k, notes[k], ms[k]) for k in names]
    med = {k: statistics.median(v) for k, v in ms.items()}
    out += [f"# {k} - plain: {med[k] - med['plain']:+.2f} ms on the medians ({(med[k] / med['plain'] - 1) * 100:+.1f} %)"
            for k in names[1:]]
    print("\n".join(out), flush=True)
    del opt, ema, paths, teachers
    m.zero_grad(set_to_none=True)
    m._engines.clear()
    torch.cuda.empty_cache()
    return out, data


for prec in [p for p in (a.prec, a.prec2) if p]:
    part, data = training(prec)
    lines += part

# ------------------------------------------------------------------------------------------------------------- (b) sampling
hps = {"ddim50": {}, "k8": {}, "k4": dict(progressive_steps=4)}
models, diffs = {}, {}
for k, hp in hps.items():
    models[k] = bench.build_model(wl, dev, a.prec, B)[0]
    diffs[k] = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, **hp))
    diffs[k].set_denoise_fn(models[k].forward, models[k].forward_with_cond_scale)
x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(23)).cuda()
dkw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=W)
base = dict(sampling_method="ddim", vis=None, log_num_per_prog=10, clip_denoised=True, dtp=1, temperature=1.0, noise_dropout=0,
            random_sample_condition=False, return_inter_dict=True, disable_tqdm=True, hip_graph=True)
skw = dict(ddim50=dict(base, num_timesteps=50, ddim_eta=0.0), k4=dict(base),
           k8=dict(base, num_timesteps=8, ddim_eta=0.0, timestep_spacing="trailing", cfg_distilled=True))
lines.append(f"# (b) whole p_sample_loop calls (uint8 tail included) on the captured step, {a.prec}; one untimed run of each first")


def traj(k):
    with torch.no_grad():
        u8, _ = diffs[k].p_sample_loop("ddim", (B, 3, S, S), dict(skw[k]), denoise_sample_fn_kwargs=dict(dkw), condition_kwargs={},
                                       x_T=x_T)
    assert u8.dtype == torch.uint8


secs = {k: [] for k in hps}
for r in range(a.rounds + 1):                           # (the first round is the untimed one: engines, captures)
    for k in (list(hps) if r % 2 == 0 else list(hps)[::-1]):
        v = timed(traj, k, 1)
        if r:
            secs[k].append(v)
notes = dict(ddim50="ddim-50, cond_scale=2, UNet at 2B", k8="8 trailing cfg_distilled DDIM steps (kwargs), UNet at B",
             k4="progressive_steps=4: 4 trailing DDIM steps, UNet at B")
lines += [row(k, notes[k], secs[k]) for k in hps]
for k in ("k8", "k4"):
    lines.append(f"# {k} / ddim50 = {min(secs[k]) / min(secs['ddim50']):.4f} on the bests, "
                 f"{statistics.median(secs[k]) / statistics.median(secs['ddim50']):.4f} on the medians")
    keys = sorted(models[k]._engines)
    assert all(e[0] == B for e in keys), keys
    lines.append(f"# engines of the {k} model: {keys} (no batch-{2 * B} engine or workspace)")
report = "\n".join(lines)
print(report)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(report + "\n")
