#!/usr/bin/env python3
"""Guidance distillation at C2 (unet_fast ch128, 64x64, f16x3), one process, the variants of each part ALTERNATING within every
round so that drift hits all of them alike; writes profiles/distill_c2.txt.

(a) the training step (forward + backward + AdamW + EMA, synthetic data, bs 40):
      plain       the hparam absent
      distill     hparam distill_guidance = 2, teacher in the student's arithmetic mode: one more inference evaluation at 2B and
                  the fused loss kernels (sgd_distill_loss_fwd / sgd_distill_loss_bwd)
      distill_f16 the same with an 'f16' teacher (single-product inference mode)
      by_hand     what a user would write without the feature: teacher.forward_with_cond_scale under no_grad as the target of
                  _MSEFn (one combine launch, the target tensor, the torch op chain)
    and, for the expected cost, the teacher's doubled inference evaluation alone.
(b) whole trajectories through p_sample_loop on the captured step, DDIM-50 and DPM-Solver++(2M)-20 (bs 40):
      teacher     cond_scale = 2: the UNet at 2B per step
      student     cfg_distilled: the UNet at B per step, the 2B engine never built (a model of its own)
No trained model exists here: the numbers are step times, the sample quality of a distilled student has NOT been measured.
(The no-regression lines at the end of the recorded profile are bench.py runs of the parent and of this tree, appended to it.)

    python tools/bench_distill.py [--batch 40] [--prec f16x3] [--rounds 5] [--steps 5] [--out profiles/distill_c2.txt]"""
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
from sgdm_amd.losses import _MSEFn, distill_teacher_from  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=40)
ap.add_argument("--prec", default="f16x3")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_c2.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about a step time"
dev = torch.device("cuda", 0)
W = 2.0
wl = bench.WORKLOADS["c2"]
B, S = a.batch, wl["image"]


def row(name, note, v):
    best, med = min(v), statistics.median(v)
    return f"{name:12s} {note:52s} best {best:9.2f} ms  median {med:9.2f} ms  best-to-median spread {(med - best) / best * 100:5.2f} %"


lines = [f"# tools/bench_distill.py: C2 = {wl['desc'].split(',')[0]}, bs {B}, precision {a.prec}, guidance weight {W}; device "
         f"{torch.cuda.get_device_name(0)}",
         f"# one process; {a.rounds} rounds, the variants of a part alternating within each round (order reversed every other "
         "round), synchronised wall clock",
         "# sample quality of a distilled student has NOT been measured: there is no trained model here"]

# ------------------------------------------------------------------------------------------------------------- (a) training
m, sd, data = bench.build_model(wl, dev, a.prec, B)
m.train()
teachers = {"distill": distill_teacher_from(m), "distill_f16": distill_teacher_from(m, hip_precision="f16")}
paths = {"plain": LatentDiffusion(device="cuda", **bench.MODEL_PARAMS).train()}
for k, t in teachers.items():
    paths[k] = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, distill_guidance=W)).train()
    paths[k].set_distill_teacher(t)
for d in paths.values():
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
ema = LitEma(m)
x, cond = data["image"].to(dev), data["cond"].to(dev)
sampler = paths["plain"].sampler


def by_hand():
    """the distillation loss with today's public pieces"""
    t = torch.randint(0, 1000, (B,), device=dev).long()
    x_noisy = sampler.q_sample(original_sample=x, t=t, noise=torch.randn_like(x))
    with torch.no_grad():
        target = teachers["distill"].forward_with_cond_scale(x_noisy, t, W, cond=cond)
    out = m.forward(x_noisy, t, cond=cond, cond_drop_prob=0.0)[0]
    return _MSEFn.apply(out, target).mean()


def step(name):
    loss = by_hand() if name == "by_hand" else paths[name].forward_tao(x, cond=cond, cond_drop_prob=0.1)[0]
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    ema(m)
    return loss


def teacher_eval(name):
    t = torch.randint(0, 1000, (B,), device=dev).long()
    with torch.no_grad():
        teachers[name].forward_with_cond_scale(x, t, W, cond=cond)


def timed(fn, arg, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn(arg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


names = ["plain", "distill", "distill_f16", "by_hand"]
for k in names:
    timed(step, k, a.warmup)
for k in teachers:
    timed(teacher_eval, k, a.warmup)
ms, ev = {k: [] for k in names}, {k: [] for k in teachers}
for r in range(a.rounds):
    for k in (names if r % 2 == 0 else names[::-1]):
        ms[k].append(timed(step, k, a.steps))
    for k in teachers:
        ev[k].append(timed(teacher_eval, k, a.steps))
notes = dict(plain="hparam absent", distill=f"distill_guidance={W}, teacher {a.prec}", distill_f16=f"distill_guidance={W}, teacher f16",
             by_hand="forward_with_cond_scale + _MSEFn")
lines.append(f"# (a) training step, {a.steps} steps per timing")
lines += [row(k, notes[k], ms[k]) for k in names]
lines += [row("eval_" + k.replace("distill", "2B"), f"teacher forward_with_cond_scale alone, {teachers[k].hip_precision}", ev[k])
          for k in teachers]
med = {k: statistics.median(v) for k, v in {**ms, **{"eval_" + k: v for k, v in ev.items()}}.items()}
lines.append(f"# distill - plain: {med['distill'] - med['plain']:+.2f} ms on the medians ({(med['distill'] / med['plain'] - 1) * 100:+.1f} %); "
             f"one doubled inference evaluation alone: {med['eval_distill']:.2f} ms")
lines.append(f"# distill_f16 - plain: {med['distill_f16'] - med['plain']:+.2f} ms ({(med['distill_f16'] / med['plain'] - 1) * 100:+.1f} %); "
             f"its evaluation alone: {med['eval_distill_f16']:.2f} ms")
lines.append(f"# distill - by_hand: {med['distill'] - med['by_hand']:+.2f} ms on the medians")
print("\n".join(lines), flush=True)
del opt, ema, paths, teachers
m.zero_grad(set_to_none=True)
m._engines.clear()
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------------------- (b) sampling
models = {"teacher": bench.build_model(wl, dev, a.prec, B)[0], "student": bench.build_model(wl, dev, a.prec, B)[0]}
diffs = {}
for k, mod in models.items():
    diffs[k] = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, guidance_distilled=(k == "student")))
    diffs[k].set_denoise_fn(mod.forward, mod.forward_with_cond_scale)
x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(23)).cuda()
dkw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=W)
lines.append("# (b) whole p_sample_loop calls (uint8 tail included) on the captured step; one untimed run of each first")
for method, steps in (("ddim", 50), ("dpmsolver", 20)):
    skw = dict(sampling_method=method, vis=None, num_timesteps=steps, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True, dtp=1,
               temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True, disable_tqdm=True,
               hip_graph=True)

    def traj(k):
        with torch.no_grad():
            u8, _ = diffs[k].p_sample_loop(method, (B, 3, S, S), dict(skw), denoise_sample_fn_kwargs=dict(dkw), condition_kwargs={},
                                           x_T=x_T)
        assert u8.dtype == torch.uint8

    secs = {k: [] for k in models}
    for r in range(a.rounds + 1):                       # (the first round is the untimed one: engines, captures)
        for k in (list(models) if r % 2 == 0 else list(models)[::-1]):
            v = timed(traj, k, 1)
            if r:
                secs[k].append(v)
    for k in models:
        note = f"{method}-{steps}: " + ("cond_scale=2, UNet at 2B" if k == "teacher" else "cfg_distilled, UNet at B")
        lines.append(row(k, note, secs[k]))
    bt, bs = min(secs["teacher"]), min(secs["student"])
    lines.append(f"# {method}-{steps}: student / teacher = {bs / bt:.3f} on the bests, "
                 f"{statistics.median(secs['student']) / statistics.median(secs['teacher']):.3f} on the medians")
keys = sorted(models["student"]._engines)
assert all(k[0] == B for k in keys), keys
lines.append(f"# engines of the student model after both samplers: {keys} (no batch-{2 * B} engine or workspace)")
report = "\n".join(lines)
print(report)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(report + "\n")
