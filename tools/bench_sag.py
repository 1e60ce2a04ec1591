#!/usr/bin/env python3
"""Wall clock of DDIM-50 trajectories at C2 (unet_fast ch128, 64x64, bs 40, f16x3) through LatentDiffusion.p_sample_loop on
the captured step under two guidance forms: CFG (cond_scale 2: one evaluation at UNet batch 80 per step) and self-attention
guidance on the middle attention (`sag_scale`: two dependent evaluations at batch 40 per step, the attention-mass and degrade
launches between them, one graph).  One process; one untimed run of each first (engines, packed weights, captures), then the
two ALTERNATE within each of `--reps` repetitions, so drift hits both alike; synchronised wall clock, best and median kept.

Then the two new launches of a SAG evaluation (sgd_attention_colmass, sgd_sag_degrade), launched eagerly on the captured step's
own buffers with a HIP event pair around each (best of `--profile-reps` passes).

`--cfg-only` times the CFG trajectories alone and prints one line: the figure to compare between two builds.

Writes profiles/sag_c2.txt.

    python tools/bench_sag.py [--prec f16x3] [--reps 5] [--scale 0.75] [--out profiles/sag_c2.txt] [--cfg-only]
"""
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

STEPS = 50


def sag_launches(diff, model, dkw, sk, reps):
    """{entry: best ms} of the two launches between the evaluations of a SAG step, on the cached captured step's buffers"""
    from sgdm_amd import diffusion as Dm
    step = next(s for s in model.__dict__["_hip_graph_steps"].values() if getattr(s, "sag", None))
    sk = dict(sk, alphas_cumprod=diff.sampler.alphas_cumprod, parameterization=diff.hparams.parameterization)
    runner = Dm._StepRunner(diff.denoise_sample_fn, dkw, sk, step.img.device)
    lib, best = runner.lib, {}
    originals = {name: getattr(lib, name) for name in ("sgd_attention_colmass", "sgd_sag_degrade")}

    def timed(name):
        def call(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = originals[name](*args)
            e1.record()
            e1.synchronize()
            best[name] = min(e0.elapsed_time(e1), best.get(name, float("inf")))
            return rc
        return call
    try:
        for name in originals:
            setattr(lib, name, timed(name))
        for _ in range(reps):
            runner.sag_degrade(step.eng, step.img, step.t, step.pair, step.x_deg, step.mass,
                               torch.cuda.current_stream().cuda_stream, step.tabs, step.taps)
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", default="f16x3", choices=["f32", "f16x3", "bf16x3", "f16", "bf16"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=0.75)
    ap.add_argument("--cfg-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sag_c2.txt"))
    a = ap.parse_args()
    from sgdm_amd.diffusion import LatentDiffusion
    wl = bench.WORKLOADS["c2"]
    model, _, data = bench.build_model(wl, "cuda", a.prec)
    diff = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS)
    diff.set_denoise_fn(model.forward, model.forward_with_cond_scale)
    B, S = wl["batch"], wl["image"]
    dkw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=2.0)
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(23)).cuda()
    skw = dict(sampling_method="ddim", vis=None, num_timesteps=STEPS, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True, dtp=1,
               temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True, disable_tqdm=True,
               hip_graph=True)
    variants = [("cfg", {})] + ([] if a.cfg_only else [("sag", dict(sag_scale=a.scale))])
    secs = {name: [] for name, _ in variants}
    with torch.no_grad():
        for rep in range(a.reps + 1):                   # (the first round is the untimed one: engines, captures)
            for name, opt in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                u8, _ = diff.p_sample_loop("ddim", (B, 3, S, S), dict(skw, **opt), denoise_sample_fn_kwargs=dict(dkw),
                                           condition_kwargs={}, x_T=x_T)
                torch.cuda.synchronize()
                if rep:
                    secs[name].append(time.perf_counter() - t0)
                assert u8.dtype == torch.uint8
    best = {k: min(v) * 1e3 for k, v in secs.items()}
    med = {k: statistics.median(v) * 1e3 for k, v in secs.items()}
    if a.cfg_only:
        print(f"cfg DDIM-{STEPS} C2 {a.prec}: ms/trajectory best {best['cfg']:.2f} median {med['cfg']:.2f} "
              f"all {' '.join(f'{v * 1e3:.2f}' for v in secs['cfg'])}")
        return
    with torch.no_grad():
        new = sag_launches(diff, model, dkw, dict(skw, sag_scale=a.scale), a.profile_reps)
    layer = next(s for s in model.__dict__["_hip_graph_steps"].values() if getattr(s, "sag", None)).sag[1]
    lines = [f"# tools/bench_sag.py: C2 = {wl['desc'].split(',')[0]}, precision {a.prec}, DDIM-{STEPS}, captured steps, sag_scale {a.scale}, "
             f"sag_layer {layer}",
             f"# device {torch.cuda.get_device_name(0)}; whole p_sample_loop calls (uint8 tail included), synchronised wall clock;",
             f"# the two forms alternate within each of the {a.reps} repetitions (one untimed run of each first)",
             f"# cfg: one evaluation at UNet batch {2 * B} per step; sag: two dependent evaluations at batch {B}, one graph",
             f"{'guidance':9s} {'ms/trajectory (best)':>21s} {'median':>9s} {'spread':>7s} {'vs cfg':>8s} {'ms/step (best)':>15s}"]
    for name, _ in variants:
        lines.append(f"{name:9s} {best[name]:21.2f} {med[name]:9.2f} {med[name] / best[name] - 1:7.2%} {best[name] / best['cfg'] - 1:+8.2%} "
                     f"{best[name] / STEPS:15.3f}")
    lines.append("# every repetition, ms/trajectory: " + "; ".join(f"{k} " + " ".join(f"{v * 1e3:.2f}" for v in vs) for k, vs in secs.items()))
    lines.append("# the two new launches of a SAG evaluation, ms (best of %d event-timed eager passes; launched one by one, so each "
                 "includes the launch gap a captured step does not pay):" % a.profile_reps)
    for name, ms in new.items():
        lines.append(f"{name:34s} {ms:9.4f}")
    lines.append(f"# both: {sum(new.values()):.4f} ms per evaluation = {sum(new.values()) / (best['sag'] / STEPS):.2%} of a SAG step")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
