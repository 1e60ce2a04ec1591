#!/usr/bin/env python3
"""Wall clock of whole sampling trajectories at C2 (unet_fast ch128, 64x64, bs 40 -> UNet batch 80, w=2) through
LatentDiffusion.p_sample_loop on the captured step: DDIM-50, PNDM-50 (12 Runge-Kutta + 47 multistep evaluations),
DPM-Solver++(2M) at 20 steps and, for reference, native-1000 (`--native-reps 0` leaves it out).  Each trajectory: one untimed
run first (engine, packed weights, captured step), then `--reps` timed runs, synchronised, best and median kept.  Writes
profiles/dpmsolver_vs_ddim_c2.txt (profiles/pndm_vs_ddim_c2.txt is the recording of the tool before it had the dpmsolver leg).

`--parameterization eps v` runs every chosen sampler once per parameterization in the same process ('v': the UNet's output
read as v, one sgd_v_to_eps launch per evaluation inside the captured step) and adds a column against the first one named;
profiles/vpred_vs_eps_c2.txt is
    python tools/bench_samplers.py --methods ddim dpmsolver --parameterization eps v --reps 5 --out profiles/vpred_vs_eps_c2.txt

    python tools/bench_samplers.py [--prec f16x3] [--reps 3] [--native-reps 1] [--methods ...] [--parameterization ...]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", default="f16x3", choices=["f32", "f16x3", "bf16x3", "f16", "bf16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--native-reps", type=int, default=1)
    ap.add_argument("--methods", nargs="+", default=["ddim", "pndm", "dpmsolver", "native"],
                    choices=["ddim", "pndm", "dpmsolver", "native"])
    ap.add_argument("--parameterization", nargs="+", default=["eps"], choices=["eps", "v"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpmsolver_vs_ddim_c2.txt"))
    a = ap.parse_args()
    from sgdm_amd.diffusion import LatentDiffusion
    wl = bench.WORKLOADS["c2"]
    model, _, data = bench.build_model(wl, "cuda", a.prec)
    diffs = {}
    for par in a.parameterization:
        diffs[par] = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, parameterization=par))
        diffs[par].set_denoise_fn(model.forward, model.forward_with_cond_scale)
    B, S = wl["batch"], wl["image"]
    dkw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=2.0)
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(23)).cuda()
    rows = []
    legs = dict(ddim=(50, 50, a.reps), pndm=(50, 59, a.reps), dpmsolver=(20, 20, a.reps), native=(1000, 1000, a.native_reps))
    for method, par in ((m, p) for m in legs if m in a.methods for p in a.parameterization):
        steps, evals, reps = legs[method]
        diff = diffs[par]
        if reps < 1:
            continue
        skw = dict(sampling_method=method, vis=None, num_timesteps=steps, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True,
                   dtp=1, temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True,
                   disable_tqdm=True, hip_graph=True)
        run = lambda: diff.p_sample_loop(method, (B, 3, S, S), skw, denoise_sample_fn_kwargs=dict(dkw), condition_kwargs={},
                                         x_T=x_T)
        with torch.no_grad():
            if method == "native":      # warm-up: the captured step is built on the first of three visited steps
                diff.sampler.sample((B, 3, S, S), sampling_kwargs=skw, denoise_sample_fn=diff.denoise_sample_fn,
                                    denoise_sample_fn_kwargs=dict(dkw), x_T=x_T, step_indices=[999, 998, 997])
            else:
                run()
            torch.cuda.synchronize()
            secs = []
            for _ in range(reps):
                t0 = time.perf_counter()
                u8, _ = run()
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
        assert u8.dtype == torch.uint8
        if method == "dpmsolver":       # de-duplicated times would mean fewer evaluations than steps
            assert len(diff.sampler_list[method].plan(dict(skw, alphas_cumprod=diff.sampler.alphas_cumprod))[0]) == evals
        rows.append((method, steps, evals, min(secs), statistics.median(secs), len(secs), par))
        print(rows[-1], flush=True)
    ddim_ms = rows[0][3] * 1e3 / rows[0][2]
    many = len(a.parameterization) > 1
    first = {r[0]: r[3] for r in reversed(rows)}            # per sampler: best time of the first parameterization named
    lines = [f"# tools/bench_samplers.py: C2 = {wl['desc'].split(',')[0]}, precision {a.prec}, captured steps (hip_graph=True)",
             f"# device {torch.cuda.get_device_name(0)}; whole p_sample_loop calls (uint8 tail included), synchronised wall clock",
             f"{'sampler':10s} {'steps':>6s} {'UNet evals':>10s} {'s/trajectory (best)':>20s} {'median':>8s} {'runs':>5s} "
             f"{'ms/eval (best)':>15s} {'vs DDIM ms/eval':>16s}"]
    if many:
        lines[-1] += f" {'param':>6s} {'vs ' + a.parameterization[0]:>8s}"
    for method, steps, evals, best, med, n, par in rows:
        ms = best * 1e3 / evals
        lines.append(f"{method:10s} {steps:6d} {evals:10d} {best:20.3f} {med:8.3f} {n:5d} {ms:15.3f} {ms / ddim_ms - 1:+15.2%}")
        if many:
            lines[-1] += f" {par:>6s} {best / first[method] - 1:+8.2%}"
    lines.append("# best-to-median spread of s/trajectory: "
                 + ", ".join(f"{r[0]}{'/' + r[6] if many else ''} {r[4] / r[3] - 1:.2%}" for r in rows))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
