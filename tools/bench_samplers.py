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

`--cfg-interval LO HI` (or `--cfg-middle FRAC`: per sampler, the interval that covers the middle FRAC of its evaluations)
and / or `--cfg-rescale PHI` time the guidance schedule instead (sampling kwargs cfg_interval / cfg_rescale): per sampler the
variants `guided` (no option: the fused step), `rescale` (guidance throughout + the guide launch), `interval` (cond-only
evaluations at batch B outside it) and `cond` (an interval that hits nothing: every evaluation cond-only), ALTERNATING within
each repetition in one process, so drift hits all of them alike; profiles/cfg_schedule_c2.txt is
    python tools/bench_samplers.py --methods ddim dpmsolver --cfg-middle 0.4 --cfg-rescale 0.7 --reps 5 --out profiles/cfg_schedule_c2.txt

`--v-form eps data` times the two forms of parameterization 'v' (sampling kwarg v_form: 'eps' = sgd_v_to_eps + the sampler's
own update kernel, 'data' = ONE sgd_v_step launch) per chosen sampler (ddim-50, dpmsolver-20), ALTERNATING within each
repetition in one process; `--zero-terminal-snr` builds the model's schedule with the hparam of that name (then only 'data'
can visit the last timestep) and `--spacing trailing` sets the sampling kwarg timestep_spacing; profiles/ztsnr_c2.txt is
    python tools/bench_samplers.py --methods ddim dpmsolver --parameterization v --v-form eps data --reps 5 --out profiles/ztsnr_c2.txt

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


def schedule_main(a, wl, model, data, diff, par):
    """the guidance-schedule variants of every chosen sampler, alternating (module docstring)"""
    from sgdm_amd.diffusion import cfg_schedule, make_ddim_timesteps
    B, S = wl["batch"], wl["image"]
    data_kw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=2.0)
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(23)).cuda()
    lines = [f"# tools/bench_samplers.py: C2 = {wl['desc'].split(',')[0]}, precision {a.prec}, parameterization {par}, captured steps",
             f"# device {torch.cuda.get_device_name(0)}; whole p_sample_loop calls (uint8 tail included), synchronised wall clock;",
             f"# per sampler the variants alternate within each of the {a.reps} repetitions (one untimed run of each first)",
             f"{'sampler':10s} {'variant':9s} {'interval':>11s} {'guided':>7s} {'cond':>5s} {'ms/trajectory (best)':>21s} {'median':>9s} "
             f"{'vs guided':>10s} {'ms/eval (best)':>15s}"]
    notes = []
    for method, steps in (("ddim", 50), ("dpmsolver", 20)):
        if method not in a.methods:
            continue
        skw = dict(sampling_method=method, vis=None, num_timesteps=steps, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True,
                   dtp=1, temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True,
                   disable_tqdm=True, hip_graph=True)
        if method == "ddim":
            times = [int(t) for t in make_ddim_timesteps("uniform", steps, 1000)]
        else:
            times = [int(t) for t in diff.sampler_list[method].plan(dict(skw, alphas_cumprod=diff.sampler.alphas_cumprod))[0]]
        E = len(times)
        if a.cfg_middle is not None:
            u = sorted(times)
            n_in = max(1, round(a.cfg_middle * E))
            lo = (E - n_in) // 2
            iv = (u[lo], u[lo + n_in - 1])
        else:
            iv = tuple(a.cfg_interval) if a.cfg_interval else None
        variants = [("guided", {})]
        if a.cfg_rescale:
            variants.append(("rescale", dict(cfg_rescale=a.cfg_rescale)))
        if iv is not None:
            variants += [("interval", dict(cfg_interval=iv)), ("cond", dict(cfg_interval=(0, 0)))]
            if a.cfg_rescale:
                variants.append(("both", dict(cfg_interval=iv, cfg_rescale=a.cfg_rescale)))
        secs = {name: [] for name, _ in variants}
        with torch.no_grad():
            for rep in range(a.reps + 1):               # (the first round is the untimed one: engines, captures)
                for name, opt in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    u8, _ = diff.p_sample_loop(method, (B, 3, S, S), dict(skw, **opt), denoise_sample_fn_kwargs=dict(data_kw),
                                               condition_kwargs={}, x_T=x_T)
                    torch.cuda.synchronize()
                    if rep:
                        secs[name].append(time.perf_counter() - t0)
                    assert u8.dtype == torch.uint8
        best = {k: min(v) * 1e3 for k, v in secs.items()}
        med = {k: statistics.median(v) * 1e3 for k, v in secs.items()}
        for name, opt in variants:
            flags = cfg_schedule(times, 2.0, model._scale_mode(), opt.get("cfg_interval"))[0]
            ng = sum(flags)
            ivs = "-" if "cfg_interval" not in opt else "%d..%d" % opt["cfg_interval"]
            lines.append(f"{method:10s} {name:9s} {ivs:>11s} {ng:7d} {E - ng:5d} {best[name]:21.2f} {med[name]:9.2f} "
                         f"{best[name] / best['guided'] - 1:+10.2%} {best[name] / E:15.3f}")
            print(lines[-1], flush=True)
        g = best["guided"] / E
        if "cond" in best:
            c = best["cond"] / E
            ng = sum(cfg_schedule(times, 2.0, model._scale_mode(), iv)[0])
            model_ms = ng * g + (E - ng) * c
            notes.append(f"# {method}: a cond-only evaluation (UNet at batch {B}) {c:.3f} ms against a guided one (batch {2 * B}) "
                         f"{g:.3f} ms: {c / g:.1%}; interval run {best['interval']:.1f} ms against {model_ms:.1f} ms = "
                         f"{ng} x guided + {E - ng} x cond-only")
        if "rescale" in best:
            notes.append(f"# {method}: the guide launch (rescale {a.cfg_rescale}) costs {(best['rescale'] - best['guided']) / E:+.3f} ms per "
                         f"evaluation (best against best; medians {(med['rescale'] - med['guided']) / E:+.3f})")
        notes.append(f"# {method}: best-to-median spread of ms/trajectory: "
                     + ", ".join(f"{k} {med[k] / best[k] - 1:.2%}" for k in best))
    text = "\n".join(lines + notes) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


def forms_main(a, wl, model, data):
    """the forms of 'v' of every chosen sampler, alternating (module docstring)"""
    from sgdm_amd.diffusion import LatentDiffusion
    hp = dict(bench.MODEL_PARAMS, parameterization="v", **(dict(zero_terminal_snr=True) if a.zero_terminal_snr else {}))
    diff = LatentDiffusion(device="cuda", **hp)
    diff.set_denoise_fn(model.forward, model.forward_with_cond_scale)
    B, S = wl["batch"], wl["image"]
    data_kw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=2.0)
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(23)).cuda()
    lines = [f"# tools/bench_samplers.py: C2 = {wl['desc'].split(',')[0]}, precision {a.prec}, parameterization v, captured steps,",
             f"# zero_terminal_snr {a.zero_terminal_snr}, timestep_spacing {a.spacing}",
             f"# device {torch.cuda.get_device_name(0)}; whole p_sample_loop calls (uint8 tail included), synchronised wall clock;",
             f"# per sampler the forms alternate within each of the {a.reps} repetitions (one untimed run of each first)",
             f"{'sampler':10s} {'v_form':>6s} {'steps':>6s} {'UNet evals':>10s} {'ms/trajectory (best)':>21s} {'median':>9s} "
             f"{'vs ' + a.v_form[0]:>8s} {'ms/eval (best)':>15s} {'launches/eval after the UNet':>29s}"]
    notes = []
    for method, steps in (("ddim", 50), ("dpmsolver", 20)):
        if method not in a.methods:
            continue
        skw = dict(sampling_method=method, vis=None, num_timesteps=steps, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True,
                   dtp=1, temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True,
                   disable_tqdm=True, hip_graph=True, timestep_spacing=a.spacing)
        if method == "dpmsolver" and a.spacing == "trailing":
            skw["dpm_spacing"] = "uniform"              # (the spacing kwarg is honoured by the uniform table; logsnr has its own)
        E = steps if method == "ddim" else len(diff.sampler_list[method].plan(
            dict(skw, alphas_cumprod=diff.sampler.alphas_cumprod), "data")[0])
        secs = {form: [] for form in a.v_form}
        with torch.no_grad():
            for rep in range(a.reps + 1):               # (the first round is the untimed one: engines, captures)
                for form in a.v_form:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    u8, _ = diff.p_sample_loop(method, (B, 3, S, S), dict(skw, v_form=form), denoise_sample_fn_kwargs=dict(data_kw),
                                               condition_kwargs={}, x_T=x_T)
                    torch.cuda.synchronize()
                    if rep:
                        secs[form].append(time.perf_counter() - t0)
                    assert u8.dtype == torch.uint8
        best = {k: min(v) * 1e3 for k, v in secs.items()}
        med = {k: statistics.median(v) * 1e3 for k, v in secs.items()}
        for form in a.v_form:
            lines.append(f"{method:10s} {form:>6s} {steps:6d} {E:10d} {best[form]:21.2f} {med[form]:9.2f} "
                         f"{best[form] / best[a.v_form[0]] - 1:+8.2%} {best[form] / E:15.3f} {2 if form == 'eps' else 1:29d}")
            print(lines[-1], flush=True)
        if len(a.v_form) > 1:
            f0, f1 = a.v_form[0], a.v_form[1]
            notes.append(f"# {method}: {f1} against {f0}: {(best[f1] - best[f0]) / E:+.4f} ms per evaluation best against best, "
                         f"{(med[f1] - med[f0]) / E:+.4f} median against median")
        notes.append(f"# {method}: best-to-median spread of ms/trajectory: "
                     + ", ".join(f"{k} {med[k] / best[k] - 1:.2%}" for k in best))
    text = "\n".join(lines + notes) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", default="f16x3", choices=["f32", "f16x3", "bf16x3", "f16", "bf16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--native-reps", type=int, default=1)
    ap.add_argument("--methods", nargs="+", default=["ddim", "pndm", "dpmsolver", "native"],
                    choices=["ddim", "pndm", "dpmsolver", "native"])
    ap.add_argument("--parameterization", nargs="+", default=["eps"], choices=["eps", "v"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpmsolver_vs_ddim_c2.txt"))
    ap.add_argument("--cfg-interval", nargs=2, type=int, metavar=("LO", "HI"), default=None)
    ap.add_argument("--cfg-middle", type=float, default=None, metavar="FRAC")
    ap.add_argument("--cfg-rescale", type=float, default=0.0, metavar="PHI")
    ap.add_argument("--zero-terminal-snr", action="store_true")
    ap.add_argument("--spacing", default="leading", choices=["leading", "trailing"])
    ap.add_argument("--v-form", nargs="+", default=["eps"], choices=["eps", "data"])
    a = ap.parse_args()
    from sgdm_amd.diffusion import LatentDiffusion
    wl = bench.WORKLOADS["c2"]
    model, _, data = bench.build_model(wl, "cuda", a.prec)
    if a.v_form != ["eps"] or a.zero_terminal_snr or a.spacing != "leading":
        if a.parameterization != ["v"]:
            ap.error("--v-form / --zero-terminal-snr / --spacing time parameterization 'v': pass --parameterization v")
        return forms_main(a, wl, model, data)
    diffs = {}
    for par in a.parameterization:
        diffs[par] = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, parameterization=par))
        diffs[par].set_denoise_fn(model.forward, model.forward_with_cond_scale)
    if a.cfg_interval or a.cfg_middle is not None or a.cfg_rescale:
        return schedule_main(a, wl, model, data, diffs[a.parameterization[0]], a.parameterization[0])
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
