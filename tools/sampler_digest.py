#!/usr/bin/env python3
"""SHA-256 of the final sample and of every snapshot tensor of a fixed, seeded list of sampler runs on the ch-32 16x16 test
models, one line per tensor.  Two trees that print the same lines compute the same bytes: run it on both sides of a change
to the sampling loops.  Public entry points only (``sampler.sample``).  (tools only)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import torch
import bench
from sgdm_amd.diffusion import LatentDiffusion
from sgdm_amd.synth import synth_batch, weights_from_seed
from sgdm_amd.unet import UNetModel, UNetModelCA

B, S = 2, 16
INDEX = json.load(open(os.path.join(ROOT, "tests", "golden", "unet_index.json")))


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def model_and_guidance(name):
    entry = INDEX[name]
    kw = dict(entry["ctor"])
    cond = AttrDict(scale_type="imagen")
    if entry["layout_dim"]:
        cond[kw["condition_method"]] = AttrDict(layout_dim=entry["layout_dim"])
    m = (UNetModel if entry["kind"] == "unet_fast" else UNetModelCA)(condition=cond, **kw)
    m.load_state_dict(weights_from_seed(entry["manifest"], entry["seed"]))
    m = m.cuda().eval()
    m.hip_precision = "f16x3"
    batch = synth_batch(kw["condition_method"], B, S, kw["cond_dim"], entry["layout_dim"], seed=23)
    c = batch["cond"].cuda() if entry["kind"] == "unet_fast" else batch["cond"].float().cuda()
    return m, dict(cond=c, layout=batch["layout"].cuda() if "layout" in batch else None, cond_scale=2.0)


def skw(steps, **kw):
    return dict(dict(vis=None, num_timesteps=steps, ddim_eta=1.0, log_num_per_prog=10, clip_denoised=True, dtp=1,
                     temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True), **kw)


def run(tag, diff, method, sk, dkw, **extra):
    torch.manual_seed(1234)
    sk = dict(sk, sampling_method=method, alphas_cumprod=diff.sampler.alphas_cumprod)
    with torch.no_grad():
        img, inter = diff.sampler_list[method].sample(shape=(B, 3, S, S), sampling_kwargs=sk, denoise_sample_fn=diff.denoise_sample_fn,
                                                      denoise_sample_fn_kwargs=dict(dkw), **extra)
    for key, t in [("sample", img)] + sorted(inter.items()):
        t = t.detach().cpu().contiguous()
        print(f"{tag} {key} {tuple(t.shape)} {hashlib.sha256(t.numpy().tobytes()).hexdigest()}", flush=True)


def main():
    print("sampling loops of", sys.modules[LatentDiffusion.__module__].__file__, file=sys.stderr)
    for name in ("uf_label_c32_s16", "ca_stego_c32_s16"):
        m, dkw = model_and_guidance(name)
        diff = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS)
        diff.set_denoise_fn(m.forward, m.forward_with_cond_scale)
        short = dict(step_indices=[999, 888, 777, 500, 111, 1, 0])      # 888, 777, 111 and 0 are snapshot steps
        for graph in (False, True):
            g = "graph" if graph else "eager"
            run(f"{name} native-short {g}", diff, "native", skw(1000, hip_graph=graph), dkw, **short)
            run(f"{name} ddim-10 {g}", diff, "ddim", skw(10, hip_graph=graph), dkw)
            run(f"{name} pndm-10 {g}", diff, "pndm", skw(10, hip_graph=graph), dkw)
            run(f"{name} dpmsolver-10 {g}", diff, "dpmsolver", skw(10, hip_graph=graph), dkw)
        run(f"{name} plms-10 eager", diff, "plms", skw(10), dkw)
        # eager only: what the captured step leaves out
        x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(8)) * 1.7
        for method, sk, extra in (("native", skw(1000), short), ("ddim", skw(10), {}), ("plms", skw(10), {})):
            run(f"{name} {method} dtp=0.9", diff, method, dict(sk, dtp=0.9), dkw, x_T=x_T.clone(), **extra)
            run(f"{name} {method} noise_dropout=0.25", diff, method, dict(sk, noise_dropout=0.25), dkw, **extra)
        for graph in (False, True):
            run(f"{name} native temperature-list {'graph' if graph else 'eager'}", diff, "native",
                skw(1000, temperature=[0.5 + 0.0005 * i for i in range(1000)], hip_graph=graph), dkw, **short)
        x0p = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, parameterization="x0"))
        x0p.set_denoise_fn(m.forward, m.forward_with_cond_scale)
        for graph in (False, True):
            run(f"{name} native parameterization=x0 {'graph' if graph else 'eager'}", x0p, "native",
                skw(1000, hip_graph=graph), dkw, **short)
        # parameterization 'v': the v -> eps pass in front of the update, eager and captured (a direct sampler call names the
        # parameterization and the schedule's two tables in its kwargs)
        vp = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, parameterization="v"))
        vp.set_denoise_fn(m.forward, m.forward_with_cond_scale)
        vk = dict(parameterization="v", sqrt_alphas_cumprod=vp.sampler.sqrt_alphas_cumprod,
                  sqrt_one_minus_alphas_cumprod=vp.sampler.sqrt_one_minus_alphas_cumprod)
        for graph in (False, True):
            for method in ("ddim", "dpmsolver"):
                run(f"{name} {method}-10 parameterization=v {'graph' if graph else 'eager'}", vp, method,
                    skw(10, hip_graph=graph, **vk), dkw)
        # a plain callable: the generic path (guided NCHW eps from the function, cfg_mode 0), never captured
        plain = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS)
        plain.set_denoise_fn(m.forward, lambda x, t, **kw: m.forward_with_cond_scale(x, t, **kw))
        for method, sk, extra in (("native", skw(1000), short), ("ddim", skw(10), {}), ("plms", skw(10), {}),
                                  ("pndm", skw(10), {}), ("dpmsolver", skw(10), {}), ("ddim", skw(10, dtp=0.9), {})):
            run(f"{name} {method} plain-callable dtp={sk['dtp']}", plain, method, sk, dkw, **extra)


if __name__ == "__main__":
    main()
