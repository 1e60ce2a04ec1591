"""Child process of tests/test_hip_grad_clip_world1.py: the clipped optimizer step behind the data-parallel backward, on a
world-size-1 ``nccl`` (= RCCL) process group with the exchange forced (``hip_force_exchange``).

The ch-32, 16x16, batch-4 model, one training step, twice on the same inputs:
  A. the plain single-process backward (``hip_ddp = False``, no arena) and a measuring step (max_grad_norm = inf, lr = 0), and
  B. the data-parallel backward (gradient arena, bucketed all-reduce on the side stream) and a clipped step.
The gradients of the two are bit-equal and the norm's reduction order depends on the table alone -- the list of n -- so the
record's norm must carry the same BITS; the arena's health slot is no row of the table.  p.grad still aliases the arena afterwards
(the clip multiplies as it loads and never rewrites a gradient).  Prints one JSON line; the parent asserts on it.
"""
import json
import os
import struct
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-guided-diffusion-models_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def _hex(x):
    return struct.pack("<f", float(x)).hex()


def main():
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    from sgdm_amd.optim import FusedAdamWEma
    from test_hip_train import _loop_inputs
    from test_hip_unet import build_model
    torch.cuda.set_device(0)
    os.environ.pop("NCCL_MAX_NCHANNELS", None)
    out = {}
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("nccl", init_method=f"file://{os.path.join(td, 'store')}", rank=0, world_size=1)
        out["backend"] = str(dist.get_backend())
        model, entry = build_model("uf_clusterlayout_c32_s16", "f16x3")
        model.dropout = 0.0
        model.train()
        diff = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS).train()
        diff.set_denoise_fn(model.forward, model.forward_with_cond_scale)
        batch, t, noise, mask = _loop_inputs(entry, 0)
        params = [p for p in model.parameters() if p.requires_grad]

        def backward():
            for p in model.parameters():
                p.grad = None
            loss, _ = diff.p_losses(batch["image"].cuda(), t.cuda(), noise.cuda(), cond=batch["cond"].float().cuda(),
                                    layout=batch["layout"].cuda() if "layout" in batch else None, cond_drop_prob=0.5,
                                    cond_drop_mask=mask.cuda())
            loss.backward()
            return float(loss.detach())

        # ---- A: plain backward; the measuring step moves nothing (lr 0, no decay: p * 1 - 0 * x)
        model.hip_ddp = False
        loss_a = backward()
        eng = next(iter(model._engines.values()))
        out["plain_backward_has_arena"] = eng.backward.arena is not None
        ref = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        measure = FusedAdamWEma(params, lr=0.0, weight_decay=0.0, max_grad_norm=float("inf"))
        measure.step()
        norm_a = float(measure.grad_norm)
        out["measuring_step_moved"] = [k for k, p in model.named_parameters() if not torch.equal(p, before[k])][:8]
        # ---- B: the exchange forced through the one-rank RCCL group, then the clipped step
        for e in model._engines.values():
            e.backward = None
        model.hip_ddp = True
        model.hip_force_exchange = True
        loss_b = backward()
        arena, red = eng.backward.arena, eng.backward.reducer
        out["arena"] = arena is not None
        out["reducer_active"] = bool(red is not None and red.active)
        got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        out["n_grads"] = len(got)
        out["same_keys"] = sorted(got) == sorted(ref)
        out["mismatched"] = [k for k in ref if k not in got or not torch.equal(got[k], ref[k])][:8]
        out["losses_equal"] = loss_a == loss_b
        lo = arena.flat.data_ptr()
        hi = lo + arena.flat.numel() * 4

        def aliased():
            return sum(1 for p in params if p.grad is not None and lo <= p.grad.data_ptr() < hi)

        out["aliased_before"] = aliased()
        ptrs = {k: p.grad.data_ptr() for k, p in model.named_parameters() if p.grad is not None}
        opt = FusedAdamWEma(params, lr=1e-3, weight_decay=0.01, max_grad_norm=0.5 * norm_a)
        opt.step()
        st = opt.clip_stats()
        out["norm_plain_bits"], out["norm_exchange_bits"] = _hex(norm_a), _hex(st["norm"])
        out["norm"], out["coef"], out["skipped"], out["clipped_steps"] = st["norm"], st["coef"], st["skipped"], st["clipped_steps"]
        out["aliased_after"] = aliased()
        out["grad_pointers_kept"] = all(p.grad is not None and p.grad.data_ptr() == ptrs[k]
                                        for k, p in model.named_parameters() if k in ptrs)
        out["grads_untouched"] = [k for k in ref if not torch.equal(model.get_parameter(k).grad, ref[k])][:8]
        out["health_slot"] = float(arena.health)
        out["params_moved"] = sum(1 for k, p in model.named_parameters() if k in ref and not torch.equal(p, before[k]))
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
