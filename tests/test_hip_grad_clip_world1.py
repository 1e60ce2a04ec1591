"""The clipped optimizer step behind the data-parallel exchange (tests/_grad_clip_world1_child.py).  GPU only.

A world-size-1 ``nccl`` group with the exchange forced runs the code an 8-GPU job runs (tests/test_hip_rccl_world1.py): gradient
arena, bucketed all-reduce on the side stream.  The gradient norm behind it must carry the BITS of the norm behind the plain
backward -- that is what lets every replica reach the same clip coefficient without another collective -- and the gradients must
still alias the arena after the step.  A fresh child process (RCCL reads its environment once per process; a hang must not take
the suite down)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "NCCL_MAX_NCHANNELS", "SGDM_FORCE_EXCHANGE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_grad_clip_world1_child.py")],
                       env=env, capture_output=True, text=True, timeout=300)       # no hang
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0][len("RESULT "):])


def test_clipped_step_behind_the_world1_rccl_exchange():
    out = _run()
    print("\n" + json.dumps(out))
    assert out["backend"] == "nccl"
    assert out["plain_backward_has_arena"] is False and out["measuring_step_moved"] == []
    assert out["arena"] is True and out["reducer_active"] is True
    # the two backward passes agree bit for bit ...
    assert out["n_grads"] > 50 and out["same_keys"] and out["mismatched"] == [] and out["losses_equal"]
    # ... and so do the norms: the reduction order depends on the table alone, the arena's health slot is no row of it
    assert out["norm_exchange_bits"] == out["norm_plain_bits"]
    assert out["norm"] > 0 and out["skipped"] is False and out["coef"] < 1.0 and out["clipped_steps"] == 1
    assert out["health_slot"] == 0.0
    # the step ran (parameters moved) without rewriting or re-homing a gradient: p.grad still aliases the arena
    assert out["params_moved"] > 0.9 * out["n_grads"]
    assert out["aliased_before"] >= 0.9 * out["n_grads"] and out["aliased_after"] == out["aliased_before"]
    assert out["grad_pointers_kept"] is True and out["grads_untouched"] == []
