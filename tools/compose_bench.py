"""Weighted multi-prompt guidance (ds_cfg_compose): the workload whose kernel trace gives the compose launch's time
beside the U-Net forward of the same step.

    rocprofv3 --kernel-trace --stats -d DIR -o compose -- python tools/compose_bench.py [--batch 64] [--prompts 2] [--steps 4] [--phi 0.7]

One warm-up call (plan, arena, allocator), then one call of ``--steps`` "ddim" steps of DiffSynthSampler.sample() with a K-prompt mix
at (4, 256, 64) latents, CFG 6, Philox noise, bf16x3 tier, synthetic weights.  In the trace's kernel statistics ``cfg_compose_kernel``
runs once per step; everything else except the step kernel is the U-Net forward on (1 + K) * batch rows.  Prints one JSON line with
the host-clock time per step of the measured call (a device synchronise at both ends).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusynth_amd.sampler import DiffSynthSampler  # noqa: E402
from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompts", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--phi", type=float, default=0.7)
    ap.add_argument("--envelope", action="store_true", help="(K, W) weights instead of (K,)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "compose_bench.py measures on the GPU"
    torch.manual_seed(0)
    H, W, B, K = 256, 64, a.batch, a.prompts
    net = ConditionedUnet(**PRODUCTION_CONFIG).cuda().set_compute_dtype("bf16x3")
    cond = torch.randn(B, K, 512, generator=torch.Generator().manual_seed(2)).cuda()
    wt = np.linspace(1.0, 0.2, K, dtype=np.float32)
    if a.envelope:
        wt = wt[:, None] * np.linspace(0.0, 1.0, W, dtype=np.float32)[None, :]
    ms = []
    for r in range(2):                                  # (round 0: warm-up)
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=B, noise_device="philox")
        s.respace(list(np.linspace(0, 999, a.steps, dtype=np.int32)))
        s.activate_classifier_free_guidance(6.0, torch.zeros(512).cuda(), guidance_rescale=a.phi)
        s.set_condition_mix(wt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.sample(net, (B, 4, H, W), return_tensor=True, condition=cond, sampler="ddim", seed=1234)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / a.steps)
    print(json.dumps({"tool": "tools/compose_bench.py", "tier": "bf16x3", "batch": B, "prompts": K, "steps": a.steps, "phi": a.phi,
                      "envelope": a.envelope, "latent": [4, H, W], "unet_rows": (1 + K) * B, "ms_per_step": round(ms[1], 3),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
