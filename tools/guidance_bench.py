"""Guidance rescale (ds_cfg_rescale): what the launch costs, what it adds to a sampler step, and the gains it applies.

One process, every shape warmed up first, medians over alternating rounds:
  kernel_us  device time of one ds_cfg_rescale launch (HIP events around `reps` back-to-back launches on the same buffers, out of place)
             at 1, 8, 64 and 128 rows of (4, 256, 64) and of (4, 128, 64), next to the byte model (5 passes of 4 bytes per element: both
             inputs are read for the statistics and again for the result, which is written once) at 4.4 TB/s
  step_ms    ms per step of DiffSynthSampler.sample() with guidance_rescale 0.7 against 0, the two alternating round by round, at the
             headline workload of bench.py (batch 64, CFG 6, "ddpm", (4, 256, 64), bf16x3, Philox noise) and at batch 1: host clock around
             the call with a device synchronise at both ends, divided by the steps
  gains      g per step (mean and extremes over a batch of 2) along a 20-step "ddim" trajectory at CFG 6 and at CFG 20, phi 0.7.
             SYNTHETIC weights (torch's default initialisation, seed 0) and random conditions: the numbers show the plumbing and the
             range of g such a model produces, not what a trained checkpoint would give.

    python tools/guidance_bench.py [--out profiles/guidance_bench.json] [--commit HASH [--dirty]]

Prints the JSON line and writes it to --out.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusynth_amd import _lib as L  # noqa: E402
from diffusynth_amd.sampler import DiffSynthSampler  # noqa: E402
from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet  # noqa: E402

STREAM_TBS = 4.4          # what a streaming kernel reaches on this chip
PHI = 0.7


def rescale(u, c, scale, phi, out, gain=None):
    p = L.CfgRescaleParams(eps_u=u.data_ptr(), eps_c=c.data_ptr(), out=out.data_ptr(), gain=None if gain is None else gain.data_ptr(),
                           cfg_scale=scale, phi=phi, B=u.shape[0], CHW=u[0].numel())
    L.call("ds_cfg_rescale", ctypes.byref(p), L.current_stream())


def kernel_table(rows=(1, 8, 64, 128), shapes=((4, 256, 64), (4, 128, 64)), rounds=9, reps=20):
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {}
    for shape in shapes:
        chw = int(np.prod(shape))
        bufs = {}
        for R in rows:
            u = torch.randn(R, chw, device="cuda", generator=g)
            bufs[R] = (u, u + 0.3 * torch.randn(R, chw, device="cuda", generator=g), torch.empty(R, chw, device="cuda"))
        us = {R: [] for R in rows}
        for r in range(rounds + 1):                     # (round 0: warm-up)
            for R in rows:
                u, c, out = bufs[R]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    rescale(u, c, 6.0, PHI, out)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    us[R].append(1e3 * e0.elapsed_time(e1) / reps)
        key = "x".join(str(v) for v in shape)
        res[key] = {}
        for R in rows:
            model = 5 * 4 * R * chw / (STREAM_TBS * 1e12) * 1e6
            med = float(np.median(us[R]))
            res[key]["rows%d" % R] = {"median_us": round(med, 2), "min_us": round(min(us[R]), 2), "max_us": round(max(us[R]), 2),
                                      "byte_model_us": round(model, 2), "over_byte_model": round(med / model, 1)}
        print(f"[guidance_bench] kernel {key}: {res[key]}", file=sys.stderr, flush=True)
    return res


def _sampler(K, B, H, scale, un, phi):
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=B, noise_device="philox")
    s.respace(list(np.linspace(0, 999, K, dtype=np.int32)))
    s.activate_classifier_free_guidance(scale, un, guidance_rescale=phi)
    return s


def step_table(net, un, cases=((64, 10, 5), (1, 20, 7)), H=256, W=64):
    """cases: (batch, steps per call, rounds)."""
    g = torch.Generator().manual_seed(2)
    res = {}
    for B, K, rounds in cases:
        cond = torch.randn(B, 512, generator=g).cuda()
        ms = {0.0: [], PHI: []}
        for r in range(rounds + 1):                     # (round 0: warm-up — plan, arena, allocator)
            for phi in (0.0, PHI):
                s = _sampler(K, B, H, 6.0, un, phi)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.sample(net, (B, 4, H, W), return_tensor=True, condition=cond, sampler="ddpm", seed=1234)
                torch.cuda.synchronize()
                if r:
                    ms[phi].append(1e3 * (time.perf_counter() - t0) / K)
        m0, m1 = float(np.median(ms[0.0])), float(np.median(ms[PHI]))
        res["B%d" % B] = {"steps_per_call": K, "rounds": rounds, "phi0_ms_per_step": round(m0, 4), "phi0_min_max": [round(min(ms[0.0]), 4), round(max(ms[0.0]), 4)],
                          "phi0.7_ms_per_step": round(m1, 4), "phi0.7_min_max": [round(min(ms[PHI]), 4), round(max(ms[PHI]), 4)],
                          "added_percent": round(100.0 * (m1 / m0 - 1.0), 3)}
        print(f"[guidance_bench] step B={B}: {res['B%d' % B]}", file=sys.stderr, flush=True)
    return res


class _Recorder:
    """The sampler's own per-step arithmetic as a model for a sampler without guidance (tests/test_hip_guidance.py holds the two to the
    same bits), keeping every step's gains."""

    def __init__(self, net, un, scale):
        self.net, self.un, self.scale, self.gains = net, un, scale, []

    def __call__(self, x, t, c):
        B = x.shape[0]
        out = self.net(torch.cat([x, x]), torch.cat([t, t]), torch.cat([self.un.unsqueeze(0).repeat(B, 1), c]))
        eu, ec = (h.contiguous().flatten(1) for h in out.chunk(2))
        res, gain = torch.empty_like(eu), torch.empty(B, device="cuda")
        rescale(eu, ec, self.scale, PHI, res, gain)
        self.gains.append(gain.cpu().tolist())
        return res.view_as(x)


def gain_table(net, un, K=20, B=2, H=256, W=64):
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B, 512, generator=g).cuda()
    res = {"weights": "synthetic (torch default initialisation, seed 0): not a trained checkpoint", "phi": PHI, "steps": K, "batch": B, "sampler": "ddim"}
    for scale in (6.0, 20.0):
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=B, noise_device="philox")
        s.respace(list(np.linspace(0, 999, K, dtype=np.int32)))
        rec = _Recorder(net, un, scale)
        s.sample(rec, (B, 4, H, W), return_tensor=True, condition=cond, sampler="ddim", seed=7)
        res["cfg%d" % scale] = {"g_mean_per_step": [round(float(np.mean(v)), 4) for v in rec.gains],
                                "g_min": round(min(min(v) for v in rec.gains), 4), "g_max": round(max(max(v) for v in rec.gains), 4)}
        print(f"[guidance_bench] gains CFG {scale}: {res['cfg%d' % scale]}", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.json"))
    ap.add_argument("--commit", default=None, help="commit hash of the measured tree (default: git rev-parse HEAD)")
    ap.add_argument("--dirty", action="store_true", help="with --commit: the measured tree is that commit plus uncommitted changes")
    a = ap.parse_args()
    commit, dirty = a.commit, a.dirty
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
            dirty = bool(subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], text=True,
                                                 stderr=subprocess.DEVNULL).strip())
        except Exception:
            commit, dirty = "unknown", None
    assert torch.cuda.is_available(), "guidance_bench.py measures on the GPU"
    torch.manual_seed(0)
    net = ConditionedUnet(**PRODUCTION_CONFIG).cuda().set_compute_dtype("bf16x3")
    un = torch.zeros(512).cuda()
    res = {"tool": "tools/guidance_bench.py", "commit": commit, "uncommitted_changes": dirty, "tier": "bf16x3", "device": torch.cuda.get_device_name(0),
           "kernel_us": kernel_table(), "step_ms": step_table(net, un), "gains": gain_table(net, un)}
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
