"""Concurrent sampler calls, sequential vs batched (diffusynth_amd.batching.SamplingBatcher), in the bf16x3 tier.

Scenarios (each timed both ways in one process, after one untimed warm-up pass of each way):
  A  16 batch-1 text requests: CFG 1, 20-step DDIM, (1, 4, 256, 64)
  B  32 arranger notes: batch-1 inpaint_sample, DDPM, dynamic masks, noising_strength 0.7, end_noise_level_ratio 0,
     mask_flexivity 1.0; eight each at widths 32 / 48 / 64 / 80, height 128, 20-step schedule
  C  8 text2sound UI-default requests: batch 8, CFG 6, 20-step DDIM, (8, 4, 128, 64), submitted one tick apart

Wall-clock is the host clock around each run with a device synchronise at both ends.  Per scenario: both times, the speed-up,
the batcher's host time per tick, its plan builds (warm-up run and timed run) and the max-norm / rms relative difference of every
request's final latents, batched against standalone.  Prints one JSON line.

    python tools/batching_bench.py [--noise-device philox|cpu|none] [--pin N] [--commit HASH [--dirty]]

--pin N (the price of batch-invariant results, ConditionedUnet.pin_launch_batch): every scenario is measured unpinned first — the
default behaviour — and then again with the model pinned at N in the same process ("pinned": the same fields; there batched against
standalone must be bit-identical, "bit_identical"), followed by "forward_ms": the time of one conditioned U-Net forward on (B, 4, 256, 64)
at B = 1 and B = 128, unpinned and pinned at 1, 16 and 128, the variants alternating in one loop (median of the rounds).  N would be the
batcher's max_rows (128).

"commit" is the measured commit and "uncommitted_changes" whether the tree carried changes on top of it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusynth_amd.batching import SamplingBatcher  # noqa: E402
from diffusynth_amd.sampler import DiffSynthSampler  # noqa: E402
from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet  # noqa: E402


def _sampler(K, B, H, noise_device, cfg=1.0, uncond=None):
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=max(B, 1), noise_device=noise_device)
    s.respace(list(np.linspace(0, 999, K, dtype=np.int32)))
    if cfg != 1.0:
        s.activate_classifier_free_guidance(cfg, uncond)
    return s


def scenarios(noise_device):
    g = torch.Generator().manual_seed(0)
    emb = lambda B: torch.randn(B, 512, generator=g).cuda()                               # noqa: E731
    un = torch.zeros(512).cuda()
    A = [(0, (lambda: _sampler(20, 1, 256, noise_device)), "sample", ((1, 4, 256, 64),),
          dict(return_tensor=True, condition=emb(1), sampler="ddim", seed=100 + i)) for i in range(16)]
    B = []
    for i in range(32):
        w = (32, 48, 64, 80)[i // 8]
        guide = torch.randn(1, 4, 128, 64, generator=g).cuda()
        B.append((0, (lambda: _sampler(20, 1, 128, noise_device)), "inpaint_sample", ((1, 4, 128, w), 0.7, guide, None),
                  dict(return_tensor=True, condition=emb(1), sampler="ddpm", use_dynamic_mask=True, end_noise_level_ratio=0.0,
                       mask_flexivity=1.0, seed=200 + i)))
    Cs = [(i, (lambda: _sampler(20, 8, 128, noise_device, 6.0, un)), "sample", ((8, 4, 128, 64),),
           dict(return_tensor=True, condition=emb(8), sampler="ddim", seed=300 + i)) for i in range(8)]
    return {"A": A, "B": B, "C": Cs}


def run_sequential(net, reqs):
    outs = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _, mk, method, args, kw in reqs:
        outs.append(getattr(mk(), method)(net, *args, **kw)[0][-1])
    torch.cuda.synchronize()
    return time.perf_counter() - t0, outs


def run_batched(net, reqs):
    b = SamplingBatcher(net, max_rows=128)
    handles = [None] * len(reqs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tick = 0
    while any(h is None for h in handles) or b.active():
        for i, (at, mk, method, args, kw) in enumerate(reqs):
            if handles[i] is None and at <= tick:
                handles[i] = b.submit(mk(), method, *args, **kw)
        b.step()
        tick += 1
    outs = [h.result()[0][-1] for h in handles]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, outs, b


def measure(net, reqs):
    """One scenario on the model as it stands (tier, pin): warm-up of both ways, then both ways timed."""
    run_sequential(net, reqs)                       # warm-up (plans of every shape, allocator)
    _, _, bw = run_batched(net, reqs)
    t_seq, seq = run_sequential(net, reqs)
    t_bat, bat, b = run_batched(net, reqs)
    mx = rms = 0.0
    for x, y in zip(bat, seq):
        d = (x.double() - y.double())
        mx = max(mx, (d.abs().max() / y.double().abs().max()).item())
        rms = max(rms, (d.norm() / y.double().norm()).item())
    return {"requests": len(reqs), "sequential_s": round(t_seq, 4), "batched_s": round(t_bat, 4),
            "speedup": round(t_seq / t_bat, 3), "ticks": b.ticks,
            "host_ms_per_tick": round(1e3 * b.host_seconds / max(b.ticks, 1), 3),
            "plan_builds_warmup": bw.plan_builds, "plan_builds_timed": b.plan_builds,
            "unet_batches": len(b.unet_batches),
            "max_norm_rel_diff": mx, "rms_rel_diff": rms, "bit_identical": all(torch.equal(x, y) for x, y in zip(bat, seq))}


def forward_table(net, batches=(1, 128), pins=(None, 1, 16, 128), rounds=7):
    """ms per conditioned forward on (B, 4, 256, 64): device events around `reps` forwards, the pins alternating inside every round."""
    g = torch.Generator().manual_seed(1)
    out = {}
    for B in batches:
        x, t, c = torch.randn(B, 4, 256, 64, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda(), torch.randn(B, 512, generator=g).cuda()
        reps = 20 if B == 1 else 3
        ms = {pin: [] for pin in pins}
        for r in range(rounds + 1):                     # (round 0: warm-up — plans, arena growth)
            for pin in pins:
                net.pin_launch_batch(pin)
                net(x, t, c)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    net(x, t, c)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    ms[pin].append(e0.elapsed_time(e1) / reps)
        out["B%d" % B] = {("unpinned" if pin is None else "pin%d" % pin): {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3),
                                                                           "max_ms": round(max(v), 3)} for pin, v in ms.items()}
        print(f"[batching_bench] forward B={B}: {out['B%d' % B]}", file=sys.stderr, flush=True)
    net.pin_launch_batch(None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise-device", default="philox", choices=["philox", "cpu", "none"])
    ap.add_argument("--pin", type=int, default=None, metavar="N",
                    help="also measure every scenario with the model pinned at N (ConditionedUnet.pin_launch_batch), and the forward table")
    ap.add_argument("--commit", default=None, help="commit hash of the measured tree (default: git rev-parse HEAD)")
    ap.add_argument("--dirty", action="store_true", help="with --commit: the measured tree is that commit plus uncommitted changes")
    a = ap.parse_args()
    nd = None if a.noise_device == "none" else a.noise_device
    commit, dirty = a.commit, a.dirty
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
            dirty = bool(subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], text=True,
                                                 stderr=subprocess.DEVNULL).strip())
        except Exception:
            commit, dirty = "unknown", None
    torch.manual_seed(0)
    net = ConditionedUnet(**PRODUCTION_CONFIG).cuda().set_compute_dtype("bf16x3")
    res = {"tool": "tools/batching_bench.py", "commit": commit, "uncommitted_changes": dirty, "tier": "bf16x3", "noise_device": a.noise_device,
           "device": torch.cuda.get_device_name(0), "scenarios": {}}
    for name, reqs in scenarios(nd).items():
        res["scenarios"][name] = measure(net, reqs)
        print(f"[batching_bench] {name}: {res['scenarios'][name]}", file=sys.stderr, flush=True)
        if a.pin is not None:
            net.pin_launch_batch(a.pin)
            pinned = res.setdefault("pinned", {"pin": a.pin, "scenarios": {}})
            pinned["scenarios"][name] = measure(net, reqs)
            pinned["scenarios"][name]["batched_s_over_unpinned"] = round(pinned["scenarios"][name]["batched_s"] / res["scenarios"][name]["batched_s"], 3)
            print(f"[batching_bench] {name} pinned at {a.pin}: {pinned['scenarios'][name]}", file=sys.stderr, flush=True)
            net.pin_launch_batch(None)
    if a.pin is not None:
        res["forward_ms"] = forward_table(net)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
