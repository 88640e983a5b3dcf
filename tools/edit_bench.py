#!/usr/bin/env python3
"""What text-guided editing by DDPM inversion costs: edit_invert and edit_sample on (B, 4, 128, 64) latents, production U-Net
(synthetic weights), 50-step schedule, CFG 3, bf16x3 tier, one MI355X.

    python tools/edit_bench.py [--batches 1,8] [--steps 50] [--iters 5] [--max-rows 128] [--out FILE.json]

  invert  edit_invert(max_rows=...) against the same evaluations issued one index at a time (edit_invert with max_rows = one index's
          U-Net rows: the same kernels and the same results in the fp32 tier, start - 1 model calls of 2 B rows).  There is no older
          inversion to compare with.
  edit    edit_sample against img_guided_sample("ddpm") of equal step count: the same U-Net work per step, given noise against a draw
The two sides of a pair alternate inside one timed loop; a time is the median over `iters` of a host clock around a call that ends
in a device synchronise (host work included: it is part of the call).  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def paired_ms(fa, fb, iters, torch):
    """Median wall milliseconds of fa and of fb, called alternately."""
    ta, tb = [], []
    for _ in range(iters):
        for fn, ts in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ta), statistics.median(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=128)
    ap.add_argument("--tier", default="bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from diffusynth_amd.sampler import DiffSynthSampler
    from diffusynth_amd.synth import synth_input, synth_state_dict
    from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet
    assert torch.cuda.is_available(), "edit_bench needs an MI355X"
    with open(os.path.join(HERE, "tests", "golden", "state_dict_keys.json")) as f:
        spec = [(k, tuple(s)) for k, s in json.load(f)["unet_production"]]
    net = ConditionedUnet(**PRODUCTION_CONFIG)
    net.load_state_dict(synth_state_dict(spec))
    net.to("cuda")
    net.set_compute_dtype(a.tier)
    H, W, cfg = 128, 64, 3.0
    un = synth_input("edit_bench_uncond", (512,)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "tier": a.tier, "steps": a.steps, "cfg": cfg, "iters": a.iters, "max_rows": a.max_rows,
           "latent": [4, H, W], "batches": {}}
    for B in (int(v) for v in a.batches.split(",")):
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=B, noise_device="philox")
        s.respace(list(np.linspace(0, 999, a.steps, dtype=np.int32)))
        s.activate_classifier_free_guidance(cfg, un)
        x0 = synth_input("edit_bench_x0:%d" % B, (B, 4, H, W)).cuda()
        src, dst = synth_input("edit_bench_src:%d" % B, (B, 512)).cuda(), synth_input("edit_bench_dst:%d" % B, (B, 512)).cuda()
        batched = lambda: s.edit_invert(net, x0, condition=src, seed=1, max_rows=a.max_rows)               # noqa: E731
        one_by_one = lambda: s.edit_invert(net, x0, condition=src, seed=1, max_rows=2 * B)                 # noqa: E731
        inv = batched()
        edit = lambda: s.edit_sample(net, inv, condition=dst, return_tensor=True)                          # noqa: E731
        sdedit = lambda: s.img_guided_sample(net, (B, 4, H, W), 1.0, x0, return_tensor=True, condition=dst, sampler="ddpm", seed=1)  # noqa: E731
        for fn in (batched, one_by_one, edit, sdedit):              # every shape of the timed window, twice
            fn()
            fn()
        r = {"unet_evaluations": (a.steps - 1) * B, "unet_rows": 2 * (a.steps - 1) * B}
        r["edit_invert_ms"], r["edit_invert_one_index_a_call_ms"] = paired_ms(batched, one_by_one, a.iters, torch)
        r["edit_sample_ms"], r["img_guided_sample_ddpm_ms"] = paired_ms(edit, sdedit, a.iters, torch)
        d = (one_by_one().z - inv.z).double().norm() / inv.z.double().norm()
        r["z_rel_distance_batched_vs_one_index_a_call"] = float(d)       # (the tier's launch choices follow the batch: not bit for bit)
        res["batches"][str(B)] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
