#!/usr/bin/env python3
"""What windowed sampling costs: 50-step DDIM of one long sound (B = 1, CFG 3, latents (4, 128, W), W in 256, 512, 1024), production
U-Net (synthetic weights), bf16x3 tier, window 64 / stride 32, one MI355X.

    python tools/window_bench.py [--widths 256,512,1024] [--steps 50] [--iters 3] [--out FILE.json]

  windowed    sample(WindowedUnet(net)): every step is one U-Net call on all 2 n window rows
  full_width  sample(net): one U-Net call at the sound's own width — the only way to make that sound without the wrapper (the baseline)
  per_window  sample(WindowedUnet(net, max_rows=2)): the same windows, one U-Net call per window (its two guidance rows)
The three alternate inside one timed loop; a time is the median over `iters` of a host clock around a call that ends in a device
synchronise (host work included: it is part of the call), divided by the steps.  ds_window_split / ds_window_merge are timed on the
same shapes with device events around `--kernel-iters` launches in a row — at these sizes that is the rate at which the host issues
launches, an upper bound of what they add to a step — and, with `--kernel-stats-dir`, by the kernel times of a profiled run:
    rocprofv3 --kernel-trace --stats -d DIR/<W> -o run --output-format csv -- python tools/window_bench.py --kernels-only --widths <W>
Their bytes are counted from the shapes: the split reads and writes every window element once, the blend reads every window element
once and writes every output element once (tables not counted).  Prints one JSON line.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alternating_ms(fns, iters, torch):
    """Median wall milliseconds of each of fns, called in turn."""
    ts = [[] for _ in fns]
    for _ in range(iters):
        for fn, t in zip(fns, ts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(t) for t in ts]


def event_ms(fn, iters, torch):
    """Milliseconds per call of fn over `iters` calls in a row, by device events."""
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_stats_us(d):
    """{"split": us, "merge": us}: the average kernel time of window_split_kernel / window_merge_kernel in rocprofv3's kernel_stats.csv under d."""
    import csv
    import glob
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                for k in ("split", "merge"):
                    if "window_%s_kernel" % k in row["Name"]:
                        out[k] = float(row["AverageNs"]) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="256,512,1024")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--tier", default="bf16x3")
    ap.add_argument("--kernels-only", action="store_true", help="launch the two kernels only (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats-dir", default=None, help="DIR/<W>/**/*kernel_stats.csv of such runs, one per width: their kernel times are added")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from diffusynth_amd import _lib as L
    from diffusynth_amd.sampler import DiffSynthSampler
    from diffusynth_amd.synth import synth_input, synth_state_dict
    from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet
    from diffusynth_amd.windowed import WindowedUnet
    assert torch.cuda.is_available(), "window_bench needs an MI355X"
    with open(os.path.join(HERE, "tests", "golden", "state_dict_keys.json")) as f:
        spec = [(k, tuple(s)) for k, s in json.load(f)["unet_production"]]
    net = ConditionedUnet(**PRODUCTION_CONFIG)
    net.load_state_dict(synth_state_dict(spec))
    net.to("cuda")
    net.set_compute_dtype(a.tier)
    H, window, stride, cfg = 128, 64, 32, 3.0
    un, cond = synth_input("window_bench_uncond", (512,)).cuda(), synth_input("window_bench_cond", (1, 512)).cuda()
    wnet, pnet = WindowedUnet(net, window, stride), WindowedUnet(net, window, stride, max_rows=2)
    res = {"device": torch.cuda.get_device_name(0), "tier": a.tier, "steps": a.steps, "cfg": cfg, "iters": a.iters, "window": window,
           "stride": stride, "height": H, "batch": 1, "kernel_iters": a.kernel_iters, "widths": {}}
    for W in (int(v) for v in a.widths.split(",")):
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=1, max_width=W, noise_device="philox")
        s.respace(list(np.linspace(0, 999, a.steps, dtype=np.int32)))
        s.activate_classifier_free_guidance(cfg, un)
        run = lambda model: s.sample(model, (1, 4, H, W), return_tensor=True, condition=cond, sampler="ddim", seed=1)[0][-1]     # noqa: E731
        fns = [lambda: run(wnet), lambda: run(net), lambda: run(pnet)]
        n = wnet.rows_per_sample(W)
        if a.kernels_only:
            fns, ms = [], [float("nan")] * 3
        r = {"windows": n, "unet_rows_per_step": {"windowed": 2 * n, "full_width": 2, "per_window": 2 * n},
             "unet_calls_per_step": {"windowed": 1, "full_width": 1, "per_window": n}, "flop_ratio_windowed_over_full_width": n * window / W}
        for fn in fns:                                  # every shape of the timed window, twice
            fn()
            fn()
        if not a.kernels_only:
            ms = alternating_ms(fns, a.iters, torch)
        r["ms_per_step"] = {k: round(v / a.steps, 4) for k, v in zip(("windowed", "full_width", "per_window"), ms)}
        r["windowed_over_full_width"] = round(ms[0] / ms[1], 3)
        r["per_window_over_windowed"] = round(ms[2] / ms[0], 3)
        if not a.kernels_only:
            d = (run(pnet) - run(wnet)).double().norm() / run(wnet).double().norm()
            r["rel_distance_per_window_vs_windowed"] = float(d)     # (the tier's launch choices follow the batch: not bit for bit)
        # the two kernels alone, on the tables and shapes of the windowed call (2 rows of n windows)
        plan = wnet.plan(W)
        lay, rows_dev, erow_dev, _, _ = wnet._layout(plan, 2, True, torch.device("cuda", torch.cuda.current_device()))
        wcol, wcoef = wnet._column_tables(plan, erow_dev.device)
        x = synth_input("window_bench_x", (1, 4, H, W)).cuda().repeat(2, 1, 1, 1).contiguous()
        xw = torch.empty((2 * n, 4, H, window), device="cuda")
        out = torch.empty_like(x)
        sp = L.WindowSplitParams(x=x.data_ptr(), out=xw.data_ptr(), rows=rows_dev.data_ptr(), R=2 * n, C=4, H=H, W=W, w=window, Bx=2, Bout=2 * n)
        mp = L.WindowMergeParams(eps=xw.data_ptr(), out=out.data_ptr(), erow=erow_dev.data_ptr(), wcol=wcol.data_ptr(), wcoef=wcoef.data_ptr(),
                                 R=2, n=n, C=4, H=H, W=W, w=window, Beps=2 * n, Bout=2)
        st = L.current_stream()
        split_ms = event_ms(lambda: L.call("ds_window_split", ctypes.byref(sp), st), a.kernel_iters, torch)
        merge_ms = event_ms(lambda: L.call("ds_window_merge", ctypes.byref(mp), st), a.kernel_iters, torch)
        split_bytes, merge_bytes = 2 * xw.numel() * 4, (xw.numel() + out.numel()) * 4
        r["split"] = {"us_per_launch_in_a_row": round(split_ms * 1e3, 2), "bytes": split_bytes}
        r["merge"] = {"us_per_launch_in_a_row": round(merge_ms * 1e3, 2), "bytes": merge_bytes}
        r["launches_in_a_row_share_of_a_windowed_step"] = round((split_ms + merge_ms) / (ms[0] / a.steps), 5)
        if a.kernel_stats_dir:                          # kernel times of a profiled --kernels-only run at this width
            ks = kernel_stats_us(os.path.join(a.kernel_stats_dir, str(W)))
            for k, us in ks.items():
                r[k]["kernel_us"], r[k]["kernel_GBps"] = round(us, 2), round(r[k]["bytes"] / us / 1e3, 1)
            if len(ks) == 2:
                r["kernel_share_of_a_windowed_step"] = round(sum(ks.values()) / 1e3 / (ms[0] / a.steps), 5)
        res["widths"][str(W)] = r
        print("[window_bench]", W, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
