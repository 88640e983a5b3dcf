#!/usr/bin/env python3
"""What windowed decoding costs: one long looping sound (B = 1, latents (4, 128, W), W in 256, 512, 1024) from quantised latents to
audio, production VQGAN decoder (synthetic weights), fp32 tier, window 64 / stride 32, loop, one MI355X.

    python tools/decode_bench.py [--widths 256,512,1024] [--iters 3] [--out profiles/decode_bench.json]

  windowed    latents_to_audio(WindowedDecoder(dec, loop=True)): one decoder call on all n window rows, ds_stft_window_merge,
              ds_istft_plus_loop
  full_width  latents_to_audio(dec): one decoder call at the sound's own width + ds_istft_plus — the only way without the wrapper
  per_window  latents_to_audio(WindowedDecoder(dec, loop=True, max_rows=1)): the same windows, one decoder call per window
The three alternate inside one timed loop; a time is the median over `iters` of a host clock around a call that ends in a device
synchronise (host work included: it is part of the call).  The two new kernels are timed on the same shapes with device events
around `--kernel-iters` launches in a row (at these sizes close to the rate at which the host issues launches) and by the kernel times
of a profiled run of their own, `rocprofv3 --kernel-trace --stats -- python tools/decode_bench.py --step kernels --widths <W>`.
Their bytes are counted from the shapes (tables not counted): the blend reads 12 bytes per entry of every (bin, frame) and writes 12;
the loop iSTFT reads the representation, writes and reads back 1024 floats per frame and writes the period.
This process starts no GPU work: every step (one timing run and one profiled run per width) is a child process under its own time
limit, and after a step that fails nothing more is started.  No thresholds: the numbers are recorded.  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, WINDOW, STRIDE, UP, F, HOP = 128, 64, 32, 4, 512, 256
KERNELS = {"merge": "stft_window_merge_kernel", "ola_loop": "istft_ola_loop_kernel", "frames": "istft_frames_r4_kernel"}


def _setup(W):
    sys.path.insert(0, HERE)
    import torch
    from diffusynth_amd.synth import synth_input, synth_state_dict
    from diffusynth_amd.vqgan import PRODUCTION_CONFIG, VQGAN
    from diffusynth_amd.windowed import WindowedDecoder
    assert torch.cuda.is_available(), "decode_bench needs an MI355X"
    with open(os.path.join(HERE, "tests", "golden", "state_dict_keys.json")) as f:
        spec = [(k, tuple(s)) for k, s in json.load(f)["vqgan_production"]]
    vae = VQGAN(**PRODUCTION_CONFIG)
    vae.load_state_dict(synth_state_dict(spec))
    dec = vae.to("cuda")._decoder
    dec.set_compute_dtype("fp32")
    q = synth_input("decode_bench_q", (1, 4, H, W)).cuda()
    return torch, dec, q, WindowedDecoder(dec, WINDOW, STRIDE, loop=True), WindowedDecoder(dec, WINDOW, STRIDE, loop=True, max_rows=1)


def _kernel_calls(torch, wdec, W):
    """The two new entry points on the shapes and tables of the windowed call, as closures, and their bytes."""
    import ctypes
    from diffusynth_amd import _lib as L
    plan, fplan = wdec.plan(W), wdec.plan(W, UP)
    n, T, w = plan.n, UP * W, UP * WINDOW
    dev = torch.device("cuda", torch.cuda.current_device())
    lay, _, erow_dev, _, _ = wdec._layout(plan, 1, False, dev)
    wcol, wcoef = wdec._column_tables(fplan, dev)
    g = torch.Generator(device="cuda").manual_seed(0)
    encw = torch.rand((n, 3, F, w), device="cuda", generator=g) * 2 - 1
    encw[:, 0] = encw[:, 0].abs() * 4
    out = torch.empty((1, 3, F, T), device="cuda")
    mp = L.StftWindowMergeParams(encw=encw.data_ptr(), out=out.data_ptr(), erow=erow_dev.data_ptr(), wcol=wcol.data_ptr(), wcoef=wcoef.data_ptr(),
                                 R=1, n=n, F=F, T=T, w=w, Bw=n, Bout=1)
    ws = torch.empty(L.load().ds_istft_ws_floats(1, F, T), device="cuda")
    audio = torch.empty((1, HOP * T), device="cuda")
    st = L.current_stream()
    merge = lambda: L.call("ds_stft_window_merge", ctypes.byref(mp), st)                                              # noqa: E731
    istft = lambda: L.call("ds_istft_plus_loop", out.data_ptr(), 1, F, T, HOP, ws.data_ptr(), audio.data_ptr(), st)   # noqa: E731
    keep = (encw, out, ws, audio, wcol, wcoef, erow_dev)
    nbytes = {"merge": int(fplan.cover.sum()) * F * 12 + T * F * 12,
              "istft_loop": 3 * F * T * 4 + T * 1024 * 4 + HOP * T * 4 * (1024 // HOP) + HOP * T * 4}
    return merge, istft, nbytes, keep


def step_timing(W, iters, kernel_iters):
    torch, dec, q, wdec, pdec = _setup(W)
    from diffusynth_amd.vocoder import latents_to_audio
    fns = [lambda: latents_to_audio(wdec, q), lambda: latents_to_audio(dec, q), lambda: latents_to_audio(pdec, q)]
    for fn in fns:                                      # every shape of the timed window, twice
        fn()
        fn()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for fn, t in zip(fns, ts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
    ms = [statistics.median(t) for t in ts]
    n = wdec.rows_per_sample(W)
    r = {"windows": n, "decoder_rows": {"windowed": n, "full_width": 1, "per_window": n}, "decoder_calls": {"windowed": 1, "full_width": 1, "per_window": n},
         "flop_ratio_windowed_over_full_width": n * WINDOW / W, "audio_samples": {"windowed": HOP * UP * W, "full_width": HOP * (UP * W - 1)},
         "ms": {k: round(v, 3) for k, v in zip(("windowed", "full_width", "per_window"), ms)},
         "windowed_over_full_width": round(ms[0] / ms[1], 3), "per_window_over_windowed": round(ms[2] / ms[0], 3)}
    a, b = latents_to_audio(wdec, q), latents_to_audio(pdec, q)
    r["per_window_equals_windowed"] = bool(torch.equal(a, b))
    merge, istft, nbytes, keep = _kernel_calls(torch, wdec, W)
    for name, fn in (("merge", merge), ("istft_loop", istft)):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(kernel_iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        r[name] = {"us_per_launch_in_a_row": round(e0.elapsed_time(e1) / kernel_iters * 1e3, 2), "bytes": nbytes[name]}
    r["launches_in_a_row_share_of_a_windowed_decode"] = round((r["merge"]["us_per_launch_in_a_row"] + r["istft_loop"]["us_per_launch_in_a_row"]) / 1e3 / ms[0], 5)
    r["device"] = torch.cuda.get_device_name(0)
    print("RESULT " + json.dumps(r), flush=True)


def step_kernels(W, kernel_iters):
    sys.path.insert(0, HERE)
    import torch
    from diffusynth_amd.windowed import WindowedDecoder
    assert torch.cuda.is_available(), "decode_bench needs an MI355X"
    merge, istft, _, keep = _kernel_calls(torch, WindowedDecoder(lambda q: q, WINDOW, STRIDE, loop=True), W)     # (the tables only: no decoder)
    for _ in range(kernel_iters):
        merge()
        istft()
    torch.cuda.synchronize()


def kernel_stats_us(d):
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                for k, name in KERNELS.items():
                    if name in row["Name"]:
                        out[k] = round(float(row["AverageNs"]) / 1e3, 2)
    return out


def child(cmd, limit):
    """Run one GPU step under its own time limit (coreutils timeout: 124 or 137 for a step that ran out of time).  (returncode, stdout)."""
    cmd = ["timeout", "-k", "10", str(limit)] + cmd
    print("[decode_bench]", " ".join(cmd), file=sys.stderr, flush=True)
    p = subprocess.run(cmd, cwd=HERE, stdout=subprocess.PIPE, text=True)
    return p.returncode, p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="256,512,1024")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--step", choices=["timing", "kernels"], default=None, help="(internal) one GPU step of one width, run as a child process")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each child step may take")
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    widths = [int(v) for v in a.widths.split(",")]
    if a.step == "timing":
        return step_timing(widths[0], a.iters, a.kernel_iters)
    if a.step == "kernels":
        return step_kernels(widths[0], a.kernel_iters)
    res = {"tier": "fp32", "iters": a.iters, "window": WINDOW, "stride": STRIDE, "loop": True, "height": H, "batch": 1, "kernel_iters": a.kernel_iters,
           "widths": {}}
    me = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--kernel-iters", str(a.kernel_iters)]
    failed = None
    for W in widths:
        rc, out = child(me + ["--step", "timing", "--widths", str(W)], a.step_timeout)
        lines = [ln for ln in out.splitlines() if ln.startswith("RESULT ")]
        if rc != 0 or not lines:
            failed = "timing step of W=%d ended with %d" % (W, rc)
            break
        r = json.loads(lines[-1][7:])
        res["device"] = r.pop("device")
        if not a.no_profile:
            with tempfile.TemporaryDirectory() as d:
                rc, _ = child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--"] + me +
                              ["--step", "kernels", "--widths", str(W)], a.step_timeout)
                if rc != 0:
                    failed = "profiled step of W=%d ended with %d" % (W, rc)
                    res["widths"][str(W)] = r
                    break
                ks = kernel_stats_us(d)
            r["kernel_us"] = ks
            if "merge" in ks:
                r["merge"]["kernel_us"], r["merge"]["kernel_GBps"] = ks["merge"], round(r["merge"]["bytes"] / ks["merge"] / 1e3, 1)
            if "frames" in ks and "ola_loop" in ks:
                us = ks["frames"] + ks["ola_loop"]
                r["istft_loop"]["kernel_us"], r["istft_loop"]["kernel_GBps"] = round(us, 2), round(r["istft_loop"]["bytes"] / us / 1e3, 1)
            if "merge" in ks and "ola_loop" in ks:
                r["new_kernels_share_of_a_windowed_decode"] = round((ks["merge"] + ks["ola_loop"]) / 1e3 / r["ms"]["windowed"], 5)
        res["widths"][str(W)] = r
        print("[decode_bench]", W, json.dumps(r), file=sys.stderr, flush=True)
    if failed:
        res["failed"] = failed                          # nothing more was started after it
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
