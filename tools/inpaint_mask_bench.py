"""What the Inpaint tab's latent mask costs on the device (diffusynth_amd.inpaint_mask), beside the numpy + scipy block it replaces.

Workload: one drawing of 512 x 256 and one of 512 x 576 pixels (latents of width 64 and 144), two ImageEditor layers each, a painted-blob
mask, a time / frequency rectangle, area "masked".  In one process, every shape warmed up first:

  layers_us, prefilter_us, zoom_us   device time of ONE call of ds_mask_layers / ds_mask_prefilter (its two launches) / ds_mask_zoom: device
                                     events around --launches back-to-back calls on one stream, divided by their number; median of --repeat
  call_ms, call_host_layers_ms       latent_mask_from_layers end to end (table upload, three entries, synchronise) by the host clock, on layers
                                     that are device tensors / numpy arrays (the second adds the upload of the layers)
  reference_ms                       the reference's block on this host, inpaint_with_text.py:205-227 (mean of the layers, threshold,
                                     scipy.ndimage.zoom, clip, rectangle, inversion) by the host clock; scipy is imported by this tool only

    python tools/inpaint_mask_bench.py [--repeat 7] [--launches 200]      -> one JSON line, profiles/inpaint_mask_bench.json
    python tools/inpaint_mask_bench.py --what kernel                      the run to put under `rocprofv3 --kernel-trace --stats`
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import inpaint_mask_ref as R  # noqa: E402
from diffusynth_amd import _lib as L  # noqa: E402
from diffusynth_amd import inpaint_mask as M  # noqa: E402

SHAPES = ((512, 256), (512, 576))
KW = dict(time_range=(0.5, 2.0), freq_range=(20, 60), inpaint_area="masked")


def wall(fn, repeat):
    """Median ms of fn() by the host clock around a device synchronise; fn is warm."""
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def events_us(fn, launches, repeat):
    """Median over `repeat` of the device time of one fn(), from events around `launches` back-to-back calls."""
    ts = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / launches)
    return statistics.median(ts)


def entries(layers, h, w):
    """The three entry calls of one mask on buffers of their own: name -> callable."""
    spec = M.plan_masks([layers], (R.zoomed_size(h), R.zoomed_size(w)), time_ranges=KW["time_range"], freq_ranges=KW["freq_range"],
                        inpaint_areas=KW["inpaint_area"])[0]
    IM = L.IM
    tab = np.zeros((1, IM["DS_IM_NI"]), np.int32)
    tab[0, IM["DS_IM_NL"]], tab[0, IM["DS_IM_H"]], tab[0, IM["DS_IM_W"]] = len(layers), h, w
    tab[0, IM["DS_IM_HO"]], tab[0, IM["DS_IM_WO"]] = spec.HO, spec.WO
    tab[0, IM["DS_IM_R0"]:IM["DS_IM_C1"] + 1], tab[0, IM["DS_IM_INV"]] = spec.rect, spec.inv
    tab_dev = torch.from_numpy(tab.reshape(-1)).cuda()
    lay = torch.cat([a.reshape(-1) for a in layers])
    planes = torch.empty(h * w, dtype=torch.uint8, device="cuda")
    ws = torch.empty(L.load().ds_mask_ws_bytes(h * w) // 8, dtype=torch.float64, device="cuda")
    out = torch.empty(spec.HO * spec.WO, dtype=torch.float32, device="cuda")
    st = L.current_stream()
    keep = (tab_dev, lay, planes, ws, out)
    return {"layers_us": lambda: L.call("ds_mask_layers", lay.data_ptr(), tab_dev.data_ptr(), 1, h * w, len(layers) * h * w, h * w, planes.data_ptr(), st),
            "prefilter_us": lambda: L.call("ds_mask_prefilter", planes.data_ptr(), tab_dev.data_ptr(), 1, h, w, h * w, ws.data_ptr(), st),
            "zoom_us": lambda: L.call("ds_mask_zoom", ws.data_ptr(), tab_dev.data_ptr(), 1, spec.HO * spec.WO, h * w, spec.HO * spec.WO, out.data_ptr(), None, st)}, keep


def reference_block(layers, zoom, time_resolution=256, VAE_scale=4):
    """inpaint_with_text.py:205-227 on numpy layers."""
    averaged = np.mean(np.stack(layers, axis=0), axis=0)[:, :, -1]
    merged = np.where(averaged > 0, 1, 0)
    latent_mask = np.clip(zoom(merged, (1 / VAE_scale, 1 / VAE_scale)), 0, 1)
    (fb, fe), (tb, te) = KW["freq_range"], KW["time_range"]
    latent_mask[int(fb):int(fe), int(tb * time_resolution / (VAE_scale * 4)):int(te * time_resolution / (VAE_scale * 4))] = 1
    return 1 - latent_mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--what", default="bench", choices=["bench", "kernel"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_mask_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inpaint_mask_bench: needs an MI355X; there is nothing to measure without one")
    repeat = max(5, args.repeat)
    res = {"tool": "tools/inpaint_mask_bench.py", "device": torch.cuda.get_device_name(0), "repeat": repeat, "launches": args.launches, "layers": 2,
           "shapes": {}}
    for h, w in SHAPES:
        host_layers = R.layers_of(R.blob_mask(h, w, seed=w), 2, seed=w)
        dev_layers = [torch.from_numpy(a).cuda() for a in host_layers]
        calls, keep = entries(dev_layers, h, w)
        for fn in calls.values():                                           # warmed, in pipeline order (the later entries read the earlier one's output)
            fn(), fn()
        torch.cuda.synchronize()
        if args.what == "kernel":
            for _ in range(args.launches):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            print(f"inpaint_mask_bench: {args.launches} calls of each entry at {h} x {w}")
            continue
        from scipy.ndimage import zoom
        lat = (R.zoomed_size(h), R.zoomed_size(w))
        row = {k: round(events_us(fn, args.launches, repeat), 3) for k, fn in calls.items()}
        jobs = {"call_ms": lambda: M.latent_mask_from_layers(dev_layers, latent_shape=lat, **KW),
                "call_host_layers_ms": lambda: M.latent_mask_from_layers(host_layers, latent_shape=lat, **KW)}
        for fn in jobs.values():
            fn(), fn()
        row.update({k: round(wall(fn, repeat), 4) for k, fn in jobs.items()})
        reference_block(host_layers, zoom)
        ts = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            want = reference_block(host_layers, zoom)
            ts.append((time.perf_counter() - t0) * 1e3)
        row["reference_ms"] = round(statistics.median(ts), 4)
        got = M.latent_mask_from_layers(dev_layers, latent_shape=lat, **KW).cpu().numpy()[0, 0]
        row["equals_reference"] = bool(np.array_equal(got, want[::-1].astype(np.float32)))
        res["shapes"]["%dx%d" % (h, w)] = row
    if args.what == "kernel":
        return
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
