#!/usr/bin/env python3
"""What a prompt's condition costs before the first U-Net step: ClapTextTower.get_text_features at production size (12 layers of 768,
125 M parameters, torch default initialisation), fp32, one MI355X.  Not a test: no number here passes or fails.

    python tools/clap_text_bench.py [--shapes 1x8,2x16,16x32] [--iters 50] [--what device,host] [--out FILE.json]

  device  get_text_features on ids that arrive on the CPU (what a tokenizer returns): device events around `iters` calls after a warm-up of
          every shape, median per call; the same with a host clock around call + synchronise (what a caller waits for); the number of
          launches of a call, counted at the library boundary
  host    the fp32 restatement of tests/clap_text_ref.py (plain torch ops) on the CPU with 16 threads, on the host this runs on: what keeping
          the tower on the CPU costs (app.py:59), without the copy of the condition to the device
Next to them the weight-streaming floor: 4 B x parameters over 4.4 TB/s, the rate a read-mostly stream measures on this GPU, once
for all parameters and once for those a call reads (the encoder, pooler and projection matrices; of the embedding tables only S rows).
For kernel times run it under `rocprofv3 --kernel-trace --stats` with --what device.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 4.4e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x8,2x16,16x32")
    ap.add_argument("--what", default="device,host")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import clap_text_ref as R
    from diffusynth_amd import ClapTextTower
    from diffusynth_amd import _lib as L
    assert torch.cuda.is_available(), "clap_text_bench needs an MI355X"
    what = set(a.what.split(","))
    torch.manual_seed(0)
    torch.set_num_threads(16)
    tower = ClapTextTower()
    sd = {k: v.detach().clone() for k, v in tower.state_dict().items()}
    tower.cuda()
    n_all = sum(p.numel() for p in tower.parameters())
    n_tables = sum(p.numel() for p in tower.text_model.embeddings.parameters())
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "parameters": n_all, "parameters_read_per_call": n_all - n_tables,
           "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "floor_all_parameters_us": 4 * n_all / HBM_BYTES_PER_S * 1e6,
           "floor_parameters_read_us": 4 * (n_all - n_tables) / HBM_BYTES_PER_S * 1e6, "shapes": {}}
    cases = []
    for shape in a.shapes.split(","):
        B, S = (int(v) for v in shape.split("x"))
        ids = R._rows(B, S, R.PROD_CONFIG["vocab_size"], [S - (b % 4) * (S // 8) for b in range(B)])         # ragged right padding
        cases.append((shape, ids, (ids != R.PAD).long()))
    if "device" in what:
        for _, ids, mask in cases:                               # every shape before any timed window
            for _ in range(3):
                tower.get_text_features(ids, mask)
        torch.cuda.synchronize()
    for shape, ids, mask in cases:
        r = {}
        if "device" in what:
            count, real = [0], L.call

            def counting(name, *args):
                count[0] += 1
                return real(name, *args)
            L.call = counting
            try:
                tower.get_text_features(ids, mask)
            finally:
                L.call = real
            torch.cuda.synchronize()
            r["launches"] = count[0]
            ev, wall = [], []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                tower.get_text_features(ids, mask)
                e1.record()
                e1.synchronize()
                wall.append((time.perf_counter() - t0) * 1e6)
                ev.append(e0.elapsed_time(e1) * 1e3)
            ev.sort()
            r["device_events_us"] = statistics.median(ev)
            r["device_events_us_min_max"] = [ev[0], ev[-1]]
            r["call_and_synchronize_us"] = statistics.median(wall)
            r["device_over_floor_parameters_read"] = r["device_events_us"] / res["floor_parameters_read_us"]
        if "host" in what:
            R.tower(sd, R.PROD_CONFIG, ids, mask, torch.float32)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                R.tower(sd, R.PROD_CONFIG, ids, mask, torch.float32)
                ts.append((time.perf_counter() - t0) * 1e3)
            r["torch_cpu_16_threads_ms"] = statistics.median(ts)
        res["shapes"][shape] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
