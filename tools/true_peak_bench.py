"""What the true-peak meter and the true-peak limiter cost on the device (diffusynth_amd.true_peak, ds_true_peak, ds_master_limit_tp), beside
their byte floors, beside the sample-peak limiter in the same process, and beside the same measurement in torch ops.

Workload: tools/master_bench.py's: one 60 s track at 16 kHz (960 000 samples) and a batch of 8 of them, at the default Mastering (A = 80,
R = 800 samples).  In one process, every case warmed first:

  meter_us, meter_env_us  device time of ONE call of ds_true_peak (its two kernels) without / with the envelope, on tables built once: device
                          events around --launches back-to-back calls on one stream, divided by their number; median of --repeat windows
  limit_us, limit_tp_us   the same for ds_master_limit and ds_master_limit_tp (the same gain, the envelope of the same input)
  floor4_us, floor8_us    4 bytes per sample (x read) and 8 (the envelope written too) at --hbm-tbs TB/s
  torch_us                what a user would write without this meter, on the device, by the same events: zero-stuff by 4, conv1d with the 49
                          taps, abs().amax() (fp32 accumulation: NOT the meter's arithmetic, only its shape); as many launches per window as
                          fit ~0.2 s, at least 3
  call_ms, call_tp_ms     master() end to end (table upload, every entry, synchronise) by the host clock, without / with true_peak=True
  meter_call_ms           true_peak() end to end

    python tools/true_peak_bench.py [--repeat 7] [--launches 200]      -> one JSON line, profiles/true_peak_bench.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from diffusynth_amd import _lib as L  # noqa: E402
from diffusynth_amd import arranger as A  # noqa: E402
from master_bench import N, SR, events_us, track, wall_ms  # noqa: E402

TM = importlib.import_module("diffusynth_amd.true_peak")


def entries(x, n_signals, m, a, r):
    MS = L.MS
    lib = L.load()
    tab = torch.from_numpy(A._flat_table([N] * n_signals).reshape(-1)).cuda()
    ws = torch.empty(lib.ds_master_ws_bytes(n_signals, N) // 8 + 1, dtype=torch.float64, device="cuda")
    tws = torch.empty(lib.ds_true_peak_ws_bytes(n_signals, N) // 4, dtype=torch.float32, device="cuda")
    stats = torch.empty((n_signals, MS["DS_MS_NS"]), dtype=torch.float32, device="cuda")
    limited = torch.empty(n_signals, dtype=torch.int32, device="cuda")
    out, env = torch.empty_like(x), torch.empty_like(x)
    tp = torch.empty(n_signals, dtype=torch.float32, device="cuda")
    coef = TM.true_peak_coefficients().ctypes.data
    st = L.current_stream()
    f32 = lambda v: float(np.float32(v))          # noqa: E731
    keep = (tab, ws, tws, stats, limited, out, env, tp)
    meter = lambda e: L.call("ds_true_peak", x.data_ptr(), tab.data_ptr(), n_signals, N, x.numel(), coef, e, tws.data_ptr(), tp.data_ptr(), st)   # noqa: E731
    L.call("ds_master_gain", x.data_ptr(), tab.data_ptr(), n_signals, N, x.numel(), f32(m.target_rms), f32(m.max_gain), ws.data_ptr(), stats.data_ptr(),
           limited.data_ptr(), st)
    meter(env.data_ptr())
    return {"meter_us": lambda: meter(None), "meter_env_us": lambda: meter(env.data_ptr()),
            "limit_us": lambda: L.call("ds_master_limit", x.data_ptr(), tab.data_ptr(), n_signals, N, x.numel(), f32(m.ceiling), a, r, stats.data_ptr(),
                                       limited.data_ptr(), out.data_ptr(), None, st),
            "limit_tp_us": lambda: L.call("ds_master_limit_tp", x.data_ptr(), env.data_ptr(), tab.data_ptr(), n_signals, N, x.numel(), f32(m.ceiling), a, r,
                                          stats.data_ptr(), limited.data_ptr(), out.data_ptr(), None, st)}, keep


def torch_meter(x2, taps):
    """x2 (B, N) -> true peak (B,): zero-stuff, one conv1d with the 49 taps, the largest magnitude."""
    z = torch.zeros((x2.shape[0], 1, 4 * x2.shape[1] + 4), dtype=x2.dtype, device=x2.device)      # from time -1, as the meter
    z[:, 0, 4::4] = x2
    return F.conv1d(z, taps, padding=24).abs().amax(dim=(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)       # what a float4 copy reaches on an MI355X (8.0 is the data sheet)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_peak_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("true_peak_bench: needs an MI355X; there is nothing to measure without one")
    repeat = max(5, args.repeat)
    res = {"tool": "tools/true_peak_bench.py", "device": torch.cuda.get_device_name(0), "repeat": repeat, "launches": args.launches, "samples": N,
           "hbm_tbs": args.hbm_tbs, "cases": {}}
    tracks = torch.from_numpy(np.stack([track(k) for k in range(8)])).cuda()
    taps = torch.tensor([TM.tap(d) for d in range(-24, 25)], dtype=torch.float32, device="cuda").view(1, 1, 49)
    m, mtp = A.Mastering(), A.Mastering(true_peak=True)
    a, r = m.samples(SR)
    for b in (1, 8):
        x2 = tracks[:b].contiguous()
        x = x2.reshape(-1)
        calls, keep = entries(x, b, m, a, r)
        for fn in calls.values():
            fn(), fn()
        torch.cuda.synchronize()
        row = {"lookahead": a, "hold": r, "signals": b}
        row.update({k: round(events_us(fn, args.launches, repeat), 3) for k, fn in calls.items()})
        row["floor4_us"] = round(4.0 * x.numel() / (args.hbm_tbs * 1e12) * 1e6, 3)
        row["floor8_us"] = round(8.0 * x.numel() / (args.hbm_tbs * 1e12) * 1e6, 3)
        chain = lambda: torch_meter(x2, taps)                            # noqa: E731
        chain()
        one = wall_ms(chain, 1)
        row["torch_launches"] = int(min(args.launches, max(3, 200.0 / max(one, 1e-3))))
        row["torch_us"] = round(events_us(chain, row["torch_launches"], repeat), 3)
        for key, job in (("call_ms", lambda: A.master(x2, m, sample_rate=SR)), ("call_tp_ms", lambda: A.master(x2, mtp, sample_rate=SR)),
                         ("meter_call_ms", lambda: TM.true_peak(x2))):
            job(), job()
            row[key] = round(wall_ms(job, repeat), 4)
        got, want = TM.true_peak(x2), chain()
        row["max_rel_diff_to_torch_meter"] = float(((got - want).abs() / want).max())
        res["cases"][f"default_x{b}"] = row
        print(b, row, flush=True)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
