"""What the mastering stage costs on the device (diffusynth_amd.arranger.master), beside its byte floor and beside the same chain in torch ops.

Workload: one 60 s track at 16 kHz (960 000 samples) and a batch of 8 of them, 55 Hz plus noise with loud and quiet stretches and a few
spikes, at the default Mastering (A = 80, R = 800 samples) and at the caps (A = 1024, R = 8192).  In one process, every case warmed first:

  gain_us, limit_us   device time of ONE call of ds_master_gain (its two kernels) / ds_master_limit on tables built once: device events around
                      --launches back-to-back calls on one stream, divided by their number; median of --repeat windows
  floor_us            12 bytes per sample (x read by the gain, x read and y written by the limiter) at --hbm-tbs TB/s
  torch_us            the chain a user would write without this stage, on the device, by the same events: rms in float64, gL x,
                      c / |u| where over, -max_pool1d(-r) over R + A + 1, avg_pool1d over 2 A + 1, the product and a clamp (fp32 average: it
                      is NOT the stage's arithmetic, only its shape); as many launches per window as fit ~0.2 s, at least 3
  call_ms             master() end to end (table upload, both entries, synchronise) by the host clock

    python tools/master_bench.py [--repeat 7] [--launches 200]      -> one JSON line, profiles/master_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusynth_amd import _lib as L  # noqa: E402
from diffusynth_amd import arranger as A  # noqa: E402

SR, N = 16000, 960000


def track(seed):
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    x = 0.4 * np.sin(2 * np.pi * 55.0 * t / SR) + 0.05 * rng.standard_normal(N)
    x = np.where((t // 40000) % 3 == 2, 0.05 * x, x)
    x[rng.integers(0, N, 40)] *= 8.0
    return x.astype(np.float32)


def events_us(fn, launches, repeat):
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


def wall_ms(fn, repeat):
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def entries(x, n_signals, m, a, r):
    MS = L.MS
    tab = torch.from_numpy(A._flat_table([N] * n_signals).reshape(-1)).cuda()
    ws = torch.empty(L.load().ds_master_ws_bytes(n_signals, N) // 8 + 1, dtype=torch.float64, device="cuda")
    stats = torch.empty((n_signals, MS["DS_MS_NS"]), dtype=torch.float32, device="cuda")
    limited = torch.empty(n_signals, dtype=torch.int32, device="cuda")
    out = torch.empty_like(x)
    st = L.current_stream()
    f32 = lambda v: float(np.float32(v))          # noqa: E731
    keep = (tab, ws, stats, limited, out)
    return {"gain_us": lambda: L.call("ds_master_gain", x.data_ptr(), tab.data_ptr(), n_signals, N, x.numel(), f32(m.target_rms), f32(m.max_gain), ws.data_ptr(),
                                      stats.data_ptr(), limited.data_ptr(), st),
            "limit_us": lambda: L.call("ds_master_limit", x.data_ptr(), tab.data_ptr(), n_signals, N, x.numel(), f32(m.ceiling), a, r, stats.data_ptr(),
                                       limited.data_ptr(), out.data_ptr(), None, st)}, keep


def torch_chain(x2, m, a, r):
    """x2 (B, N) -> y (B, N): the shape of the stage in torch ops."""
    c = float(np.float32(m.ceiling))
    rms = x2.double().pow(2).mean(dim=1, keepdim=True).sqrt()
    gl = torch.clamp(m.target_rms / rms, max=m.max_gain).float()
    u = gl * x2
    au = u.abs()
    req = torch.where(au > c, c / au, torch.ones_like(au))
    ext = F.pad(req, (a + r, 2 * a), value=1.0)
    hold = -F.max_pool1d(-ext.unsqueeze(1), r + a + 1, stride=1)
    g = F.avg_pool1d(hold, 2 * a + 1, stride=1).squeeze(1)
    return torch.clamp(g * u, -c, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)       # what a float4 copy reaches on an MI355X (8.0 is the data sheet)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "master_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("master_bench: needs an MI355X; there is nothing to measure without one")
    repeat = max(5, args.repeat)
    res = {"tool": "tools/master_bench.py", "device": torch.cuda.get_device_name(0), "repeat": repeat, "launches": args.launches, "samples": N,
           "hbm_tbs": args.hbm_tbs, "cases": {}}
    tracks = torch.from_numpy(np.stack([track(k) for k in range(8)])).cuda()
    for label, m in (("default", A.Mastering()), ("caps", A.Mastering(lookahead=1024.5 / SR, hold=8192.5 / SR))):
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
            row["floor_us"] = round(12.0 * x.numel() / (args.hbm_tbs * 1e12) * 1e6, 3)
            chain = lambda: torch_chain(x2, m, a, r)                         # noqa: E731
            chain()
            one = wall_ms(chain, 1)
            row["torch_launches"] = int(min(args.launches, max(3, 200.0 / max(one, 1e-3))))
            row["torch_us"] = round(events_us(chain, row["torch_launches"], repeat), 3)
            job = lambda: A.master(x2, m, sample_rate=SR)                    # noqa: E731
            job(), job()
            row["call_ms"] = round(wall_ms(job, repeat), 4)
            got, want = A.master(x2, m, sample_rate=SR), chain()
            row["max_abs_diff_to_torch_chain"] = float((got - want).abs().max())
            res["cases"][f"{label}_x{b}"] = row
            print(label, b, row, flush=True)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
