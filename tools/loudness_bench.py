"""What the loudness meter costs on the device (diffusynth_amd.loudness, ds_loudness), beside its byte floor and beside the same measurement
on the host.

Workload: one 60 s track at 16 kHz (960 000 samples) and a batch of 8 of them, the mastering bench's tracks.  In one process, every case
warmed first:

  loudness_us   device time of ONE call of ds_loudness (its four kernels) on a table built once: device events around --launches back-to-back
                calls on one stream, divided by their number; median of --repeat windows
  gain_us       the same for ds_loudness_gain
  floor_us      8 bytes per sample (x is read twice) at --hbm-tbs TB/s
  host_ms       scipy.signal.lfilter twice plus numpy gating on this host's CPU, float64, per batch (null without scipy); the host's clock
  call_ms       loudness() end to end (table upload, ds_loudness, synchronise) by the host clock
  master_ms     master() to a LUFS target end to end, beside master() to an RMS target (master_rms_ms)

    python tools/loudness_bench.py [--repeat 7] [--launches 200]      -> one JSON line, profiles/loudness_bench.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from diffusynth_amd import _lib as L  # noqa: E402
from diffusynth_amd import arranger as A  # noqa: E402
from master_bench import N, SR, events_us, track, wall_ms  # noqa: E402

LM = importlib.import_module("diffusynth_amd.loudness")


def entries(x, n_signals):
    LU, MS = L.LU, L.MS
    h = LM.hop(SR)
    tab = torch.from_numpy(A._flat_table([N] * n_signals).reshape(-1)).cuda()
    ws = torch.empty(L.load().ds_loudness_ws_bytes(n_signals, N, h) // 8, dtype=torch.float64, device="cuda")
    lu = torch.empty((n_signals, LU["DS_LU_NS"]), dtype=torch.float64, device="cuda")
    cnt = torch.empty((n_signals, 3), dtype=torch.int32, device="cuda")
    stats = torch.empty((n_signals, MS["DS_MS_NS"]), dtype=torch.float32, device="cuda")
    coef = LM._coefficients(SR)
    st = L.current_stream()
    keep = (tab, ws, lu, cnt, stats, coef)
    return {"loudness_us": lambda: L.call("ds_loudness", x.data_ptr(), tab.data_ptr(), n_signals, N, x.numel(), coef.ctypes.data, h, LM.Z_ABS, ws.data_ptr(),
                                          lu.data_ptr(), cnt.data_ptr(), None, 0, st),
            "gain_us": lambda: L.call("ds_loudness_gain", lu.data_ptr(), n_signals, LM.energy_of(-16.0), 10.0, stats.data_ptr(), st)}, keep


def host_loudness(x2):
    """The measurement a user would make on the host: lfilter twice, block energies by a cumulative sum, the two gates -> LUFS per signal."""
    from scipy.signal import lfilter
    (b1, a1), (b2, a2) = LM.kweighting(SR)
    h = LM.hop(SR)
    out = []
    for x in x2:
        y = lfilter(b2, a2, lfilter(b1, a1, x.astype(np.float64)))
        q = (y[:len(y) // h * h] ** 2).reshape(-1, h).sum(axis=1)
        z = (q[:-3] + q[1:-2] + q[2:-1] + q[3:]) / (4.0 * h)
        j1 = z[z > LM.Z_ABS]
        j2 = j1[j1 > 0.1 * j1.mean()] if len(j1) else j1
        out.append(-0.691 + 10.0 * np.log10(j2.mean()) if len(j2) else -np.inf)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)       # what a float4 copy reaches on an MI355X (8.0 is the data sheet)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_bench: needs an MI355X; there is nothing to measure without one")
    repeat = max(5, args.repeat)
    res = {"tool": "tools/loudness_bench.py", "device": torch.cuda.get_device_name(0), "repeat": repeat, "launches": args.launches, "samples": N,
           "sample_rate": SR, "hbm_tbs": args.hbm_tbs, "host_cpus": os.cpu_count(), "cases": {}}
    host_tracks = np.stack([track(k) for k in range(8)])
    tracks = torch.from_numpy(host_tracks).cuda()
    m_lufs, m_rms = A.Mastering(target_rms=None, target_lufs=-16.0), A.Mastering()
    for b in (1, 8):
        x2 = tracks[:b].contiguous()
        x = x2.reshape(-1)
        calls, keep = entries(x, b)
        for fn in calls.values():
            fn(), fn()
        torch.cuda.synchronize()
        row = {"signals": b}
        row.update({k: round(events_us(fn, args.launches, repeat), 3) for k, fn in calls.items()})
        row["floor_us"] = round(8.0 * x.numel() / (args.hbm_tbs * 1e12) * 1e6, 3)
        job = lambda: LM.loudness(x2, SR)                                       # noqa: E731
        job(), job()
        row["call_ms"] = round(wall_ms(job, repeat), 4)
        for key, m in (("master_ms", m_lufs), ("master_rms_ms", m_rms)):
            job = lambda: A.master(x2, m, sample_rate=SR)                        # noqa: E731
            job(), job()
            row[key] = round(wall_ms(job, repeat), 4)
        got = LM.loudness(x2, SR).integrated.cpu().numpy()
        try:
            want = host_loudness(host_tracks[:b])
            row["host_ms"] = round(wall_ms(lambda: host_loudness(host_tracks[:b]), 5), 3)
            row["max_lu_diff_to_host"] = float(np.max(np.abs(got - np.array(want))))
        except ImportError:
            row["host_ms"] = row["max_lu_diff_to_host"] = None
        row["integrated_lufs"] = [round(float(v), 4) for v in got]
        res["cases"][f"x{b}"] = row
        print(b, row, flush=True)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
