"""What the formant-preserving mode of the arranger's pitch shifter costs (diffusynth_amd.arranger.Formant, ds_pv_formant).

Workload: that of tools/arranger_bench.py — the reference's five preset MIDI files (message lists of tests/golden/arranger.npz), two tracks
each, max_notes = 100, two instruments — with the seeded synthetic notes of tests/arranger_ref.py in place of sampled ones: they have the
package's note length for every duration, and nothing in the audio stage depends on what a note holds, so the launches are the same.
In one process, after one untimed pass of both modes:

  arrange      per preset, DiffSynth.arrange with formant=None and with Formant(), ALTERNATING, wall clock around a device synchronise, the
               median (and the smallest and largest) of --repeat runs each; launches counted from the entry points called; next to it the
               parent commit's audio_s and launches from profiles/arranger_bench.json (formant=None must be the same launches)
  level        the widest tree level of --level-preset: one batched pitch_shift of all its nodes (arranger._shift_flat: table upload, the
               entry points, the allocations) with and without a Formant, alternating, device events around --level-reps calls per window,
               the median of --repeat windows
  kernels      on that level's tables, already on the device: device events around back-to-back calls of each entry point by itself, the
               median of --repeat windows -> us per call, the share of the level's kernel time, and for ds_pv_formant the rate against its
               byte model, 2 x 2049 x 8 B per synthesis frame (one read and one write of the frame).  ds_pv_formant works in place, so its
               window is --kernel-reps calls behind one restoring copy (the copy is outside the events)

Writes one JSON document (--out, default profiles/formant_bench.json) and prints it.

    python tools/formant_bench.py [--presets A,B] [--repeat 7] [--out profiles/formant_bench.json]
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

import arranger_ref as R  # noqa: E402
from diffusynth_amd import _lib as L  # noqa: E402
from diffusynth_amd import arranger as A  # noqa: E402

PRESETS = ("Ode_to_Joy_Easy_variation", "Air_on_the_G_String", "Canon_in_D", "Arhbo", "Rrharil")
KERNELS = {"ds_pv_stft": 1, "ds_pv_vocode": 1, "ds_pv_formant": 1, "ds_pv_istft": 2, "ds_resample_sinc": 1, "ds_peak_normalize": 2, "ds_mix_notes": 1,
           "ds_mix_notes_shaped": 1}
NAMES = ["organ", "string"]
NB = A.N_FFT // 2 + 1


def spread(ts, digits=6):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def events_us(fn, reps, before=None):
    """us per call: device events around `reps` back-to-back calls (before(): untimed, ahead of the first event)."""
    if before is not None:
        before()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def counted(fn):
    counts, call = {}, L.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return call(name, *args)
    A.L.call = counting
    try:
        fn()
    finally:
        A.L.call = call
    return counts


def arrange_bench(g, name, repeat, fm, parent):
    tpb = int(g[name + ".tpb"])
    tracks = [A.Track(R.messages(g[f"{name}.t{k}.msgs"]), tpb, 100) for k in range(int(g[name + ".n_tracks"]))]
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda")
    wanted = list(dict.fromkeys(ds.wanted_notes(tracks, NAMES)))
    notes = {w: torch.from_numpy(R.synthetic_note(w[1])).cuda() for w in wanted}
    levels = [A.shift_tree([(s[0], s[3]) for s in t.schedule()]) for t in tracks]
    row = {"distinct_notes": len(wanted), "tree_nodes": sum(len(lv) for ls in levels for lv in ls), "tree_levels": [len(ls) for ls in levels]}
    modes = {"none": None, "formant": fm}
    for mode, f in modes.items():                          # warm-up, launches
        counts = counted(lambda f=f: ds.arrange(tracks, NAMES, notes, formant=f))
        row[mode] = {"launches": sum(KERNELS.get(k, 0) * v for k, v in counts.items()), "ds_pv_formant_calls": counts.get("ds_pv_formant", 0)}
    ts = {mode: [] for mode in modes}
    for _ in range(repeat):                                # alternating
        for mode, f in modes.items():
            ts[mode].append(wall(lambda f=f: ds.arrange(tracks, NAMES, notes, formant=f)))
    for mode in modes:
        row[mode]["audio_s"] = spread(ts[mode])
    row["formant_over_none"] = round(row["formant"]["audio_s"]["median"] / row["none"]["audio_s"]["median"], 4)
    music = ds.arrange(tracks, NAMES, notes, formant=fm)
    row["music_samples"], row["finite"] = music.numel(), bool(torch.isfinite(music).all())
    if parent is not None and name in parent.get("presets", {}):
        p = parent["presets"][name]
        row["parent"] = {"audio_s": p.get("audio_s"), "launches": p.get("launches"), "source": "profiles/arranger_bench.json (notes sampled by the U-Net there)"}
        if p.get("audio_s"):
            row["none_over_parent"] = round(row["none"]["audio_s"]["median"] / p["audio_s"], 4)
        row["none_launches_equal_parent"] = p.get("launches") == row["none"]["launches"]
    return row, tracks, notes


def level_bench(tracks, notes, repeat, level_reps, kernel_reps, fm):
    """The widest level of the preset's trees: the batched shift end to end, then every entry point by itself on its tables."""
    best = None
    for i, t in enumerate(tracks):
        sched = t.schedule()
        for li, nodes in enumerate(A.shift_tree([(s[0], s[3]) for s in sched])):
            if li == 0 and (best is None or len(nodes) > len(best[1])):
                best = (i, nodes, {s[0]: s[1] for s in sched})
    i, nodes, dur = best
    srcs = A.peak_normalize([notes[(NAMES[i], dur[k])] for k, _, _, _ in nodes])
    lengths, steps = [s.numel() for s in srcs], [st for _, _, _, st in nodes]
    orders = A.node_orders(nodes, fm)
    x = torch.cat(srcs)
    out = {"track": i, "nodes": len(nodes), "samples": int(x.numel()), "n_steps": steps, "orders": orders}
    modes = {"none": (), "formant": (fm, orders)}
    for args in modes.values():
        A._shift_flat(x, lengths, steps, *args)
    ts = {m: [] for m in modes}
    for _ in range(repeat):
        for m, args in modes.items():
            ts[m].append(events_us(lambda args=args: A._shift_flat(x, lengths, steps, *args), level_reps))
    out["shift_us"] = {m: spread(ts[m], 2) for m in modes}
    out["shift_formant_over_none"] = round(out["shift_us"]["formant"]["median"] / out["shift_us"]["none"]["median"], 4)
    # every entry point by itself
    p = A._Plan(lengths, steps, orders)
    tables = torch.from_numpy(p.host).cuda()
    b = tables.data_ptr()
    rates, tab, idx, alpha, order, warp = b, b + 4 * p.o_tab, b + 4 * p.o_idx, b + 4 * p.o_alpha, b + 4 * p.o_order, b + 4 * p.o_warp
    dev = x.device
    spec = torch.empty(p.total_frames * NB * 2, dtype=torch.float32, device=dev)
    voc = torch.empty(p.total_out * NB * 2, dtype=torch.float32, device=dev)
    ws = torch.empty(L.load().ds_pv_istft_ws_bytes(p.total_out) // 4, dtype=torch.float32, device=dev)
    ys = torch.empty(p.total_stretched, dtype=torch.float32, device=dev)
    res = torch.empty(p.total_samples, dtype=torch.float32, device=dev)
    st = L.current_stream()
    calls = {
        "ds_pv_stft": lambda: L.call("ds_pv_stft", x.data_ptr(), tab, p.n, p.max_frames, p.total_samples, p.total_frames, spec.data_ptr(), st),
        "ds_pv_vocode": lambda: L.call("ds_pv_vocode", spec.data_ptr(), tab, idx, alpha, p.n, p.total_frames, p.total_out, voc.data_ptr(), st),
        "ds_pv_formant": lambda: L.call("ds_pv_formant", voc.data_ptr(), tab, order, warp, fm.limit, p.n, p.max_out, p.total_out, st),
        "ds_pv_istft": lambda: L.call("ds_pv_istft", voc.data_ptr(), tab, p.n, p.max_out, p.max_stretched, p.total_out, p.total_stretched, ws.data_ptr(),
                                      ys.data_ptr(), st),
        "ds_resample_sinc": lambda: L.call("ds_resample_sinc", ys.data_ptr(), tab, rates, p.n, p.max_len, p.total_stretched, p.total_samples,
                                           res.data_ptr(), st),
    }
    calls["ds_pv_stft"]()
    calls["ds_pv_vocode"]()
    pristine = voc.clone()
    for fn in calls.values():
        fn()
    us = {k: [] for k in calls}
    for _ in range(repeat):
        for k, fn in calls.items():
            us[k].append(events_us(fn, kernel_reps, before=lambda: voc.copy_(pristine)))
    voc.copy_(pristine)
    out["frames"] = {"analysis": p.total_frames, "synthesis": p.total_out}
    out["kernel_us"] = {k: spread(v, 2) for k, v in us.items()}
    med = {k: out["kernel_us"][k]["median"] for k in calls}
    out["formant_share_of_level_kernel_time"] = round(med["ds_pv_formant"] / sum(med.values()), 4)
    out["formant_over_stft_plus_istft"] = round(med["ds_pv_formant"] / (med["ds_pv_stft"] + med["ds_pv_istft"]), 4)
    model = 2 * NB * 8 * p.total_out
    out["formant_byte_model"] = {"bytes": model, "bytes_per_frame": 2 * NB * 8, "GB_per_s": round(model / (med["ds_pv_formant"] * 1e-6) / 1e9, 1),
                                 "blocks": sum((int(n) + 1) // 2 for n in p.host[p.o_tab:p.o_idx].reshape(-1, L.PV["DS_PV_NI"])[:, L.PV["DS_PV_NOUT"]])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default=",".join(PRESETS))
    ap.add_argument("--level-preset", default="Arhbo")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--level-reps", type=int, default=20)
    ap.add_argument("--kernel-reps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formant_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("formant_bench: no GPU (there is nothing to measure without one)")
    g = np.load(os.path.join(ROOT, "tests", "golden", "arranger.npz"), allow_pickle=False)
    parent = None
    ppath = os.path.join(ROOT, "profiles", "arranger_bench.json")
    if os.path.exists(ppath):
        with open(ppath) as f:
            parent = json.load(f)
    fm = A.Formant()
    res = {"tool": "tools/formant_bench.py", "device": torch.cuda.get_device_name(0), "repeat": a.repeat, "max_notes": 100,
           "formant": {"order": fm.order, "max_gain_db": fm.max_gain_db, "track_pitch": fm.track_pitch}, "notes": "synthetic (tests/arranger_ref.py)",
           "presets": {}}
    names = a.presets.split(",")
    kept = {}
    for name in names:
        row, tracks, notes = arrange_bench(g, name, a.repeat, fm, parent)
        res["presets"][name] = row
        kept[name] = (tracks, notes)
        print(f"[formant_bench] {name}: {row}", file=sys.stderr, flush=True)
    lp = a.level_preset if a.level_preset in kept else names[0]
    res["level"] = {"preset": lp, "calls_per_window": a.level_reps, "kernel_calls_per_window": a.kernel_reps, **level_bench(*kept[lp], a.repeat, a.level_reps, a.kernel_reps, fm)}
    print(f"[formant_bench] level: {res['level']}", file=sys.stderr, flush=True)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
