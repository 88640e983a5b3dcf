"""What pitch detection and the arranger's tuned mode cost (diffusynth_amd.pitch, arranger tune=).  Recorded, not judged: nobody had
measured these before, so there is no threshold.

In one process, every timed call warmed up first, each figure the median of --repeat (>= 5) runs:

  estimate_pitch   40 notes of 28 416 ... 77 568 samples (the presets' note lengths: latent widths 28 ... 76) as one batch: two launches and
                   one device -> host copy.  event_ms: device events around the call (they close after the copy); wall_ms: host clock
                   around the call, which ends in that copy.  frames_ms: ds_yin_frames alone (pitch.yin), by events.
  host             the float64 restatement (tests/pitch_ref.py, numpy, one process) on ONE such note: one run
  arrange          DiffSynth.arrange on a synthetic 100-event track (notes 40 ... 75 from given notes at MIDI 50.37, four durations: no
                   U-Net) with tune=None, tune=52 and tune="detect"; wall clock around a device synchronise, tree nodes and levels beside it

Prints one JSON line and writes it to profiles/pitch_bench.json.

    python tools/pitch_bench.py [--repeat 7]
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
import pitch_ref as P  # noqa: E402
from diffusynth_amd import arranger as A  # noqa: E402
from diffusynth_amd import pitch  # noqa: E402


def by_events(fn, repeat):
    """(median ms by device events, median ms by the host clock, last result); fn is warm."""
    ev, wall, out = [], [], None
    for _ in range(repeat):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return statistics.median(ev), statistics.median(wall), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pitch_bench: needs an MI355X; there is nothing to measure without one")
    repeat = max(5, args.repeat)
    res = {"tool": "tools/pitch_bench.py", "device": torch.cuda.get_device_name(0), "repeat": repeat}

    # ---- estimate_pitch on 40 notes
    lengths = [256 * (4 * int(w) - 1) for w in np.linspace(28, 76, 40).round()]
    assert lengths[0] == 28416 and lengths[-1] == 77568
    host_notes = [R.probe_signal(n, seed=i, f0=110.0 * 2 ** (i / 13.0)) for i, n in enumerate(lengths)]
    notes = [torch.from_numpy(x).cuda() for x in host_notes]
    frames = [pitch.frame_count(n, 1024, 290, 256) for n in lengths]
    pitch.estimate_pitch(notes), pitch.yin(notes)                              # warm-up
    ev, wall, est = by_events(lambda: pitch.estimate_pitch(notes), repeat)
    fev, _, _ = by_events(lambda: pitch.yin(notes), repeat)
    want = np.array([69 + 12 * np.log2(110.0 * 2 ** (i / 13.0) / 440.0) for i in range(40)])
    res["estimate_pitch"] = {"notes": 40, "samples": int(sum(lengths)), "frames": int(sum(frames)), "event_ms": round(ev, 4), "wall_ms": round(wall, 4),
                             "yin_frames_event_ms": round(fev, 4), "difference_gflop": round(3 * 291 * 1024 * sum(frames) / 1e9, 3),
                             "worst_cents_from_the_tones": round(float(np.abs(est.midi - want).max() * 100), 4), "unpitched": int(np.isnan(est.midi).sum())}
    # ---- the float64 restatement on one note, on the host
    t0 = time.perf_counter()
    f0, midi, voiced, n = P.estimate(host_notes[0])
    res["host_restatement_float64_one_note"] = {"samples": lengths[0], "frames": int(n), "s": round(time.perf_counter() - t0, 4),
                                                "device_minus_host_cents": round(float(est.midi[0] - midi) * 100, 6)}

    # ---- arrange on a synthetic 100-event track
    rng = np.random.default_rng(0)
    durs = (720, 960, 1440, 1920)
    events = [(int(rng.integers(40, 76)), int(durs[rng.integers(0, 4)])) for _ in range(100)]
    track = A.Track(P.note_messages(events, gap=0), P.TPB, 100)
    keys = list(dict.fromkeys((s[0], s[1]) for s in track.schedule()))
    given = {("probe", dur): torch.from_numpy(R.probe_signal(256 * (4 * int(256 * ((dur + 1) / 4) / 4) - 1), seed=i, f0=150.0)).cuda()
             for i, (_, dur) in enumerate(keys)}
    res["arrange"] = {"events": 100, "distinct_notes": len(given), "track_samples": track.track_length()}
    for tune in (None, 52, "detect"):
        ds = A.DiffSynth({}, None, None, None, None, None, "cuda", tune=tune)
        ds.arrange([track], ["probe"], given)                                   # warm-up
        _, wall, out = by_events(lambda: ds.arrange([track], ["probe"], given), repeat)
        if tune is None:
            levels = A.shift_tree([(s[0], s[3]) for s in track.schedule()])
        else:
            p = {k: 52.0 for k, _ in keys} if tune == 52 else {k: ds.last_pitches[("probe", dur)] for k, dur in keys}
            levels = A.signed_tree([(s[0], (s[3] + 52) - p[s[0]]) for s in track.schedule()])
        res["arrange"][f"tune={tune!r}"] = {"wall_ms": round(wall, 4), "tree_nodes": sum(len(lv) for lv in levels), "tree_levels": len(levels),
                                            "finite": bool(torch.isfinite(out).all())}
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
