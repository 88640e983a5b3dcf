"""What the Arrangement tab's audio stage costs beside the sampling of its notes (diffusynth_amd.arranger.DiffSynth).

Workload: the reference's five preset MIDI files (message lists of tests/golden/arranger.npz), two tracks each, max_notes = 100, two
synthetic-weight instruments, 20 inpaint steps (DDPM, dynamic masks), bf16x3 U-Net, fp32 decoder tier.  Per preset, in one process,
after one untimed warm-up pass, each figure the median of --repeat (>= 5) runs, wall clock around a device synchronise:

  notes_s      sample_notes: every distinct (instrument, duration) note through one SamplingBatcher, then VQ, decoder, ISTFT+ / iSTFT
  audio_s      arrange: peak normalisation, the chains' shared-prefix tree level by level, one mix per track, the sum of the tracks
  share        audio_s / notes_s — the gate is share <= 0.10
  launches     kernels the library launched for arrange (from the entry points called; torch's concatenations and the final sum are
               not counted), levels and nodes of the trees, distinct notes and latent widths
  host_s       (--what host) the float64 RESTATEMENT of the same stage (tests/arranger_ref.py; not librosa, which is not installed) on the same
               notes, the nodes of a level spread over 16 processes: one run

  mix          (--what mix, a run of its own) the performed mix next to the plain mix of the SAME schedule: Canon in D track 0 read with
               pairing="midi", first 100 notes, the default Performance's sampled durations and starts, synthetic notes; ds_mix_notes over
               the whole notes against ds_mix_notes_shaped with velocity gains and gated envelopes, alternating in one process, device
               events around --mix-reps launches on tables already on the device, the median of --repeat windows each -> "mix" in the JSON;
               --parent-lib OTHER.so times ds_mix_notes of another build of the library (the parent commit's) in the same alternation

Prints one JSON line (-> profiles/arranger_bench.json).  --what audio --presets NAME is the run to put under a kernel trace.

    python tools/arranger_bench.py [--what notes,audio,host,mix] [--presets A,B] [--repeat 5]
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
from diffusynth_amd.synth import synth_input, synth_state_dict  # noqa: E402

PRESETS = ("Ode_to_Joy_Easy_variation", "Air_on_the_G_String", "Canon_in_D", "Arhbo", "Rrharil")
KERNELS = {"ds_pv_stft": 1, "ds_pv_vocode": 1, "ds_pv_istft": 2, "ds_resample_sinc": 1, "ds_peak_normalize": 2, "ds_mix_notes": 1, "ds_mix_notes_shaped": 1}
NAMES = ["organ", "string"]


def timed(fn, repeat):
    out, ts = None, []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def _host_node(args):
    y, st = args
    return R.pitch_shift(y, st)


def host_stage(tracks, notes, pool):
    """The restatement of arrange() on the host (float64), the nodes of a level in parallel."""
    t0 = time.perf_counter()
    audios = []
    for i, t in enumerate(tracks):
        sched = t.schedule()
        have = {}
        for key, dur, _, _ in sched:
            if (key, 0) not in have:
                s = notes[(NAMES[i], dur)]
                have[(key, 0)] = s / np.max(np.abs(s))
        for nodes in A.shift_tree([(s[0], s[3]) for s in sched]):
            for (k, _, cum, _), y in zip(nodes, pool.map(_host_node, [(have[(k, lo)], st) for k, lo, _, st in nodes])):
                have[(k, cum)] = y
        audio = np.zeros(t.track_length(), dtype=np.float32)
        for key, _, start, total in sched:
            note = have[(key, max(total, 0))]
            audio[start:start + len(note)] += note
        audios.append(audio)
    full = np.zeros(max(len(a) for a in audios), dtype=np.float32)
    for a in audios:
        full[:len(a)] += a
    return time.perf_counter() - t0, full


def mix_bench(g, repeat, reps, parent_lib=None):
    """us per launch of the plain and of the performed mix of one schedule, through the C entry points on tables built once."""
    name = "Canon_in_D"
    t = A.Track(R.messages(g[name + ".t0.msgs"]), int(g[name + ".tpb"]), 100, pairing="midi")
    perform = A.Performance()
    sched = t.schedule(perform=perform)
    keys = list(dict.fromkeys(s[0] for s in sched))
    dur = {s[0]: s[1] for s in sched}
    notes = A.peak_normalize([torch.from_numpy(R.synthetic_note(dur[k])).cuda() for k in keys])
    events = [(s[2], keys.index(s[0])) for s in sched]
    n = max(start + notes[i].numel() for start, i in events)
    gains, envs = t.shape(perform=perform)
    out = {"preset": name, "events": len(events), "distinct_notes": len(keys), "track_samples": n, "launches_per_window": reps,
           "plain": {"us": []}, "performed": {"us": []}}
    # the tables of both launches, built once from the package's public pieces and kept on the device
    lengths = [x.numel() for x in notes]
    offs = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    starts, note_off, note_len = [s for s, _ in events], [offs[i] for _, i in events], [lengths[i] for _, i in events]
    flat, st = torch.cat(notes), L.current_stream()
    tracks, launches = {}, {}
    for kind, fn, ev in (("plain", "ds_mix_notes", np.array(list(zip(starts, note_off, note_len)), dtype=np.int32)),
                         ("performed", "ds_mix_notes_shaped", A.shaped_rows(starts, note_off, note_len, gains, envs))):
        ptr, lst = A.mix_lists(ev[:, L.MX["DS_MX_START"]].tolist(), ev[:, L.MX["DS_MX_LEN"]].tolist(), n)
        tables = torch.from_numpy(np.concatenate([ev.reshape(-1), ptr, lst, np.zeros(1, np.int32)])).cuda()
        tracks[kind] = torch.empty(n, dtype=torch.float32, device="cuda")
        base = tables.data_ptr()
        launches[kind] = (tables, (fn, flat.data_ptr(), flat.numel(), base, len(ev), base + 4 * ev.size, base + 4 * (ev.size + ptr.size), len(lst),
                                   tracks[kind].data_ptr(), n, st))
        out[kind]["entry"], out[kind]["block_list_entries"] = fn, len(lst)
        L.call(*launches[kind][1])                       # warm-up
    kinds, run = ["plain", "performed"], {"plain": L.call, "performed": L.call}
    if parent_lib:                                       # ds_mix_notes of ANOTHER build of the library (the parent commit's) on the plain tables
        import ctypes
        other = ctypes.CDLL(os.path.abspath(parent_lib))
        other.ds_mix_notes.restype, other.ds_mix_notes.argtypes = L._PROTOS["ds_mix_notes"]
        tracks["plain_parent"] = torch.empty(n, dtype=torch.float32, device="cuda")
        args = list(launches["plain"][1])
        args[8] = tracks["plain_parent"].data_ptr()
        launches["plain_parent"] = (launches["plain"][0], tuple(args))

        def call_other(fn, *a):
            assert getattr(other, fn)(*a) == 0, fn
        kinds, run["plain_parent"] = ["plain_parent"] + kinds, call_other
        out["plain_parent"] = {"us": [], "entry": "ds_mix_notes", "library": os.path.basename(parent_lib), "block_list_entries": out["plain"]["block_list_entries"]}
        call_other(*launches["plain_parent"][1])
    for _ in range(repeat):                              # alternating
        for kind in kinds:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                run[kind](*launches[kind][1])
            t1.record()
            t1.synchronize()
            out[kind]["us"].append(t0.elapsed_time(t1) * 1e3 / reps)
    plain, shaped = tracks["plain"], tracks["performed"]
    assert torch.equal(plain, A.mix_notes(notes, events, n)) and torch.equal(shaped, A.mix_notes(notes, events, n, gains=gains, envelopes=envs))
    if parent_lib:
        torch.cuda.synchronize()
        out["plain_equals_parent_bit_for_bit"] = bool(torch.equal(tracks["plain_parent"], plain))
    for row in [out[k] for k in kinds]:
        row["us_median"], row["us_min"], row["us_max"] = round(statistics.median(row["us"]), 3), round(min(row["us"]), 3), round(max(row["us"]), 3)
        del row["us"]
    mixed = t.mixed_lengths({k: x.numel() for k, x in zip(keys, notes)}, perform=perform)
    out["plain"]["note_samples_read"] = sum(notes[i].numel() for _, i in events)
    out["performed"]["note_samples_read"] = sum(mixed)
    out["performed_over_plain"] = round(out["performed"]["us_median"] / out["plain"]["us_median"], 4)
    if parent_lib:
        out["performed_over_plain_parent"] = round(out["performed"]["us_median"] / out["plain_parent"]["us_median"], 4)
        out["plain_over_plain_parent"] = round(out["plain"]["us_median"] / out["plain_parent"]["us_median"], 4)
    out["finite"] = bool(torch.isfinite(plain).all() and torch.isfinite(shaped).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix-reps", type=int, default=200)
    ap.add_argument("--parent-lib", default=None, help="--what mix: another build of the library (the parent commit's) whose ds_mix_notes is timed beside")
    ap.add_argument("--what", default="notes,audio")
    ap.add_argument("--presets", default=",".join(PRESETS))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    what = set(a.what.split(","))
    if what == {"mix"}:
        g = np.load(os.path.join(ROOT, "tests", "golden", "arranger.npz"), allow_pickle=False)
        print(json.dumps({"tool": "tools/arranger_bench.py", "device": torch.cuda.get_device_name(0), "repeat": a.repeat,
                          "mix": mix_bench(g, a.repeat, a.mix_reps, a.parent_lib)}), flush=True)
        return
    pool = None
    if "host" in what:
        import multiprocessing as mp
        pool = mp.get_context("fork").Pool(16)           # forked BEFORE this process opens the device: the children only ever run numpy
    from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet
    from diffusynth_amd.vqgan import PRODUCTION_CONFIG as VQ_CFG, VQGAN
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        keys = json.load(f)
    net = ConditionedUnet(**PRODUCTION_CONFIG)
    net.load_state_dict(synth_state_dict([(k, tuple(s)) for k, s in keys["unet_production"]]))
    net.to("cuda").set_compute_dtype("bf16x3")
    vae = VQGAN(**VQ_CFG)
    vae.load_state_dict(synth_state_dict([(k, tuple(s)) for k, s in keys["vqgan_production"]]))
    vae.to("cuda")
    vae._decoder.set_compute_dtype("fp32")
    g = np.load(os.path.join(ROOT, "tests", "golden", "arranger.npz"), allow_pickle=False)
    cfg = lambda tag: dict(sample_steps=a.steps, sampler="ddpm", noising_strength=0.7, attack=0.5, before_release=0.5,      # noqa: E731
                           latent_representation=synth_input("arr_guide_" + tag, (1, 4, 128, 64)).cuda())
    ds = A.DiffSynth({NAMES[0]: cfg("a"), NAMES[1]: cfg("b")}, net, vae._vq_vae, vae._decoder, None, None, "cuda",
                     condition=synth_input("arr_cond", (1, 512)).cuda(), seed=1)
    res = {"tool": "tools/arranger_bench.py", "device": torch.cuda.get_device_name(0), "unet_tier": "bf16x3", "decoder_tier": "fp32",
           "inpaint_steps": a.steps, "max_notes": 100, "repeat": a.repeat, "presets": {}}
    for name in a.presets.split(","):
        tpb = int(g[name + ".tpb"])
        tracks = [A.Track(R.messages(g[f"{name}.t{k}.msgs"]), tpb, 100) for k in range(int(g[name + ".n_tracks"]))]
        wanted = ds.wanted_notes(tracks, NAMES)
        levels = [A.shift_tree([(s[0], s[3]) for s in t.schedule()]) for t in tracks]
        row = {"distinct_notes": len(set(wanted)), "latent_widths": sorted({ds.note_width(d) for _, d in wanted}),
               "pitch_shift_calls_reference": sum(len(A.chain_steps(s[3])) for t in tracks for s in t.schedule()),
               "tree_nodes": sum(len(lv) for ls in levels for lv in ls), "tree_levels": [len(ls) for ls in levels]}
        notes = ds.sample_notes(wanted)                   # warm-up (plans of every width, allocator)
        ds.arrange(tracks, NAMES, notes)
        if "notes" in what:
            row["notes_s"], notes = timed(lambda: ds.sample_notes(wanted), a.repeat)
            row["notes_s"] = round(row["notes_s"], 5)
        if "audio" in what:
            counts, call = {}, L.call

            def counting(fn, *args):
                counts[fn] = counts.get(fn, 0) + 1
                return call(fn, *args)
            A.L.call = counting
            try:
                ds.arrange(tracks, NAMES, notes)
            finally:
                A.L.call = call
            row["launches"] = sum(KERNELS.get(k, 0) * v for k, v in counts.items())
            t_audio, music = timed(lambda: ds.arrange(tracks, NAMES, notes), a.repeat)
            row["audio_s"] = round(t_audio, 5)
            row["music_samples"], row["finite"] = music.numel(), bool(torch.isfinite(music).all())
            if "notes_s" in row:
                row["share"] = round(row["audio_s"] / row["notes_s"], 4)
                row["gate_share_le_0.10"] = row["share"] <= 0.10
        if pool is not None:
            t_host, full = host_stage(tracks, {k: v.cpu().numpy() for k, v in notes.items()}, pool)
            row["host_restatement_float64_16_processes_s"] = round(t_host, 3)
            if "audio" in what:
                d = music.cpu().numpy().astype(np.float64) - full
                row["device_vs_restatement_rms_rel"] = float(np.linalg.norm(d) / np.linalg.norm(full))
        res["presets"][name] = row
        print(f"[arranger_bench] {name}: {row}", file=sys.stderr, flush=True)
    if pool is not None:
        pool.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
