#!/usr/bin/env python3
"""Generate tests/golden/arranger.npz by running the reference's own Track (webUI/natural_language_guided_4/track_maker.py).

Runs only where the reference tree exists (the path tools/gen_golden.py uses, or --reference); the module is loaded at run time with stub
modules for what it imports and this machine lacks (mido: only tick2second; librosa: effects.pitch_shift replaced by a recorder; tqdm,
torchaudio, and the reference's sampler / UI helpers, which Track never touches).  Only data is written:

  <case>.tpb, <case>.n_tracks, and per track <case>.t<k>.
      msgs    (n, 6) int64: type code (0 note_on, 1 note_off, 2 set_tempo, 3 other meta, 4 other), delta time, note, velocity, tempo,
              is_meta — the five preset MIDI files decoded by the small Standard-MIDI-File reader below, and three synthetic lists
      events  (n, 3): note, start tick, duration ticks of Track.events          tempi   Track._get_tempo_at(start) per event
      total   Track._get_total_time()
      calls   (m, 2): event index, n_steps of every librosa.effects.pitch_shift call synthesize_track made (max_notes = 100)
      starts  start_sample per synthesised event (read back from the track a unit impulse note was mixed into)
      audio   (two short synthetic cases) synthesize_track's result when pitch_shift is the float64 restatement of tests/arranger_ref.py
              and the note callback its seeded tone: the reference's own normalise / cache / mix code produced the array
"""
import argparse
import importlib.util
import os
import struct
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import arranger_ref as R  # noqa: E402

NOTE_ON, NOTE_OFF, SET_TEMPO, OTHER_META, OTHER = 0, 1, 2, 3, 4
PRESETS = ("Ode_to_Joy_Easy_variation", "Air_on_the_G_String", "Canon_in_D", "Arhbo", "Rrharil")


def read_smf(path):
    """Standard MIDI File -> (ticks_per_beat, [rows per track]); every message keeps its delta time, as mido's do."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:4] == b"MThd"
    hlen, _fmt, ntrk, div = struct.unpack(">IHHH", data[4:14])
    assert not div & 0x8000, "SMPTE time division"
    pos, tracks = 8 + hlen, []

    def varlen(p):
        v = 0
        while True:
            b = data[p]
            p += 1
            v = (v << 7) | (b & 0x7F)
            if not b & 0x80:
                return v, p

    for _ in range(ntrk):
        assert data[pos:pos + 4] == b"MTrk"
        end = pos + 8 + struct.unpack(">I", data[pos + 4:pos + 8])[0]
        p, rows, status = pos + 8, [], 0
        while p < end:
            dt, p = varlen(p)
            b = data[p]
            if b == 0xFF:
                kind = data[p + 1]
                n, p = varlen(p + 2)
                body = data[p:p + n]
                p += n
                if kind == 0x51:
                    rows.append((SET_TEMPO, dt, 0, 0, int.from_bytes(body, "big"), 1))
                else:
                    rows.append((OTHER_META, dt, 0, 0, 0, 1))
            elif b in (0xF0, 0xF7):
                n, p = varlen(p + 1)
                p += n
                rows.append((OTHER, dt, 0, 0, 0, 0))
            else:
                if b & 0x80:
                    status = b
                    p += 1
                hi = status & 0xF0
                nbytes = 1 if hi in (0xC0, 0xD0) else 2
                args = data[p:p + nbytes]
                p += nbytes
                if hi == 0x90:
                    rows.append((NOTE_ON, dt, args[0], args[1], 0, 0))
                elif hi == 0x80:
                    rows.append((NOTE_OFF, dt, args[0], args[1], 0, 0))
                else:
                    rows.append((OTHER, dt, 0, 0, 0, 0))
        tracks.append(np.array(rows, dtype=np.int64).reshape(-1, 6))
        pos = end
    return div, tracks


def synthetic_cases():
    on, off = (lambda dt, n, v=80: (NOTE_ON, dt, n, v, 0, 0)), (lambda dt, n: (NOTE_ON, dt, n, 0, 0, 0))
    tempo = lambda dt, us: (SET_TEMPO, dt, 0, 0, us, 1)          # noqa: E731
    meta = (OTHER_META, 0, 0, 0, 0, 1)
    # a tempo change mid-track (and a note_off message, which the reference ignores)
    # (as the reference parses it, a set_tempo holds for a note only when it follows that note's note_on at the same tick)
    a = [meta, tempo(0, 400000), on(0, 53), off(240, 53), on(0, 56), tempo(0, 700000), off(240, 56), on(120, 57), (NOTE_OFF, 60, 57, 0, 0, 0),
         off(900, 57), on(0, 50), tempo(0, 300000), off(480, 50), meta]
    # a chord = overlapping notes (the reference closes every one of them against the LAST note_on)
    b = [meta, on(0, 52), on(0, 56), on(0, 59), off(480, 52), off(0, 56), off(0, 59), on(240, 64), off(480, 64), meta]
    # notes below, at and above 52: totals -7, 0, 1, 4, 5, 8, 31 and repeats that share prefixes
    c = [meta]
    for n in (45, 52, 53, 56, 57, 60, 83, 57, 60, 64, 53):
        c += [on(10, n), off(400 if n % 2 else 700, n)]
    return {"syn_tempo": (480, [a]), "syn_chord": (480, [b, a]), "syn_ladder": (480, [c])}


def load_track_maker(ref):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    stub("mido", tick2second=lambda tick, tpb, tempo: tick * tempo * 1e-6 / tpb)
    lib = stub("librosa")
    lib.effects = stub("librosa.effects", pitch_shift=None)
    stub("tqdm", tqdm=lambda it: it)
    ta = stub("torchaudio")
    ta.transforms = stub("torchaudio.transforms")
    stub("gradio")
    stub("model")
    stub("model.DiffSynthSampler", DiffSynthSampler=object)
    stub("webUI")
    stub("webUI.natural_language_guided_4")
    stub("webUI.natural_language_guided_4.utils", encodeBatch2GradioOutput_STFT=None)
    spec = importlib.util.spec_from_file_location("ref_track_maker", os.path.join(ref, "webUI", "natural_language_guided_4", "track_maker.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, lib


def main():
    ap = argparse.ArgumentParser()
    from gen_golden import REF
    ap.add_argument("--reference", default=REF)
    args = ap.parse_args()
    tm, lib = load_track_maker(args.reference)
    cases = {}
    for name in PRESETS:
        cases[name] = read_smf(os.path.join(args.reference, "webUI", "presets", "midis", name + ".mid"))
    cases.update(synthetic_cases())
    out = {"names": np.array(list(cases))}
    for name, (tpb, tracks) in cases.items():
        out[f"{name}.tpb"], out[f"{name}.n_tracks"] = np.int64(tpb), np.int64(len(tracks))
        for k, rows in enumerate(tracks):
            rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
            key = f"{name}.t{k}."
            out[key + "msgs"] = rows
            t = tm.Track(R.messages(rows), tpb, 100)
            out[key + "events"] = np.array([(e.note, e.start_time, e.duration) for e in t.events], dtype=np.int64).reshape(-1, 3)
            out[key + "tempi"] = np.array([t._get_tempo_at(e.start_time) for e in t.events], dtype=np.int64)
            total = t._get_total_time()
            out[key + "total"] = np.float64(total)
            # the call list: which event made which pitch_shift call
            calls, cur = [], [0]

            def counting(it):
                for i, e in enumerate(it):
                    cur[0] = i
                    yield e
            tm.tqdm = counting

            def record(y, sr, n_steps, n_fft, hop_length):
                assert (sr, n_fft, hop_length) == (16000, 4096, 1024)
                calls.append((cur[0], n_steps))
                return y
            lib.effects.pitch_shift = record
            t.synthesize_track(lambda velocity, duration: np.ones(4, dtype=np.float32))
            out[key + "calls"] = np.array(calls, dtype=np.int64).reshape(-1, 2)
            n_calls = len(calls)
            # start_sample per event: one event at a time through the reference's own lines, a unit impulse as the note
            starts, events = [], t.events
            t._get_total_time = lambda total=total: total
            for e in events[:100]:
                t.events = [e]
                starts.append(int(np.argmax(t.synthesize_track(lambda velocity, duration: np.ones(1, dtype=np.float32)))))
            t.events = events
            del t._get_total_time
            out[key + "starts"] = np.array(starts, dtype=np.int64)
            if name in ("syn_tempo", "syn_chord") and k == 0:
                lib.effects.pitch_shift = lambda y, sr, n_steps, n_fft, hop_length: R.pitch_shift(y, n_steps)
                audio = t.synthesize_track(lambda velocity, duration: R.synthetic_note(duration))
                assert audio.dtype == np.float32
                out[key + "audio"] = audio[:int(np.flatnonzero(audio)[-1]) + 1]       # (the tail behind the last note is zeros: total says how long)
            print(f"{name} track {k}: {len(rows)} messages, {len(t.events)} events, {n_calls} pitch_shift calls")
    path = os.path.join(ROOT, "tests", "golden", "arranger.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
