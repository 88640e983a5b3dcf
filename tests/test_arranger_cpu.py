"""CPU suite for the arranger: the float64 restatement of the audio stage (tests/arranger_ref.py) against torch and closed forms, the
package's host logic (Track, the chains, the shared-prefix tree) against what the reference's own Track recorded in golden/arranger.npz,
the C-ABI entries and their argument validation without a device, and the no-fallback error."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import arranger_ref as R
from conftest import ROOT, load_golden
from diffusynth_amd import _lib as L

ENTRIES = ("ds_pv_stft", "ds_pv_vocode", "ds_pv_istft_ws_bytes", "ds_pv_istft", "ds_resample_sinc", "ds_peak_normalize_ws_bytes",
           "ds_peak_normalize", "ds_mix_notes")


def _cases(g):
    for name in g["names"]:
        for k in range(int(g[f"{name}.n_tracks"])):
            yield str(name), k, f"{name}.t{k}."


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_stft_istft_match_torch():
    y = R.probe_signal(30001, seed=3)
    win = torch.hann_window(R.N_FFT, dtype=torch.float64)
    want = torch.stft(torch.from_numpy(y).double(), R.N_FFT, R.HOP, window=win, center=True, pad_mode="constant", return_complex=True).numpy().T
    D = R.stft(y)
    assert D.shape == (1 + len(y) // R.HOP, R.N_FFT // 2 + 1)
    assert np.abs(D - want).max() / np.abs(want).max() < 1e-13
    back = R.istft(D, len(y))
    assert np.abs(back - y).max() < 1e-13                                      # STFT -> iSTFT round trip
    ti = torch.istft(torch.from_numpy(np.ascontiguousarray(want.T)), R.N_FFT, R.HOP, window=win, center=True, length=len(y)).numpy()
    assert np.abs(back - ti).max() < 1e-13
    assert np.array_equal(R.istft(D, len(y) + 5000)[len(y) + 3000:], np.zeros(2000))     # behind the last frame: zeros, not a division by zero


@pytest.mark.parametrize("rate", [2 ** (-1 / 12), 2 ** (-4 / 12), 2 ** (4 / 12)])
def test_restatement_resampler_reproduces_a_sinusoid(rate):
    """A sinusoid at 0.8 of the pass band comes out as its closed form (measured: 1.4e-6 at worst), away from the two ends, where the kernel
    reaches outside the signal and the closed form does not apply."""
    fc = R.RS_FC * min(1.0, rate)
    f, n = 0.8 * fc * 0.5, 8000
    x = np.sin(2 * np.pi * f * np.arange(n) + 0.3)
    m = int(n * rate)
    got = R.resample(x, rate, m)
    want = np.sin(2 * np.pi * f * np.arange(m) / rate + 0.3)
    edge = int(np.ceil(R.RS_Z / fc * rate)) + 2
    err = np.abs(got - want)[edge:-edge].max()
    print(f"rate {rate:.4f}: {err:.2e}")
    assert err < 1e-5


def test_restatement_phasor_form_equals_angle_form():
    y = R.probe_signal(28416, seed=1)
    for n_steps in (4, 1, -3):
        a, b = R.pitch_shift(y, n_steps), R.pitch_shift(y, n_steps, form="angle")
        assert np.abs(a - b).max() / np.abs(b).max() < 1e-10
    D = R.stft(y)
    D[2, 100:200] = 0                                                          # zero bins: np.angle(0) = 0 <-> unit phasor 1
    a, b = R.phase_vocoder(D, R.rate_of(4)), R.phase_vocoder(D, R.rate_of(4), form="angle")
    assert np.abs(a - b).max() / np.abs(b).max() < 1e-10


@pytest.mark.parametrize("total", [4, 7, 12, 32])
def test_restatement_shifts_the_pitch(total):
    f0, sr, n = 164.8, 16000, 16384
    t = np.arange(28416) / sr
    y = sum(np.sin(2 * np.pi * f0 * (h + 1) * t + h) / (h + 1) ** 2 for h in range(8)) * np.exp(-1.5 * t)       # the fundamental is the strongest partial
    z = R.pitch_shift_chain(y, total)
    peak = np.argmax(np.abs(np.fft.rfft(z[:n] * np.hanning(n)))) * sr / n
    print(f"total {total}: {peak:.1f} Hz for {f0 * 2 ** (total / 12):.1f} Hz")
    assert abs(peak - f0 * 2 ** (total / 12)) <= sr / R.N_FFT                   # one analysis bin


def test_chain_does_nothing_at_or_below_zero():
    y = R.probe_signal(5000)
    assert R.pitch_shift_chain(y, 0) is y and R.pitch_shift_chain(y, -7) is y
    assert R.chain_steps(31) == [4] * 7 + [3] and R.chain_steps(5) == [4, 1] and R.chain_steps(0) == [] and R.chain_steps(-3) == []
    from diffusynth_amd import arranger as A
    for t in range(-8, 40):
        assert A.chain_steps(t) == R.chain_steps(t)


# ---------------------------------------------------------------------------------------------------- host logic against the reference's Track
def test_fixture_holds_the_presets_and_the_synthetic_lists():
    g = load_golden("arranger")
    names = [str(n) for n in g["names"]]
    assert names[:5] == ["Ode_to_Joy_Easy_variation", "Air_on_the_G_String", "Canon_in_D", "Arhbo", "Rrharil"] and len(names) == 8
    assert int(g["Ode_to_Joy_Easy_variation.n_tracks"]) == 2
    lad = g["syn_ladder.t0.calls"]
    totals = [int(lad[lad[:, 0] == i, 1].sum()) for i in range(len(g["syn_ladder.t0.events"]))]
    assert {0, 1, 4, 5, 8, 31} <= set(totals)
    assert len(set(g["syn_tempo.t0.tempi"].tolist())) > 1                       # a tempo change mid-track
    ch = g["syn_chord.t0.events"]
    assert (ch[:3, 1] == ch[0, 1]).all()                                        # a chord


def test_track_matches_the_reference_track():
    from diffusynth_amd import arranger as A
    g = load_golden("arranger")
    for name, k, key in _cases(g):
        t = A.Track(R.messages(g[key + "msgs"]), int(g[name + ".tpb"]), 100)
        ev = np.array([(e.note, e.start_time, e.duration) for e in t.events], dtype=np.int64).reshape(-1, 3)
        assert np.array_equal(ev, g[key + "events"]), key
        assert [t._get_tempo_at(e.start_time) for e in t.events] == g[key + "tempi"].tolist(), key
        assert t._get_total_time() == float(g[key + "total"]), key
        sched = t.schedule()
        assert [s[2] for s in sched] == g[key + "starts"].tolist(), key
        calls = [(i, s) for i, (_, _, _, total) in enumerate(sched) for s in A.chain_steps(total)]
        assert calls == [tuple(c) for c in g[key + "calls"].tolist()], key
        r = R.Track(R.messages(g[key + "msgs"]), int(g[name + ".tpb"]), 100)     # the restatement's Track says the same
        assert [(e.note, e.start_time, e.duration) for e in r.events] == [tuple(x) for x in ev.tolist()] and r._get_total_time() == t._get_total_time()


@pytest.mark.parametrize("case", ["syn_tempo", "syn_chord"])
def test_restatement_mix_equals_the_reference_track_audio(case):
    g = load_golden("arranger")
    t = R.Track(R.messages(g[case + ".t0.msgs"]), int(g[case + ".tpb"]), 100)
    got = t.synthesize_track(lambda velocity, duration: R.synthetic_note(duration))
    want = g[case + ".t0.audio"]
    assert got.dtype == np.float32 and len(got) == int(float(g[case + ".t0.total"]) * 16000)
    assert np.array_equal(got[:len(want)], want) and not got[len(want):].any()


def test_tree_expands_to_the_reference_call_list():
    from diffusynth_amd import arranger as A
    g = load_golden("arranger")
    counts = {}
    for name, k, key in _cases(g):
        t = A.Track(R.messages(g[key + "msgs"]), int(g[name + ".tpb"]), 100)
        sched = t.schedule()
        levels = A.shift_tree([(s[0], s[3]) for s in sched])
        nodes = {(kk, cum): (lo, st) for lv in levels for kk, lo, cum, st in lv}
        assert sum(len(lv) for lv in levels) == len(nodes)                      # every (key, cumulative) once
        calls = g[key + "calls"]
        distinct = set()
        for i, (dkey, _, _, total) in enumerate(sched):
            path, cum = [], max(total, 0)
            while cum > 0:                                                      # walk from the event's node back to its source
                lo, st = nodes[(dkey, cum)]
                path.append(st)
                cum = lo
            want = calls[calls[:, 0] == i, 1].tolist()
            assert path[::-1] == want, (key, i)
            distinct |= {(dkey, c) for c in np.cumsum(want).tolist()}
        assert len(nodes) == len(distinct), key
        counts[(name, k)] = len(nodes)
    assert [counts[(n, 0)] + counts[(n, 1)] for n in ("Ode_to_Joy_Easy_variation", "Air_on_the_G_String", "Canon_in_D", "Arhbo", "Rrharil")] == [39, 51, 39, 50, 26]


def test_mix_lists_cover_every_event_in_order():
    from diffusynth_amd import arranger as A
    starts, lengths, n = [0, 1000, 1023, 1024, 5000, 5000, 9000], [10, 100, 1, 3000, 4000, 1, 1240], 10240
    ptr, lst = A.mix_lists(starts, lengths, n)
    assert len(ptr) == n // L.MIX_BLOCK + 1
    for b in range(len(ptr) - 1):
        want = [e for e, (s, m) in enumerate(zip(starts, lengths)) if s < (b + 1) * L.MIX_BLOCK and s + m > b * L.MIX_BLOCK]
        assert lst[ptr[b]:ptr[b + 1]].tolist() == want


# ---------------------------------------------------------------------------------------------------- C ABI without a device
def test_header_and_binding_declare_the_entries():
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", text))
    lib = L.load()
    for name in ENTRIES:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.ds_pv_istft_ws_bytes(10) == 10 * 4096 * 4 and lib.ds_pv_istft_ws_bytes(0) == 0
    assert lib.ds_peak_normalize_ws_bytes(3, 77568) == 3 * 19 * 4 and lib.ds_peak_normalize_ws_bytes(2, 10 ** 6) == 2 * 64 * 4
    assert L.PV["DS_PV_NI"] == 9 and L.MIX_BLOCK == 1024


def test_entries_validate_before_any_gpu_work():
    """Callable on a machine without a device: bad arguments answer DS_EINVAL (-1) or DS_EALIGN (-3) and the message names the entry."""
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    calls = {
        "pv_stft": [lambda: lib.ds_pv_stft(p, p, 0, 4, 100, 4, p, None), lambda: lib.ds_pv_stft(None, p, 1, 4, 100, 4, p, None),
                    lambda: lib.ds_pv_stft(p, p, 1, 0, 100, 4, p, None), lambda: lib.ds_pv_stft(p, p, 1, 4, 1 << 31, 4, p, None)],
        "pv_vocode": [lambda: lib.ds_pv_vocode(p, p, p, p, 0, 4, 4, p, None), lambda: lib.ds_pv_vocode(p, p, None, p, 1, 4, 4, p, None),
                      lambda: lib.ds_pv_vocode(p, p, p, p, 1, 4, 0, p, None)],
        "pv_istft": [lambda: lib.ds_pv_istft(p, p, 1, 0, 10, 4, 10, p, p, None), lambda: lib.ds_pv_istft(p, p, 1, 4, 10, 4, 10, None, p, None),
                     lambda: lib.ds_pv_istft(p, p, 1, 4, 10, 1 << 20, 10, p, p, None)],
        "resample_sinc": [lambda: lib.ds_resample_sinc(p, p, None, 1, 10, 10, 10, p, None), lambda: lib.ds_resample_sinc(p, p, p, 1, 0, 10, 10, p, None)],
        "peak_normalize": [lambda: lib.ds_peak_normalize(p, p, 0, 10, 10, p, p, None), lambda: lib.ds_peak_normalize(p, p, 1, 10, 10, None, p, None)],
        "mix_notes": [lambda: lib.ds_mix_notes(p, 10, p, 0, p, p, 0, p, 10, None), lambda: lib.ds_mix_notes(p, 10, p, 1, p, p, 0, p, 0, None),
                      lambda: lib.ds_mix_notes(p, 10, p, 1, p, p, -1, p, 10, None)],
    }
    for name, fns in calls.items():
        for fn in fns:
            assert fn() == -1, name
            assert name.encode() in lib.ds_last_error_string(), (name, lib.ds_last_error_string())
    assert lib.ds_resample_sinc(p, p, p + 4, 1, 10, 10, 10, p, None) == -3 and b"resample_sinc" in lib.ds_last_error_string()
    assert lib.ds_pv_vocode(p + 4, p, p, p, 1, 4, 4, p, None) == -3 and b"pv_vocode" in lib.ds_last_error_string()
    with pytest.raises(L.DsError, match="mix_notes"):
        L.call("ds_mix_notes", p, 10, p, 0, p, p, 0, p, 10, None)


def test_arranger_fails_loudly_without_gpu(monkeypatch):
    from diffusynth_amd import arranger as A
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.pitch_shift(torch.zeros(1, 5000), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.pitch_shift_chain([torch.zeros(5000)], [5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.pitch_shift_librosa(torch.zeros(5000), 16000, 5)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    g = load_golden("arranger")
    t = A.Track(R.messages(g["syn_chord.t0.msgs"]), 480)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.synthesize_track(lambda velocity, duration: R.synthetic_note(duration))
