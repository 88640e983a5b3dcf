"""CPU suite for the pitch detector and the arranger's tuned mode: the float64 restatement of YIN (tests/pitch_ref.py) against closed
form, the unpitched cases, the signed chains and their tree, the tune= validation and defaults, the C-ABI entries without a device, and
the end-to-end check in float64 (detect, shift by signed chains of the arranger's restatement, detect again).

Accuracy of the restatement's median on the test tones (30 001 samples, noise 0.01, strong | weak fundamental), in cents, every frame
voiced; the assertions hold twice the larger figure:
    65.41 Hz 0.035 | 0.023    110 Hz 0.042 | 0.028    164.81 Hz 0.118 | 0.104    155 Hz 0.104 | 0.091    440 Hz 0.663 | 0.620
    830.6 Hz 3.62 | 3.30      (988 Hz: 5.3 | 4.8, not asserted)
The growth with frequency is the method's: a parabola through three points of a dip that is 16 samples per period wide at 1 kHz."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import arranger_ref as R
import pitch_ref as P
from conftest import ROOT
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

CENTS = {65.41: 0.07, 110.0: 0.085, 164.81: 0.24, 155.0: 0.21, 440.0: 1.33, 830.6: 7.3}     # 2 x the measured figure (docstring)


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("amps", [P.STRONG, P.WEAK], ids=["strong", "weak"])
@pytest.mark.parametrize("i,f0", list(enumerate(P.TONE_F0)))
def test_restatement_finds_the_tone(i, f0, amps):
    x = P.tone(f0, 30001, seed=i, amps=amps)
    period, aper, picks = P.yin(x)
    got, midi, voiced, frames = P.estimate(x)
    err = 1200.0 * np.log2(got / f0)
    print(f"{f0} Hz: {got:.4f} Hz, {err:+.4f} cents (bound {CENTS[f0]}), {voiced} of {frames} voiced")
    assert frames == P.frame_count(30001, P.W, 290, P.HOP) == 113 and voiced == frames        # no octave error on any frame, either
    assert abs(err) <= CENTS[f0]
    assert abs(midi - (69 + 12 * np.log2(f0 / 440))) * 100 <= CENTS[f0]
    assert np.all(np.abs(period - P.SR / f0) < 1.0) and np.all(aper < P.THRESHOLD) and np.all(picks == np.floor(period + 0.5))


def test_twin_decides_as_the_restatement_does():
    x = P.tone(164.81, 8000, seed=2)
    p64, a64, k64 = P.yin(x)
    p32, a32, k32 = P.yin(x, dtype=np.float32)
    assert p32.dtype == a32.dtype == np.float32 and np.array_equal(k32, k64) and not P.fragile(x).any()
    assert np.abs(p32 - p64).max() / p64.max() < 1e-6 and np.abs(a32 - a64).max() / a64.max() < 1e-5


@pytest.mark.parametrize("name,x,frames", [
    ("white noise", P.white_noise(28416, 3), 106),
    ("silence", np.zeros(4097, np.float32), 11),
    ("a tone under noise 0.3", P.tone(164.81, 30001, seed=5, noise=0.3), 113),
    ("shorter than one frame", P.tone(110.0, P.W + 290 - 1, seed=1), 0)], ids=["noise", "silence", "noisy_tone", "short"])
def test_unpitched(name, x, frames):
    for dtype in (np.float64, np.float32):
        period, aper, picks = P.yin(x, dtype=dtype)
        assert len(period) == frames and not np.isnan(period).any() and not np.isnan(aper).any(), name
        assert not period.any() and np.all(aper == 1) and not picks.any(), name
        assert not np.isnan(P.cmnd(x, dtype=dtype)).any(), name
        f0, midi, voiced, n = P.estimate(x, dtype=dtype)
        assert np.isnan(f0) and np.isnan(midi) and voiced == 0 and n == frames, name


def test_min_voiced_and_lower_median():
    assert P.lower_median(np.array([0, 5.0, 3.0, 0, 9.0, 7.0])) == (5.0, 4)      # rank (4 - 1) // 2 = 1 of 3 5 7 9
    assert P.lower_median(np.array([4.0, 0, 2.0, 8.0])) == (4.0, 3) and P.lower_median(np.zeros(3)) == (0.0, 0)
    x = np.concatenate([P.tone(220.0, 6000, seed=1), P.white_noise(24000, 1)])
    f0, midi, voiced, frames = P.estimate(x)
    assert 0 < voiced < 0.25 * frames and np.isnan(midi)
    assert abs(P.estimate(x, min_voiced=0.05)[0] - 220.0) < 0.5


# ---------------------------------------------------------------------------------------------------- signed chains, the signed tree
def test_signed_chain():
    for t in range(1, 40):
        assert A.signed_chain(t) == A.chain_steps(t) and all(isinstance(s, int) for s in A.signed_chain(t))
        assert A.signed_chain(-t) == [-s for s in A.chain_steps(t)]
    assert A.signed_chain(0) == [] and A.signed_chain(0.049) == [] and A.signed_chain(-0.049) == [] and A.signed_chain(float("nan")) == []
    assert A.signed_chain(0.05) == [0.05] and A.signed_chain(-0.3) == [-0.3]
    c = A.signed_chain(9.37)
    assert c[:2] == [4, 4] and c[2] == 9.37 - 8 and len(c) == 3                    # the real remainder comes last
    c = A.signed_chain(-10.37)
    assert c[:2] == [-4, -4] and c[2] == -10.37 + 8 and len(c) == 3
    assert A.signed_chain(7.5, step_size=3) == [3, 3, 1.5] and A.signed_chain(0.3, deadband=0.5) == []


def test_signed_tree_shares_prefixes_and_nothing_across_signs():
    reqs = [("a", 5.03), ("a", 9.03), ("a", -9.37), ("a", -3.37), ("b", 4), ("a", 0.01), ("a", 9.03), ("b", -4.0), ("a", 8)]
    levels = A.signed_tree(reqs)
    nodes = [(k, cum) for lv in levels for k, _, cum, _ in lv]
    assert len(nodes) == len(set(nodes))                                          # every (key, cumulative) once
    assert nodes.count(("a", 4)) == 1 and ("a", 4, 5.03, 5.03 - 4) in levels[1] and ("a", 4, 8, 4) in levels[1] and ("a", 8, 9.03, 9.03 - 8) in levels[2]
    assert ("a", 0.01) not in nodes                                               # the deadband: no node, the source itself
    by = {(k, cum): (lo, st) for lv in levels for k, lo, cum, st in lv}
    for k, t in reqs:                                                             # every request's path is its signed_chain
        path, cum = [], t if A.signed_chain(t) else 0
        while cum != 0:
            lo, st = by[(k, cum)]
            assert lo == 0 or (lo > 0) == (cum > 0)                               # a chain never changes sign: only the root is shared
            path.append(st)
            cum = lo
        assert path[::-1] == A.signed_chain(t), (k, t)
    assert {(k, lo) for lv in levels[:1] for k, lo, _, _ in lv} == {("a", 0), ("b", 0)}
    pos = [(k, t) for k, t in reqs if isinstance(t, int) and t > 0]
    assert A.signed_tree(pos) == A.shift_tree(pos)                                # positive integers: the existing tree, node for node


# ---------------------------------------------------------------------------------------------------- tune=
def _track(events=((57, 960), (40, 1440), (64, 960))):
    return A.Track(P.note_messages(events), P.TPB)


@pytest.mark.parametrize("bad", ["Detect", "", True, float("nan"), float("inf"), [52], (52,), "52", object()])
def test_tune_is_validated_before_anything_else(bad, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    called = []
    with pytest.raises(ValueError, match="^tune: "):
        _track().render(lambda v, d: called.append(d), tune=bad)
    assert not called
    with pytest.raises(ValueError, match="^tune: "):
        A.DiffSynth({}, None, None, None, None, None, "cuda", tune=bad)
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda")
    with pytest.raises(ValueError, match="^tune: "):
        ds.arrange([_track()], ["x"], {}, tune=bad)


@pytest.mark.parametrize("good", [None, "detect", 52, 50.37, np.float32(48.5), np.int64(60)])
def test_a_valid_tune_reaches_the_no_fallback_error(good, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _track().render(lambda v, d: np.ones(100, np.float32), tune=good)
    assert A.DiffSynth({}, None, None, None, None, None, "cuda", tune=good).tune == (good if good is None or good == "detect" else float(good))


def test_tune_none_is_the_default_and_leaves_schedule_and_requests_alone(monkeypatch):
    for fn in (A.Track.render, A.DiffSynth.__init__):
        p = inspect.signature(fn).parameters["tune"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(A.pitch_shift_chain).parameters["signed"].default is False
    t = _track(((57, 960), (40, 1440), (64, 960), (52, 960), (53, 1440)))
    sched = t.schedule()
    spt = 500000 * 1e-6 / P.TPB
    assert sched == [(str(d * spt), d * spt, int(s * spt * 16000), n - 52)
                     for n, d, s in ((57, 960, 240), (40, 1440, 1440), (64, 960, 3120), (52, 960, 4320), (53, 1440, 5520))]
    seen = {}
    monkeypatch.setattr(A, "_run_tree", lambda sources, requests, step_size=4: seen.setdefault("req", list(requests)) and {})
    monkeypatch.setattr(A, "_run_levels", lambda *a: pytest.fail("tune=None must not build a signed tree"))
    monkeypatch.setattr(A, "_mix_nodes", lambda have, placed, n: seen.setdefault("placed", placed))
    t._mix_reference(sched, t.track_length(), {})
    assert seen["req"] == [(k, tot) for k, _, _, tot in sched if tot > 0] == [(sched[0][0], 5), (sched[2][0], 12), (sched[4][0], 1)]
    assert seen["placed"] == [((k, max(tot, 0)), s) for k, _, s, tot in sched] and t.last_pitches is None


def test_tuned_plans_on_the_host(monkeypatch):
    """_mix_tuned with stated pitches: signed totals per event, the reference's rule for an unpitched note, the deadband."""
    t = _track(((57, 960), (40, 1440), (64, 960), (52, 960), (50, 1440)))
    sched = t.schedule()
    k1, k2 = sched[0][0], sched[1][0]
    seen = {}
    monkeypatch.setattr(A, "_run_levels", lambda sources, levels: seen.setdefault("levels", levels) and {})
    monkeypatch.setattr(A, "_mix_nodes", lambda have, placed, n: seen.setdefault("placed", placed))
    t._mix_tuned(sched, t.track_length(), {k1: None, k2: None}, {k1: 52.03, k2: float("nan")})
    assert t.last_pitches[k1] == 52.03 and np.isnan(t.last_pitches[k2])
    assert [node for node, _ in seen["placed"]] == [(k1, 57 - 52.03), (k2, 0), (k1, 64 - 52.03), (k1, 0), (k2, 0)]   # 52 - 52.03: the deadband
    assert seen["levels"] == A.signed_tree([(k1, 57 - 52.03), (k1, 64 - 52.03)])


# ---------------------------------------------------------------------------------------------------- the package without a device
def test_pitch_fails_loudly_without_gpu_and_validates_first():
    import diffusynth_amd
    from diffusynth_amd import pitch
    assert diffusynth_amd.yin is pitch.yin and diffusynth_amd.estimate_pitch is pitch.estimate_pitch
    x = torch.zeros(2, 5000)
    for fn in (pitch.yin, pitch.estimate_pitch):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn([x[0], x[1, :3000]])
        for kw, name in (({"fmin": 10.0}, "fmin"), ({"fmin": 0}, "fmin"), ({"fmax": 50.0}, "fmax"), ({"fmax": 0}, "fmax"),
                         ({"frame_length": 2049}, "frame_length"), ({"frame_length": 0}, "frame_length"), ({"frame_length": 512.0}, "frame_length"),
                         ({"threshold": 0.0}, "threshold"), ({"threshold": 1.0}, "threshold"), ({"threshold": -0.1}, "threshold"),
                         ({"hop_length": 0}, "hop_length")):
            with pytest.raises(ValueError, match="^" + name):                   # the arguments come first: nothing has touched a device
                fn(x, **kw)
    assert pitch._taus(16000, 55.0, 1000.0, 1024, 256, 0.1) == (1024, 256, 16, 290) == (P.W, P.HOP) + P.taus()
    assert pitch._taus(16000, 15.625, 8000.0, 2048, 1, 0.5) == (2048, 1, 2, 1024)
    assert [pitch.frame_count(n, 1024, 290, 256) for n in (1313, 1314, 1569, 1570)] == [0, 1, 1, 2]


def test_header_and_binding_declare_the_entries():
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", text))
    lib = L.load()
    for name in ("ds_yin_frames", "ds_pitch_median"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert L.YIN == {"DS_YIN_XOFF": 0, "DS_YIN_LEN": 1, "DS_YIN_FOFF": 2, "DS_YIN_NF": 3, "DS_YIN_NI": 4, "DS_YIN_MAX_W": 2048, "DS_YIN_MAX_TAU": 1024}
    assert L.PITCH_MAX_FRAMES == 8192 and lib.ds_abi_version() == 1


def test_entries_validate_before_any_gpu_work():
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    yin = lambda **kw: lib.ds_yin_frames(*[kw.get(k, v) for k, v in (("x", p), ("tab", p), ("n", 1), ("mf", 4), ("ts", 5000), ("tf", 4), ("W", 1024), ("hop", 256),       # noqa: E731
                                                                       ("tmin", 16), ("tmax", 290), ("thr", 0.1), ("per", p), ("ap", p), ("st", None))])
    for kw in ({"x": None}, {"per": None}, {"n": 0}, {"mf": 0}, {"tf": 0}, {"ts": 0}, {"W": 2049}, {"W": 0}, {"hop": 0}, {"tmin": 1}, {"tmin": 290},
               {"tmax": 1025}, {"thr": 0.0}, {"thr": 1.0}, {"n": 65536}, {"ts": 1 << 31}):
        assert yin(**kw) == -1, kw
        assert b"yin_frames" in lib.ds_last_error_string(), kw
    assert yin(x=p + 2) == -3 and b"yin_frames" in lib.ds_last_error_string()
    med = lambda **kw: lib.ds_pitch_median(*[kw.get(k, v) for k, v in (("per", p), ("tab", p), ("n", 1), ("mf", 4), ("tf", 4), ("med", p), ("nv", p), ("st", None))])   # noqa: E731
    for kw in ({"per": None}, {"nv": None}, {"n": 0}, {"mf": 0}, {"tf": 0}, {"mf": 8193}):
        assert med(**kw) == -1, kw
        assert b"pitch_median" in lib.ds_last_error_string(), kw
    assert b"8192" in lib.ds_last_error_string()                                  # the frame limit says what it is
    assert med(med=p + 1) == -3
    with pytest.raises(L.DsError, match="pitch_median"):
        L.call("ds_pitch_median", p, p, 1, 8193, 4, p, p, None)


# ---------------------------------------------------------------------------------------------------- end to end, float64
def test_detected_and_shifted_notes_land_in_tune():
    """The probe tone at 150 Hz (MIDI 50.37): detect, shift by the signed chains of the arranger's restatement, detect again.  1 cent is
    the musical condition (a fifth of the smallest audible mistuning); measured: 0.064 cent at worst."""
    x = R.probe_signal(28416, seed=0, f0=150.0).astype(np.float64)
    x /= np.abs(x).max()
    f0, p, voiced, frames = P.estimate(x)
    assert voiced == frames == 106 and abs(p - (69 + 12 * np.log2(150.0 / 440))) < 0.001
    for note in (40, 47, 52, 57, 64):
        chain = A.signed_chain(note - p)
        assert all(abs(s) <= 4 for s in chain) and abs(sum(chain) - (note - p)) < 1e-12
        cur = x
        for s in chain:
            cur = R.pitch_shift(cur, s)
        _, midi, v, n = P.estimate(cur)
        print(f"note {note}: chain {chain} -> {midi:.5f} ({100 * (midi - note):+.4f} cents), {v} of {n} voiced")
        assert abs(midi - note) * 100 <= 1.0
