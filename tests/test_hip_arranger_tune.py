"""The arranger's tuned mode on the GPU: Track.render(tune=) and DiffSynth(tune=) bit for bit against the public pieces they are made of
(peak_normalize, pitch.estimate_pitch, pitch_shift_chain(signed=True), mix_notes), the musical condition (every shifted note within
1 cent of its MIDI note — a fifth of the smallest audible mistuning; the float64 form of this check is tests/test_pitch_cpu.py's last
test, the device adds the fp32 chain's error, which tests/test_hip_arranger.py bounds), the defaults (tune=None and tune omitted: the
reference's rule, today's bits) and the signed chains against the arranger's restatement by test_hip_arranger.py's tolerance rule.

The source is the project's probe tone at 150 Hz (MIDI 50.37: off every note, so every event needs a real, signed shift)."""
import functools

import numpy as np
import pytest
import torch

import arranger_ref as R
import pitch_ref as P
from diffusynth_amd import arranger as A
from diffusynth_amd import pitch
from test_hip_arranger import check
from test_hip_pitch import CopyCounter

pytestmark = pytest.mark.gpu

EVENTS = ((40, 960), (47, 1440), (52, 960), (52, 1440), (57, 960), (64, 1440), (45, 960), (60, 960))      # (note, ticks): two durations


def probe(n, seed):
    return torch.from_numpy(R.probe_signal(n, seed=seed, f0=150.0)).cuda()


def track(events=EVENTS):
    return A.Track(P.note_messages(events), P.TPB)


def given(t, sigs):
    """{duration key: signal} for the track's distinct durations, in event order."""
    keys = list(dict.fromkeys(s[0] for s in t.schedule()))
    assert len(keys) == len(sigs)
    return dict(zip(keys, sigs))


@functools.lru_cache(maxsize=None)
def by_hand():
    """The eight-event track from its public pieces: (track, notes, estimate, per-event shifted notes, the mixed track)."""
    t = track()
    notes = given(t, [0.6 * probe(28416, 0), 0.8 * probe(20000, 1)])
    keys = list(notes)
    normed = dict(zip(keys, A.peak_normalize([notes[k] for k in keys])))
    est = pitch.estimate_pitch([normed[k] for k in keys])
    midi = dict(zip(keys, est.midi.tolist()))
    sched = t.schedule()
    totals = [e.note - midi[key] for (key, _, _, _), e in zip(sched, t.events)]
    shifted = A.pitch_shift_chain([normed[key] for key, _, _, _ in sched], totals, signed=True)
    mixed = A.mix_notes(shifted, [(start, i) for i, (_, _, start, _) in enumerate(sched)], t.track_length())
    return t, notes, midi, shifted, mixed


# ---------------------------------------------------------------------------------------------------- tune="detect"
def test_detect_is_its_public_pieces_bit_for_bit(monkeypatch):
    t, notes, midi, shifted, mixed = by_hand()
    assert all(abs(m - (69 + 12 * np.log2(150.0 / 440))) < 0.01 for m in midi.values())       # MIDI 50.37
    base = CopyCounter(monkeypatch)
    plain = t.render(None, notes=notes)
    n_plain = base.count
    got = t.render(None, notes=notes, tune="detect")
    assert base.count - n_plain == n_plain + 1                                    # exactly one device -> host copy more than tune=None
    monkeypatch.undo()
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == mixed.shape and torch.equal(got, mixed)
    assert t.last_pitches == midi
    assert not torch.equal(got, plain)
    host = t.render(None, notes=notes, tune="detect", return_tensor=False)
    assert isinstance(host, np.ndarray) and np.array_equal(host, mixed.cpu().numpy())
    fn = t.render(lambda v, d: notes[str(d)].cpu().numpy(), tune="detect")       # through the callback, from the host
    assert torch.equal(fn, mixed)


def test_detected_and_shifted_notes_are_in_tune():
    t, notes, midi, shifted, mixed = by_hand()
    est = pitch.estimate_pitch(shifted)
    for e, m, v, n in zip(t.events, est.midi, est.voiced, est.frames):
        print(f"note {e.note}: {m:.5f} ({100 * (m - e.note):+.4f} cents), {v} of {n} frames voiced")
        assert abs(m - e.note) * 100 <= 1.0


def test_an_unpitched_source_follows_the_reference_rule():
    t = track()
    noise = torch.from_numpy(P.white_noise(28416, 9)).cuda()
    notes = given(t, [noise, torch.from_numpy(P.white_noise(20000, 10)).cuda()])
    got = t.render(None, notes=notes, tune="detect")
    assert all(np.isnan(p) for p in t.last_pitches.values()) and len(t.last_pitches) == 2
    assert torch.equal(got, t.render(None, notes=notes))
    # one noise note beside a tone: the tone's events are tuned, the noise's are mixed as tune=None mixes them
    mixed_notes = given(t, [0.6 * probe(28416, 0), noise[:20000].clone()])
    k_tone, k_noise = list(mixed_notes)
    got = t.render(None, notes=mixed_notes, tune="detect")
    assert np.isnan(t.last_pitches[k_noise]) and abs(t.last_pitches[k_tone] - 50.37) < 0.01
    sched = t.schedule()
    normed = dict(zip([k_tone, k_noise], A.peak_normalize([mixed_notes[k_tone], mixed_notes[k_noise]])))
    parts, idx = [], []
    for (key, _, start, total), e in zip(sched, t.events):
        tot = max(total, 0) if key == k_noise else e.note - t.last_pitches[k_tone]
        parts.append(A.pitch_shift_chain([normed[key]], [tot], signed=True)[0])
        idx.append((start, len(idx)))
    assert torch.equal(got, A.mix_notes(parts, idx, t.track_length()))


# ---------------------------------------------------------------------------------------------------- tune=<number>, tune=None
def test_tune_52_is_the_reference_rule_without_its_bug():
    up = track(((52, 960), (57, 1440), (64, 960), (53, 960), (52, 1440), (76, 960)))
    notes = given(up, [0.6 * probe(28416, 0), 0.8 * probe(20000, 1)])
    assert torch.equal(up.render(None, notes=notes, tune=52), up.render(None, notes=notes))      # nothing below 52: the same bits
    assert up.last_pitches == {k: 52.0 for k in notes}
    t = track()
    notes = given(t, [0.6 * probe(28416, 0), 0.8 * probe(20000, 1)])
    plain, tuned = t.render(None, notes=notes), t.render(None, notes=notes, tune=52.0)
    covered = torch.zeros(plain.numel(), dtype=torch.bool, device="cuda")
    low = [(start, notes[key].numel()) for (key, _, start, _), e in zip(t.schedule(), t.events) if e.note < 52]
    assert len(low) == 3                                                          # 40, 47, 45
    for start, n in low:
        covered[start:start + n] = True
        assert not torch.equal(plain[start:start + n], tuned[start:start + n])
    assert torch.equal(plain[~covered], tuned[~covered]) and 0 < int(covered.sum()) < plain.numel()
    assert (plain[covered] != tuned[covered]).float().mean() > 0.99               # the shifted notes are other signals, sample for sample


def test_tune_none_and_omitted_are_todays_render():
    t = track()
    notes = given(t, [0.6 * probe(28416, 0), 0.8 * probe(20000, 1)])
    a, b = t.render(None, notes=notes), t.render(None, notes=notes, tune=None)
    assert torch.equal(a, b) and t.last_pitches is None
    # today's render, from its pieces: the reference's rule through the unsigned chains
    keys = list(notes)
    normed = dict(zip(keys, A.peak_normalize([notes[k] for k in keys])))
    sched = t.schedule()
    shifted = A.pitch_shift_chain([normed[key] for key, _, _, _ in sched], [total for _, _, _, total in sched])
    assert torch.equal(a, A.mix_notes(shifted, [(start, i) for i, (_, _, start, _) in enumerate(sched)], t.track_length()))


# ---------------------------------------------------------------------------------------------------- DiffSynth.arrange
def test_arrange_detects_every_distinct_note_once(monkeypatch):
    tracks = [track(), track(((50, 1440), (62, 960), (38, 1440), (55, 480)))]
    names = ["lead", "bass"]
    sigs = {"lead": [0.6 * probe(28416, 0), 0.8 * probe(20000, 1)], "bass": [0.5 * probe(30001, 2), 0.9 * probe(28416, 3), torch.from_numpy(P.white_noise(12000, 4)).cuda()]}
    notes = {}
    for name, t in zip(names, tracks):
        durs = list(dict.fromkeys(s[1] for s in t.schedule()))
        notes.update({(name, d): s for d, s in zip(durs, sigs[name])})
    assert len(notes) == 5
    want_tracks = [t.render(None, notes={s[0]: notes[(name, s[1])] for s in t.schedule()}, tune="detect") for name, t in zip(names, tracks)]
    want_pitches = {(name, s[1]): t.last_pitches[s[0]] for name, t in zip(names, tracks) for s in t.schedule()}
    want = torch.zeros(max(a.numel() for a in want_tracks), device="cuda")
    for a in want_tracks:
        want[:a.numel()] += a
    calls = []
    real = pitch.estimate_pitch
    monkeypatch.setattr(pitch, "estimate_pitch", lambda *a, **kw: calls.append(len(a[0])) or real(*a, **kw))
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda", tune="detect")
    got = ds.arrange(tracks, names, notes)
    assert calls == [5]                                                           # one call, every distinct (instrument, duration) note once
    assert torch.equal(got, want)
    assert set(ds.last_pitches) == set(notes) and all(ds.last_pitches[k] == v or (np.isnan(v) and np.isnan(ds.last_pitches[k])) for k, v in want_pitches.items())
    assert np.isnan(ds.last_pitches[("bass", list(dict.fromkeys(s[1] for s in tracks[1].schedule()))[2])])
    # the keyword of arrange wins over the constructor's; None is the reference's rule
    plain = A.DiffSynth({}, None, None, None, None, None, "cuda").arrange(tracks, names, notes)
    assert torch.equal(ds.arrange(tracks, names, notes, tune=None), plain) and not torch.equal(plain, got)
    assert calls == [5]


# ---------------------------------------------------------------------------------------------------- signed chains
@functools.lru_cache(maxsize=None)
def _signed_ref(n, seed, total, f32):
    """Restatement of the signed chain on the probe tone, sharing prefixes between totals."""
    chain = A.signed_chain(total)
    if not chain:
        return R.probe_signal(n, seed=seed, f0=150.0)
    prev = _signed_ref(n, seed, 0 if len(chain) == 1 else (4 if total > 0 else -4) * (len(chain) - 1), f32)
    return R.pitch_shift(prev, chain[-1], np.float32 if f32 else np.float64)


def test_signed_chains_equal_their_steps_one_by_one():
    n, totals = 12001, (-9.37, -3.37, 1.63, 6.63, 0.02)
    x = probe(n, 6)
    got = A.pitch_shift_chain([x] * len(totals), list(totals), signed=True)
    assert got[4] is x                                                            # the deadband: the input itself
    for t, g in zip(totals[:4], got):
        cur = x
        for s in A.signed_chain(t):
            cur = A.pitch_shift([cur], s)[0]
        assert torch.equal(g, cur), t
        check(g.cpu(), _signed_ref(n, 6, t, False), _signed_ref(n, 6, t, True), f"signed chain total {t} len {n}")
    stacked = A.pitch_shift_chain(torch.stack([x, x]), [-3.37, 6.63], signed=True)             # (B, L) form: rows are different tensors
    assert torch.equal(stacked[0], got[1]) and torch.equal(stacked[1], got[3])
    assert A.pitch_shift_chain([x, x], [-3, 5])[0] is x                           # signed=False: today's rule
