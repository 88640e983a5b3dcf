"""CPU suite for the arranger's performed mode: the restated envelope (tests/perform_ref.py) against what the reference's own
tools.adsr_envelope recorded in golden/perform.npz, MIDI pairing and the tempo integral against values written out by hand, Performance
and the planning of the shaped mix, the new C entry's argument validation without a device, and the unchanged default."""
import ctypes
import dataclasses

import numpy as np
import pytest

import arranger_ref as R
import perform_ref as P
from conftest import load_golden
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

CASES = ("ordinary", "attack_decay_zero", "attack_decay_past_hold", "one_sample_segments", "release_zero", "longer_than_signal",
         "release_one_second", "sustain_zero")


def on(dt, note, vel=80):
    return R.Msg((0, dt, note, vel, 0, 0))


def off(dt, note):
    return R.Msg((0, dt, note, 0, 0, 0))


def noff(dt, note, vel=64):
    return R.Msg((1, dt, note, vel, 0, 0))


def tempo(dt, us):
    return R.Msg((2, dt, 0, 0, us, 1))


def meta(dt):
    return R.Msg((3, dt, 0, 0, 0, 1))


def chan(msg, c):
    msg.channel = c
    return msg


def events_of(t):
    return [(e.note, e.velocity, e.start_time, e.duration) for e in t.events]


def _all_tracks(g):
    for name in g["names"]:
        for k in range(int(g[f"{name}.n_tracks"])):
            yield str(name), int(g[f"{name}.tpb"]), f"{name}.t{k}."


# ---------------------------------------------------------------------------------------------------- the envelope
@pytest.mark.parametrize("case", CASES)
def test_restated_envelope_equals_the_reference_function(case):
    g = load_golden("perform")
    assert case in [str(n) for n in g["names"]]
    length, seed, sr, dur, at, dt, sus, rt = g[case + ".params"].tolist()
    want = g[case + ".out"]
    got = P.adsr(P.golden_signal(length, seed), int(sr), dur, at, dt, sus, rt)
    assert want.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
    n_a, n_d, n_s, n_r = P.segments(int(sr), dur, at, dt, sus, rt)
    assert A.adsr_segments(int(sr), dur, at, dt, sus, rt) == (n_a, n_d, n_s, n_r) and len(want) == n_a + n_d + n_s + int(sr)
    assert not want[n_a + n_d + n_s + n_r:].any()                               # behind the release: zeros


def test_fixture_holds_the_telling_cases():
    g = load_golden("perform")
    seg = {c: P.segments(int(g[c + ".params"][2]), *g[c + ".params"][3:].tolist()) for c in CASES}
    assert seg["attack_decay_zero"][:2] == (0, 0) and seg["one_sample_segments"] == (1, 1, 1, 1) and seg["release_zero"][3] == 0
    assert seg["attack_decay_past_hold"][2] == 0 and sum(seg["attack_decay_past_hold"][:2]) > int(g["attack_decay_past_hold.params"][3] * 2000)
    assert len(g["longer_than_signal.out"]) > g["longer_than_signal.params"][0]
    assert min(seg["ordinary"]) > 1


def test_release_longer_than_a_second_is_refused():
    g = load_golden("perform")
    length, seed, sr, dur, at, dt, sus, rt = g["refused"].tolist()
    assert rt > 1.0
    with pytest.raises(AssertionError):
        P.adsr(P.golden_signal(length, seed), int(sr), dur, at, dt, sus, rt)
    with pytest.raises(ValueError, match="release_time > 1.0"):
        A.adsr_segments(int(sr), dur, at, dt, sus, rt)


# ---------------------------------------------------------------------------------------------------- pairing
PAIRING = {
    "chord closed in opening order": ([on(0, 60, 70), on(0, 64, 90), off(480, 60), off(0, 64)], [(60, 70, 0, 480), (64, 90, 0, 480)]),
    "chord closed in reverse order": ([on(0, 60, 70), on(0, 64, 90), off(240, 64), off(240, 60)], [(60, 70, 0, 480), (64, 90, 0, 240)]),
    "one pitch opened twice (FIFO)": ([on(0, 60, 50), on(100, 60, 80), off(100, 60), off(100, 60)], [(60, 50, 0, 200), (60, 80, 100, 200)]),
    "note_off closes, unmatched closes are ignored": ([on(0, 60, 70), noff(120, 60), off(10, 61), noff(10, 60)], [(60, 70, 0, 120)]),
    "a note left open ends at the last tick": ([on(0, 60, 70), on(50, 62, 71), off(50, 60), meta(30)], [(60, 70, 0, 100), (62, 71, 50, 80)]),
    "two channels on one pitch": ([chan(on(0, 60, 70), 0), chan(on(10, 60, 90), 1), chan(off(100, 60), 1), chan(off(50, 60), 0)],
                                  [(60, 70, 0, 160), (60, 90, 10, 100)]),
}


@pytest.mark.parametrize("case", list(PAIRING))
def test_midi_pairing(case):
    msgs, want = PAIRING[case]
    assert events_of(A.Track(msgs, 480, pairing="midi")) == want
    assert P.midi_events(msgs)[0] == want


@pytest.mark.parametrize("key,tpb", [("syn_chord.t0.", "syn_chord.tpb"), ("Air_on_the_G_String.t0.", "Air_on_the_G_String.tpb")])
def test_pairing_on_the_golden_lists(key, tpb):
    g = load_golden("arranger")
    msgs = R.messages(g[key + "msgs"])
    for t in (A.Track(msgs, int(g[tpb])), A.Track(msgs, int(g[tpb]), pairing="reference")):
        assert np.array_equal(np.array([(e.note, e.start_time, e.duration) for e in t.events]), g[key + "events"])
        assert all(e.velocity == 0 for e in t.events)
    now, opened = 0, []
    for m in msgs:
        now += m.time
        if m.type == "note_on" and m.velocity > 0:
            opened.append((m.note, m.velocity, now))
    t = A.Track(msgs, int(g[tpb]), pairing="midi")
    assert [(e.note, e.velocity, e.start_time) for e in t.events] == opened     # every event: the pitch and velocity of its own note_on
    assert min(v for _, v, _ in opened) > 0 and events_of(t) == P.midi_events(msgs)[0]
    assert all(e.duration >= 0 for e in t.events)


def test_bad_pairing_arguments():
    with pytest.raises(ValueError, match="pairing"):
        A.Track([], 480, pairing="fifo")
    with pytest.raises(ValueError, match="tempo_map"):
        A.Track([], 480, tempo_map=[(0, 400000)])
    with pytest.raises(ValueError, match="tempo_map"):
        A.Track([], 480, pairing="reference", tempo_map=[])


# ---------------------------------------------------------------------------------------------------- tempo
def test_tempo_change_between_on_and_off():
    msgs = [tempo(0, 500000), on(0, 60), tempo(240, 250000), off(240, 60)]
    t = A.Track(msgs, 480, pairing="midi")
    held = 240 * 500000 * 1e-6 / 480 + 240 * 250000 * 1e-6 / 480                # 0.25 s at 120 bpm + 0.125 s at 240 bpm
    assert t.seconds(0) == 0.0 and t.held() == [held] and held == 0.375
    assert t.schedule()[0][1:3] == (0.75, 0) and P.Track(msgs, 480).plan()[0][:3] == (0.75, 0, held)
    assert t.tempo_map == [(0, 500000), (240, 250000)]


def test_of_two_tempo_entries_on_one_tick_the_last_holds():
    msgs = [tempo(0, 400000), tempo(0, 600000), on(480, 60), tempo(480, 300000), tempo(0, 200000), off(480, 60)]
    t = A.Track(msgs, 480, pairing="midi")
    on_sec = 480 * 600000 * 1e-6 / 480
    off_sec = on_sec + 480 * 600000 * 1e-6 / 480 + 480 * 200000 * 1e-6 / 480
    assert t.seconds(480) == on_sec and t.seconds(1440) == off_sec
    assert t.schedule()[0][2] == int(on_sec * 16000) == 9600 and t.held() == [off_sec - on_sec]
    assert P.seconds(1440, 480, P.tempo_map_of([msgs])) == off_sec


def test_a_track_without_tempo_takes_the_files_map():
    t0 = [tempo(0, 250000), tempo(960, 1000000), meta(0)]
    t1 = [on(480, 60), off(960, 60)]
    file_map = A.tempo_map_of([t0, t1])
    assert file_map == [(0, 250000), (960, 1000000)] == P.tempo_map_of([t0, t1])
    own, shared = A.Track(t1, 480, pairing="midi"), A.Track(t1, 480, pairing="midi", tempo_map=file_map)
    assert own.schedule()[0][2] == int(480 * 500000 * 1e-6 / 480 * 16000) == 8000      # alone: 120 bpm
    on_sec = 480 * 250000 * 1e-6 / 480
    held = 480 * 250000 * 1e-6 / 480 + 480 * 1000000 * 1e-6 / 480                       # the change falls inside the note
    assert shared.schedule()[0][2] == int(on_sec * 16000) == 4000 and shared.held() == [(on_sec + held) - on_sec]
    assert shared.schedule()[0][1] == max((on_sec + held) - on_sec, 0.75) == 1.25


def test_a_meta_delta_in_front_of_a_note_counts():
    msgs = [meta(240), on(0, 60), off(480, 60)]
    assert A.Track(msgs, 480, pairing="midi").schedule()[0][2] == int(240 * 500000 * 1e-6 / 480 * 16000) == 4000
    assert A.Track(msgs, 480).schedule()[0][2] == 0                                      # the reference drops it


# ---------------------------------------------------------------------------------------------------- Performance, planning
def test_performance_validation():
    p = A.Performance()
    assert dataclasses.asdict(p) == dict(velocity_exponent=2.0, attack_time=0.0, decay_time=0.0, sustain_level=1.0, release_time=0.1,
                                         duration_step=0.0625)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.release_time = 0.2
    with pytest.raises(TypeError):
        A.Performance(2.0)                                                       # keyword-only
    bad = [dict(attack_time=-0.1), dict(decay_time=-1), dict(release_time=-0.01), dict(release_time=1.01), dict(sustain_level=1.5),
           dict(sustain_level=-0.1), dict(duration_step=0.0), dict(duration_step=-1.0), dict(velocity_exponent=float("nan")),
           dict(attack_time=float("inf")), dict(velocity_exponent=-1.0), dict(sustain_level="1"), dict(duration_step=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError, match="Performance"):
            A.Performance(**kw)
    assert A.Performance(release_time=1.0, sustain_level=0.0).release_time == 1.0
    assert p.gain(127) == 1.0 and p.gain(64) == (64 / 127) ** 2 and A.Performance(velocity_exponent=0.0).gain(1) == 1.0
    assert P.Perf().gain(49) == p.gain(49)
    import diffusynth_amd
    assert diffusynth_amd.Performance is A.Performance and diffusynth_amd.adsr_envelope is A.adsr_envelope
    assert diffusynth_amd.tempo_map_of is A.tempo_map_of


def test_duration_step_rounding():
    p = A.Performance()
    assert p.sampled_duration(0.75) == 0.75                                      # exactly on a multiple (12 steps): stays
    assert p.sampled_duration(0.3) == 0.75 and p.sampled_duration(0.0) == 0.75   # the floor first
    assert p.sampled_duration(0.76) == 0.8125 and p.sampled_duration(0.8125) == 0.8125 and p.sampled_duration(1.0) == 1.0
    assert p.sampled_duration(0.8125 + 1e-12) == 0.8125                          # 1.6e-11 steps above: that multiple
    assert p.sampled_duration(0.8125 + 1e-6) == 0.875
    q = A.Performance(duration_step=0.1)
    assert q.sampled_duration(0.9) == 9 * 0.1 and q.sampled_duration(0.3 * 3) == 9 * 0.1 and q.sampled_duration(0.91) == 10 * 0.1
    for held in (0.0, 0.3, 0.75, 0.76, 0.8125, 0.8125 + 1e-12, 0.8125 + 1e-6, 1.0, 2.345):
        assert P.Perf().sampled_duration(held) == p.sampled_duration(held)
    # one latent column at 16 kHz: durations of one sampled length share one sampled note
    width = lambda d: int(256 * ((d + 1) / 4) / 4)                               # noqa: E731
    assert width(p.sampled_duration(0.76)) == width(p.sampled_duration(0.81)) and str(p.sampled_duration(0.76)) == str(p.sampled_duration(0.81))


def test_block_lists_are_built_from_the_mixed_length():
    MX = L.MX
    assert MX["DS_MX_NI"] == 12 and MX["DS_MX_NI_PLAIN"] == 3 and (MX["DS_MX_START"], MX["DS_MX_OFF"], MX["DS_MX_LEN"]) == (0, 1, 2)
    ev = A.shaped_rows([0, 500, 3000], [0, 28416, 0], [28416, 5000, 28416], [0.5, 1.0, 0.25],
                       [(0, 0, 1000, 200, 1.0), (100, 200, 9000, 1600, 0.5), (1, 1, 1, 1, 0.25)])
    assert ev.dtype == np.int32 and ev.shape == (3, 12)
    assert ev[:, MX["DS_MX_LEN"]].tolist() == [1200, 5000, 4]                     # gated; the envelope outlasts the note; four samples
    assert ev[:, MX["DS_MX_NA"]:MX["DS_MX_NR"] + 1].tolist() == [[0, 0, 1000, 200], [100, 200, 9000, 1600], [1, 1, 1, 1]]
    fv = ev.view(np.float32)
    assert fv[:, MX["DS_MX_GAIN"]].tolist() == [0.5, 1.0, 0.25] and fv[:, MX["DS_MX_SUSTAIN"]].tolist() == [1.0, 0.5, 0.25]
    assert fv[1, MX["DS_MX_STEP_A"]] == np.float32(1 / 99) and fv[1, MX["DS_MX_STEP_D"]] == np.float32(-0.5 / 199)
    assert fv[1, MX["DS_MX_STEP_R"]] == np.float32(-0.5 / 1599) and fv[0, MX["DS_MX_STEP_R"]] == np.float32(-1 / 199)
    assert fv[2, MX["DS_MX_STEP_A"]:].tolist() == [0.0, 0.0, 0.0] and fv[0, MX["DS_MX_STEP_A"]] == 0.0    # segments of 0 or 1 samples
    ptr, lst = A.mix_lists(ev[:, 0].tolist(), ev[:, 2].tolist(), 30000)
    per = [lst[ptr[b]:ptr[b + 1]].tolist() for b in range(len(ptr) - 1)]
    assert per[0] == [0, 1] and per[1] == [0, 1] and per[2] == [1, 2] and per[5] == [1] and not any(per[6:])    # event 0 left after block 1
    plain_ptr, plain_lst = A.mix_lists([0, 500, 3000], [28416, 5000, 28416], 30000)
    assert len(plain_lst) > len(lst) and 0 in plain_lst[plain_ptr[10]:plain_ptr[11]]
    whole = A.shaped_rows([7], [0], [300], None, None)                            # no envelope: the whole note at level 1
    assert whole[0, :7].tolist() == [7, 0, 300, 0, 0, 300, 0] and whole.view(np.float32)[0, 7:].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    for kw in (dict(gains=[float("nan")], envelopes=None), dict(gains=None, envelopes=[(0, -1, 5, 0, 1.0)]), dict(gains=None, envelopes=[(0, 0, 1.5, 0, 1.0)]),
               dict(gains=[1.0, 2.0], envelopes=None)):
        with pytest.raises(ValueError, match="mix_notes"):
            A.shaped_rows([0], [0], [10], kw["gains"], kw["envelopes"])


def test_track_length_is_the_last_sounding_sample():
    msgs = [on(0, 60, 100), off(4800, 60), on(0, 64, 64), off(120, 64), meta(10000)]            # 5 s held, then 0.125 s held
    t = A.Track(msgs, 480, pairing="midi")
    sched = t.schedule()
    assert [s[1:3] for s in sched] == [(5.0, 0), (0.75, 80000)] and t.held() == [5.0, 0.125]
    lens = {sched[0][0]: 97024, sched[1][0]: 28416}
    assert t.track_length(note_lengths=lens) == 80000 + 28416                    # plain: the whole sampled note sounds
    p = A.Performance(release_time=0.25)
    sp = t.schedule(perform=p)
    assert [s[1] for s in sp] == [5.0, 0.75]
    assert t.mixed_lengths(lens, perform=p) == [80000 + 4000, 2000 + 4000]       # held + release
    assert t.track_length(note_lengths=lens, perform=p) == max(0 + 84000, 80000 + 6000) == 86000
    short = {sched[0][0]: 50000, sched[1][0]: 28416}
    assert t.track_length(note_lengths=short, perform=p) == 86000 and t.mixed_lengths(short, perform=p)[0] == 50000
    gains, envs = t.shape(perform=p)
    assert gains == [(100 / 127) ** 2, (64 / 127) ** 2] and envs == [(0, 0, 80000, 4000, 1.0), (0, 0, 2000, 4000, 1.0)]
    with pytest.raises(ValueError, match="note_lengths"):
        t.track_length()
    r = P.Track(msgs, 480)
    assert [(d, s) for d, s, *_ in r.plan(perf=P.Perf(release_time=0.25))] == [(s[1], s[2]) for s in sp]
    assert A.Track([], 480, pairing="midi").track_length(note_lengths={}) == 0


def test_perform_needs_midi_pairing():
    g = load_golden("arranger")
    t = A.Track(R.messages(g["syn_chord.t0.msgs"]), 480)
    for call in (lambda: t.schedule(perform=A.Performance()), lambda: t.shape(perform=A.Performance()),
                 lambda: t.render(lambda v, d: R.synthetic_note(d), perform=A.Performance())):
        with pytest.raises(ValueError, match="perform needs pairing"):
            call()
    with pytest.raises(ValueError, match="perform"):
        A.Track(R.messages(g["syn_chord.t0.msgs"]), 480, pairing="midi").render(None, perform={"release_time": 0.1})
    with pytest.raises(ValueError, match="perform needs pairing"):
        A.DiffSynth({}, None, None, None, None, None, "cuda", perform=A.Performance())
    with pytest.raises(ValueError, match="pairing"):
        A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="oldest")
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi", perform=A.Performance(release_time=0.3))
    assert ds.pairing == "midi" and ds.perform.release_time == 0.3


def test_the_plan_of_the_presets_matches_the_restatement():
    g = load_golden("arranger")
    p, rp = A.Performance(attack_time=0.01, decay_time=0.05, sustain_level=0.7, release_time=0.2), P.Perf(2.0, 0.01, 0.05, 0.7, 0.2)
    for name, tpb, key in _all_tracks(g):
        msgs = R.messages(g[key + "msgs"])
        t, r = A.Track(msgs, tpb, pairing="midi"), P.Track(msgs, tpb)
        assert [(s[1], s[2], s[3] + 52) for s in t.schedule()] == [(d, s, n) for d, s, _, n, _ in r.plan()], key
        plan = r.plan(perf=rp)
        assert [(s[1], s[2]) for s in t.schedule(perform=p)] == [(d, s) for d, s, *_ in plan], key
        shape = t.shape(perform=p)
        if plan:
            assert shape[0] == [rp.gain(v) for *_, v in plan] and shape[1] == [rp.segments(h, 16000) + (0.7,) for _, _, h, _, _ in plan], key


def test_the_default_is_unchanged_on_every_golden_list():
    g = load_golden("arranger")
    for name, tpb, key in _all_tracks(g):
        t = A.Track(R.messages(g[key + "msgs"]), tpb, 100)
        assert t.pairing == "reference"
        assert np.array_equal(np.array([(e.note, e.start_time, e.duration) for e in t.events], dtype=np.int64).reshape(-1, 3), g[key + "events"]), key
        assert all(e.velocity == 0 for e in t.events), key
        sched = t.schedule()
        r = R.Track(R.messages(g[key + "msgs"]), tpb, 100)
        want = []
        for e in r.events[:100]:
            spt = R.tick2second(1, tpb, r._get_tempo_at(e.start_time))
            dur = max(e.duration * spt, 0.75)
            want.append((str(dur), dur, int(e.start_time * spt * 16000), e.note - 52))
        assert sched == want and [s[2] for s in sched] == g[key + "starts"].tolist(), key
        assert t.track_length() == int(float(g[key + "total"]) * 16000), key


# ---------------------------------------------------------------------------------------------------- C ABI without a device
def test_shaped_entry_validates_before_any_gpu_work():
    lib = L.load()
    assert "ds_mix_notes_shaped" in L.EXPORTS and hasattr(lib, "ds_mix_notes_shaped")
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    for fn in (lambda: lib.ds_mix_notes_shaped(p, 10, p, 0, p, p, 0, p, 10, None), lambda: lib.ds_mix_notes_shaped(p, 10, p, 1, p, p, 0, p, 0, None),
               lambda: lib.ds_mix_notes_shaped(p, 10, p, 1, p, p, -1, p, 10, None), lambda: lib.ds_mix_notes_shaped(p, 10, None, 1, p, p, 0, p, 10, None),
               lambda: lib.ds_mix_notes_shaped(p, 1 << 31, p, 1, p, p, 0, p, 10, None),
               lambda: lib.ds_mix_notes_shaped(p, 10, p, 1 << 28, p, p, 0, p, 10, None)):
        assert fn() == -1
        assert b"mix_notes_shaped" in lib.ds_last_error_string()
    assert lib.ds_mix_notes_shaped(p, 10, p + 2, 1, p, p, 0, p, 10, None) == -3 and b"mix_notes_shaped" in lib.ds_last_error_string()
    with pytest.raises(L.DsError, match="mix_notes_shaped"):
        L.call("ds_mix_notes_shaped", p, 10, p, 0, p, p, 0, p, 10, None)
    assert lib.ds_mix_notes(p, 10, p, 0, p, p, 0, p, 10, None) == -1 and b"mix_notes: bad args" in lib.ds_last_error_string()
