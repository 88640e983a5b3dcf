"""The arranger's audio stage on the GPU against its float64 restatement (tests/arranger_ref.py).

Tolerance rule (every parity check of this file): the float32 twin of the restatement — the same operations in fp32, phasor form — is run
against the float64 form on the same inputs on the CPU; the device is allowed 8 x the twin's error (a different FFT factorisation, a
tabulated window and fused multiply-adds may cost that much; more is a bug), never less than 2e-6 (what fp32 kernels give against float64,
DESIGN §2) and never more than the project's 1e-3, through conftest.rel_err so that the max-norm and the rms error are both held.  Each
check prints its figure and its bound.
"""
import functools

import numpy as np
import pytest
import torch

import arranger_ref as R
from conftest import load_golden, rel_err, rel_errs
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

pytestmark = pytest.mark.gpu

NB = R.N_FFT // 2 + 1
SINGLE = [(28416,), (77568,), (30001,)]                                       # latent widths 28 and 76 (the presets' extremes) and an odd length
RAGGED = (28416, 77568, 30001, 4097, 1023, 50000, 28416)
STEPS7 = (1, 2, 3, 4, -3, 0.5, 4)
BATCHES = [(n, (4,)) for n in SINGLE] + [(RAGGED, STEPS7)]
IDS = ["28416", "77568", "30001", "ragged7"]


def bound(twin, want):
    """8 x the twin's error, inside [2e-6, 1e-3]."""
    return min(max(8.0 * max(rel_errs(twin, want)), 2e-6), 1e-3)


def check(got, want, twin, what):
    err, tol = rel_err(got, want), bound(twin, want)
    print(f"{what}: device {err:.2e}, twin {max(rel_errs(twin, want)):.2e}, bound {tol:.2e}")
    assert err < tol, (what, err, tol)


def signal(n, seed):
    return R.probe_signal(n, seed=seed)


def cplx(a):
    """complex array -> (..., 2) float view for the norms."""
    a = np.asarray(a)
    return np.stack([a.real, a.imag], axis=-1)


class Stages:
    """The four entry points of one batched pitch_shift, each callable on its own input."""

    def __init__(self, lengths, steps):
        self.p = p = A._Plan(list(lengths), list(steps))
        self.tab_host = p.host[p.o_tab:p.o_idx].reshape(-1, L.PV["DS_PV_NI"])
        self.tables = torch.from_numpy(p.host).cuda()
        b = self.tables.data_ptr()
        self.rates, self.tab, self.idx, self.alpha = b, b + 4 * p.o_tab, b + 4 * p.o_idx, b + 4 * p.o_alpha
        self.st = L.current_stream()

    def col(self, name):
        return self.tab_host[:, L.PV[name]].tolist()

    def split(self, flat, off, cnt, width=1):
        flat = flat.cpu().numpy()
        return [flat[o * width:(o + n) * width] for o, n in zip(self.col(off), self.col(cnt))]

    def stft(self, sigs):
        p, x = self.p, torch.from_numpy(np.concatenate(sigs)).cuda()
        spec = torch.full((p.total_frames * NB * 2,), float("nan"), device="cuda")
        L.call("ds_pv_stft", x.data_ptr(), self.tab, p.n, p.max_frames, p.total_samples, p.total_frames, spec.data_ptr(), self.st)
        return [s.reshape(-1, NB, 2) for s in self.split(spec, "DS_PV_FOFF", "DS_PV_NF", NB * 2)]

    def vocode(self, specs):
        p = self.p
        spec = torch.from_numpy(np.concatenate([cplx(s).astype(np.float32).reshape(-1) for s in specs])).cuda()
        voc = torch.full((p.total_out * NB * 2,), float("nan"), device="cuda")
        L.call("ds_pv_vocode", spec.data_ptr(), self.tab, self.idx, self.alpha, p.n, p.total_frames, p.total_out, voc.data_ptr(), self.st)
        return [s.reshape(-1, NB, 2) for s in self.split(voc, "DS_PV_TOFF", "DS_PV_NOUT", NB * 2)]

    def istft(self, vocs):
        p = self.p
        voc = torch.from_numpy(np.concatenate([cplx(s).astype(np.float32).reshape(-1) for s in vocs])).cuda()
        ws = torch.empty(L.load().ds_pv_istft_ws_bytes(p.total_out) // 4, device="cuda")
        y = torch.full((p.total_stretched,), float("nan"), device="cuda")
        L.call("ds_pv_istft", voc.data_ptr(), self.tab, p.n, p.max_out, p.max_stretched, p.total_out, p.total_stretched, ws.data_ptr(), y.data_ptr(), self.st)
        return self.split(y, "DS_PV_SOFF", "DS_PV_SLEN")

    def resample(self, ys):
        p = self.p
        x = torch.from_numpy(np.concatenate(ys).astype(np.float32)).cuda()
        out = torch.full((p.total_samples,), float("nan"), device="cuda")
        L.call("ds_resample_sinc", x.data_ptr(), self.tab, self.rates, p.n, p.max_len, p.total_stretched, p.total_samples, out.data_ptr(), self.st)
        return self.split(out, "DS_PV_XOFF", "DS_PV_LEN")


def _inputs(lengths):
    return [signal(n, 10 + i) for i, n in enumerate(lengths)]


# ---------------------------------------------------------------------------------------------------- each kernel alone
@pytest.mark.parametrize("lengths,steps", BATCHES, ids=IDS)
def test_stft_kernel(lengths, steps):
    sigs = _inputs(lengths)
    for i, got in enumerate(Stages(lengths, steps).stft(sigs)):
        want, twin = R.stft(sigs[i]), R.stft(sigs[i], np.float32)
        assert got.shape[:2] == want.shape
        check(got, cplx(want), cplx(twin), f"stft[{i}] len {lengths[i]}")


@pytest.mark.parametrize("lengths,steps", BATCHES, ids=IDS)
def test_vocode_kernel(lengths, steps):
    specs = [R.stft(s).astype(np.complex64) for s in _inputs(lengths)]
    specs[0][3, 50:60] = 0                                                     # zero bins: unit phasor 1, magnitude 0
    for i, got in enumerate(Stages(lengths, steps).vocode(specs)):
        rate = R.rate_of(steps[i])
        want = R.phase_vocoder(specs[i].astype(np.complex128), rate)
        twin = R.phase_vocoder(specs[i], rate, np.float32)
        assert got.shape[:2] == want.shape
        check(got, cplx(want), cplx(twin), f"vocode[{i}] len {lengths[i]} n_steps {steps[i]}")


@pytest.mark.parametrize("lengths,steps", BATCHES, ids=IDS)
def test_istft_kernel(lengths, steps):
    vocs = [R.phase_vocoder(R.stft(s), R.rate_of(st)).astype(np.complex64) for s, st in zip(_inputs(lengths), steps)]
    for i, got in enumerate(Stages(lengths, steps).istft(vocs)):
        n = R.stretched_length(lengths[i], R.rate_of(steps[i]))
        want, twin = R.istft(vocs[i].astype(np.complex128), n), R.istft(vocs[i], n, np.float32)
        assert got.shape == want.shape
        check(got, want, twin, f"istft[{i}] len {lengths[i]} -> {n}")


@pytest.mark.parametrize("lengths,steps", BATCHES, ids=IDS)
def test_resample_kernel(lengths, steps):
    ys = [signal(R.stretched_length(n, R.rate_of(st)), 30 + i) for i, (n, st) in enumerate(zip(lengths, steps))]
    for i, got in enumerate(Stages(lengths, steps).resample(ys)):
        rate = R.rate_of(steps[i])
        nres = min(R.resampled_length(len(ys[i]), rate), lengths[i])
        want, twin = np.zeros(lengths[i]), np.zeros(lengths[i], np.float32)
        want[:nres], twin[:nres] = R.resample(ys[i], rate, nres), R.resample(ys[i], rate, nres, np.float32)
        assert got.shape == want.shape and not got[nres:].any()               # fix_length: zeros behind ceil(len_stretched * rate)
        check(got, want, twin, f"resample[{i}] len {lengths[i]} rate {rate:.4f}")


@pytest.mark.parametrize("lengths", [n for n, _ in BATCHES], ids=IDS)
def test_peak_normalize_kernel(lengths):
    sigs = [3.7 * s for s in _inputs(lengths)]
    for i, got in enumerate(A.peak_normalize([torch.from_numpy(s).cuda() for s in sigs])):
        want = sigs[i].astype(np.float64) / np.abs(sigs[i].astype(np.float64)).max()
        twin = sigs[i] / np.max(np.abs(sigs[i]))
        check(got.cpu(), want, twin, f"peak_normalize[{i}]")
        assert np.array_equal(got.cpu().numpy(), twin)                         # a true division: numpy's fp32 result bit for bit


# ---------------------------------------------------------------------------------------------------- pitch_shift, chains
@functools.lru_cache(maxsize=None)
def _chain_ref(n, seed, total, f32):
    """Restatement of the chain on signal(n, seed), sharing prefixes between totals."""
    steps = R.chain_steps(total)
    if not steps:
        return signal(n, seed)
    prev = _chain_ref(n, seed, total - steps[-1], f32)
    return R.pitch_shift(prev, steps[-1], np.float32 if f32 else np.float64)


@pytest.mark.parametrize("n_steps", [1, 2, 3, 4, -3, 0.5])
def test_pitch_shift(n_steps):
    sigs = _inputs((28416, 30001))
    got = A.pitch_shift([torch.from_numpy(s).cuda() for s in sigs], n_steps)
    for i, s in enumerate(sigs):
        check(got[i].cpu(), R.pitch_shift(s, n_steps), R.pitch_shift(s, n_steps, np.float32), f"pitch_shift n_steps {n_steps} [{i}]")
    same = A.pitch_shift(torch.from_numpy(np.stack([sigs[0], sigs[0]])).cuda(), n_steps)       # (B, L) form
    assert same.shape == (2, 28416) and torch.equal(same[0], got[0]) and torch.equal(same[1], got[0])


@pytest.mark.parametrize("n", [28416, 77568])
def test_pitch_shift_chain(n):
    totals = [1, 4, 5, 8, 12, 31, 32, 0, -7]
    x = torch.from_numpy(signal(n, 5)).cuda()
    got = A.pitch_shift_chain([x] * len(totals), totals)
    for t, g in zip(totals, got):
        if t <= 0:
            assert g is x and torch.equal(g, x)                                # the reference's empty loop: the input itself
        else:
            check(g.cpu(), _chain_ref(n, 5, t, False), _chain_ref(n, 5, t, True), f"chain total {t} len {n}")
    one = A.pitch_shift_librosa(x, 16000, 5)
    assert torch.equal(one, got[2])


def test_ragged_batch_equals_its_signals_one_by_one_and_runs_repeat():
    sigs = [torch.from_numpy(s).cuda() for s in _inputs(RAGGED)]
    a = A.pitch_shift(sigs, list(STEPS7))
    b = A.pitch_shift(sigs, list(STEPS7))
    for i, s in enumerate(sigs):
        assert torch.equal(a[i], b[i]), i                                      # no atomics: two runs are bit-equal
        assert torch.equal(a[i], A.pitch_shift([s], STEPS7[i])[0]), i          # what shares the batch does not matter


def test_tree_equals_the_naive_chains():
    xs = [torch.from_numpy(signal(n, 7 + i)).cuda() for i, n in enumerate((28416, 30001))]
    reqs = [(0, 31), (0, 5), (1, 8), (0, 8), (1, 1), (0, -2), (1, 12), (0, 4), (0, 31)]
    got = A.pitch_shift_chain([xs[i] for i, _ in reqs], [t for _, t in reqs])
    for (i, t), g in zip(reqs, got):
        cur = xs[i]
        for s in A.chain_steps(t):
            cur = A.pitch_shift([cur], s)[0]
        assert torch.equal(g, cur), (i, t)
    assert sum(len(lv) for lv in A.shift_tree(reqs)) == 9 + 4                    # signal 0: 4, 8 .. 28, 31 and 5; signal 1: 4, 8, 12 and 1


# ---------------------------------------------------------------------------------------------------- mix, Track
def _cached_chain(dtype):
    """R.pitch_shift_chain that computes every (note, cumulative semitones) once (the restatement's Track hands over the same array per
    duration)."""
    have = {}

    def shift(y, total):
        steps = R.chain_steps(total)
        if not steps:
            return y
        key = (id(y), total)
        if key not in have:
            have[key] = (y, R.pitch_shift(shift(y, total - steps[-1]), steps[-1], dtype))
        return have[key][1]
    return shift


def test_mix_notes_equals_numpy():
    rng = np.random.default_rng(0)
    n = 40000
    notes = [rng.standard_normal(m).astype(np.float32) for m in (28416, 5000, 1, 11584, 2048)]
    events = [(0, 0), (100, 1), (100, 1), (1023, 2), (28416, 3), (3000, 4), (n - 5000, 1), (1024, 4), (0, 4)]     # sample 0, the last sample, overlaps
    want = np.zeros(n, dtype=np.float32)
    for start, i in events:
        want[start:start + len(notes[i])] += notes[i].astype(np.float64)
    got = A.mix_notes([torch.from_numpy(x).cuda() for x in notes], events, n)
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="does not fit"):
        A.mix_notes([torch.from_numpy(x).cuda() for x in notes], [(n - 4999, 1)], n)


@pytest.mark.parametrize("case", ["syn_tempo", "syn_chord"])
def test_track_render_matches_the_reference_track_audio(case):
    g = load_golden("arranger")
    msgs, tpb = R.messages(g[case + ".t0.msgs"]), int(g[case + ".tpb"])
    want = g[case + ".t0.audio"]
    calls = []

    def note_fn(velocity, duration):
        calls.append(duration)
        return R.synthetic_note(duration)
    t = A.Track(msgs, tpb, 100)
    got = t.synthesize_track(note_fn)
    assert got.dtype == np.float32 and len(got) == int(float(g[case + ".t0.total"]) * 16000) and not got[len(want):].any()
    assert len(calls) == len(set(calls)) == len({s[0] for s in t.schedule()})  # once per distinct duration
    twin = R.Track(msgs, tpb, 100).synthesize_track(lambda v, d: R.synthetic_note(d), shift=_cached_chain(np.float32))
    check(got[:len(want)], want, twin[:len(want)], f"Track.render {case}")
    dev = t.render(lambda v, d: torch.from_numpy(R.synthetic_note(d)).cuda())  # a tensor callback, the track left on the device
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)


def test_a_note_past_the_end_of_the_track_is_rejected():
    g = load_golden("arranger")
    t = A.Track(R.messages(g["syn_chord.t0.msgs"]), int(g["syn_chord.tpb"]), 100)
    with pytest.raises(ValueError, match="ends past"):
        t.render(lambda v, d: np.ones(400000, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------- DiffSynth.get_music
class _Mid:
    def __init__(self, g, name):
        self.ticks_per_beat = int(g[name + ".tpb"])
        self.tracks = [R.messages(g[f"{name}.t{k}.msgs"]) for k in range(int(g[name + ".n_tracks"]))]


def test_get_music_ode_to_joy(unet_sd, vqgan_sd):
    from diffusynth_amd.synth import synth_input
    from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet
    from diffusynth_amd.vqgan import PRODUCTION_CONFIG as VQ_CFG, VQGAN
    net = ConditionedUnet(**PRODUCTION_CONFIG)
    net.load_state_dict(unet_sd)
    net.to("cuda")
    vae = VQGAN(**VQ_CFG)
    vae.load_state_dict(vqgan_sd)
    vae.to("cuda")
    g = load_golden("arranger")
    mid = _Mid(g, "Ode_to_Joy_Easy_variation")
    cfg = lambda tag: dict(sample_steps=3, sampler="ddpm", noising_strength=0.7, attack=0.5, before_release=0.5,      # noqa: E731
                           latent_representation=synth_input("arr_guide_" + tag, (1, 4, 128, 64)).cuda())
    ds = A.DiffSynth({"organ": cfg("a"), "string": cfg("b")}, net, vae._vq_vae, vae._decoder, None, None, "cuda",
                     condition=synth_input("arr_cond", (1, 512)).cuda(), seed=11)
    music = ds.get_music(mid, ["organ", "string"], max_notes=20)
    tracks = [A.Track(t, mid.ticks_per_beat, 20) for t in mid.tracks]
    assert music.dtype == np.float32 and np.isfinite(music).all() and np.abs(music).max() > 0
    assert len(music) == max(t.track_length() for t in tracks)
    wanted = {(name, s[1]) for name, t in zip(("organ", "string"), tracks) for s in t.schedule()}
    widths = {ds.note_width(d) for _, d in wanted}
    b = ds.last_batcher
    per_width = {w: max(n for n, _, ww, *_ in b.unet_batches if ww == w) for w in {ww for _, _, ww, *_ in b.unet_batches}}
    assert set(per_width) == widths and sum(per_width.values()) == len(wanted)   # one request per distinct (instrument, duration), batched per width
    assert b.plan_builds <= len(widths)
    # the same notes off the batcher (same seeds -> same notes, bit for bit) through the float64 restatement on the host
    ds2 = A.DiffSynth(ds.instruments_configs, net, vae._vq_vae, vae._decoder, None, None, "cuda", condition=ds.condition, seed=11)
    order = [(name, s[1]) for name, t in zip(("organ", "string"), tracks) for s in t.schedule()]
    notes = {k: v.cpu().numpy() for k, v in ds2.sample_notes(order).items()}
    want = np.zeros(len(music))
    twin = np.zeros(len(music), np.float32)
    for name, (msgs, t) in zip(("organ", "string"), zip(mid.tracks, tracks)):
        r = R.Track(msgs, mid.ticks_per_beat, 20)
        fn = lambda v, d, name=name: notes[(name, d)]                          # noqa: E731
        a64 = r.synthesize_track(fn, shift=_cached_chain(np.float64))
        a32 = r.synthesize_track(fn, shift=_cached_chain(np.float32))
        want[:len(a64)] += a64
        twin[:len(a32)] += a32
    check(music, want, twin, "get_music Ode to Joy, 20 notes per track")
