"""The formant-preserving pitch shift on the GPU: ds_pv_formant alone and pitch_shift(formant=...) / chains against the restatement
(tests/formant_ref.py), identity at rate 1, every signal its own, the tree against its chains, formant=None against the call without
the argument, bounds, and the property that justifies the mode on the device's own +12 chain.

Tolerance rule: that of tests/test_hip_arranger.py — the device may err 8 x what the restatement's float32 twin errs against its float64
form on the same inputs, through conftest.rel_err, capped at the project's 1e-3 — with one derived change to its floor: 2e-6 max(1, max|L|),
max|L| taken from the float64 reference of the case.  The smoothed log envelope S is a linear transform of L = ln max(|V|, 1e-6), so an
fp32 transform returns it with an ABSOLUTE error of the project's 2e-6 times the size of L, and exp turns the exponent's absolute error
into the gain's relative error.  Each check prints the device's figure, the twin's figure and the bound."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import arranger_ref as R
import formant_ref as F
from conftest import load_golden, rel_err, rel_errs
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

pytestmark = pytest.mark.gpu

NB = R.N_FFT // 2 + 1
LENGTHS = (30001, 4097, 1023, 28416, 4097)         # odd frame counts, one- and two-frame signals, a rate-1 row, a repeated length
STEPS = (4, -3, 0.5, 0, 4)
FM = A.Formant()
GAIN_DB = FM.max_gain_db


def bound(twin, want, max_abs_l):
    return min(max(8.0 * max(rel_errs(twin, want)), 2e-6 * max(1.0, max_abs_l)), 1e-3)


def check(got, want, twin, max_abs_l, what):
    err, tol = rel_err(got, want), bound(twin, want, max_abs_l)
    print(f"{what}: device {err:.2e}, twin {max(rel_errs(twin, want)):.2e}, bound {tol:.2e} (max|L| {max_abs_l:.2f})")
    assert err < tol, (what, err, tol)


def cplx(a):
    a = np.asarray(a)
    return np.stack([a.real, a.imag], axis=-1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def signals():
    return tuple(R.probe_signal(n, seed=40 + i) for i, n in enumerate(LENGTHS))


@functools.lru_cache(maxsize=None)
def vocs():
    """The synthesis frames of every signal as the phase vocoder hands them over (complex64), with a run of bins at the floor."""
    out = [R.phase_vocoder(R.stft(s), R.rate_of(st)).astype(np.complex64) for s, st in zip(signals(), STEPS)]
    out[0][3, 50:60] = 0
    return tuple(out)


def launch(frames, lengths, steps, orders, *, limit=FM.limit, pad=0, fill=-777.0, edit=None):
    """ds_pv_formant on its own: frames (one (nout, 2049) complex64 array per signal) -> the corrected frames, and the padding behind voc.
    edit(tab): changes the signal table (int32 (n, DS_PV_NI)) before the upload."""
    p = A._Plan(list(lengths), list(steps), list(orders))
    host = p.host.copy()
    tab = host[p.o_tab:p.o_idx].reshape(-1, L.PV["DS_PV_NI"])
    toff, nout = tab[:, L.PV["DS_PV_TOFF"]].tolist(), tab[:, L.PV["DS_PV_NOUT"]].tolist()
    assert [len(f) for f in frames] == nout
    if edit is not None:
        edit(tab)
    tables = torch.from_numpy(host).cuda()
    b = tables.data_ptr()
    flat = np.concatenate([cplx(f).astype(np.float32).reshape(-1) for f in frames] + [np.full(pad, fill, np.float32)])
    voc = torch.from_numpy(flat).cuda()
    L.call("ds_pv_formant", voc.data_ptr(), b + 4 * p.o_tab, b + 4 * p.o_order, b + 4 * p.o_warp, limit, p.n, p.max_out, p.total_out, L.current_stream())
    got = voc.cpu().numpy()
    return [got[o * NB * 2:(o + n) * NB * 2].reshape(-1, NB, 2) for o, n in zip(toff, nout)], got[p.total_out * NB * 2:]


@functools.lru_cache(maxsize=None)
def batch(order):
    return launch(vocs(), LENGTHS, STEPS, [order] * len(LENGTHS))[0]


# ---------------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("order", [30, 7, 512])
def test_kernel_against_the_restatement(order):
    assert sorted(len(v) % 2 for v in vocs()) == [0, 0, 0, 1, 1] and min(len(v) for v in vocs()) <= 2        # odd counts, a signal of <= 2 frames
    for i, got in enumerate(batch(order)):
        rate, info = R.rate_of(STEPS[i]), {}
        want = F.correct(vocs()[i].astype(np.complex128), rate, order, GAIN_DB, info=info)
        twin = F.correct(vocs()[i], rate, order, GAIN_DB, np.float32)
        assert got.shape[:2] == want.shape
        check(got, cplx(want), cplx(twin), info["max_abs_L"], f"formant[{i}] len {LENGTHS[i]} n_steps {STEPS[i]} order {order} ({len(want)} frames)")
    changed = [not np.array_equal(bits(g), bits(cplx(v))) for g, v in zip(batch(order), vocs())]
    assert changed == [True, True, True, False, True]                              # not vacuous: every row but the rate-1 one was corrected


def test_the_clamp_is_reached_and_held():
    """A limit of 1 dB: most bins sit on it, and no gain exceeds it by more than fp32 rounding."""
    lim_db = 1.0
    fm = A.Formant(max_gain_db=lim_db)
    got = launch(vocs()[:1], LENGTHS[:1], STEPS[:1], [30], limit=fm.limit)[0][0]
    v = cplx(vocs()[0]).astype(np.float64)
    mag_in, mag_out = np.hypot(v[..., 0], v[..., 1]), np.hypot(got[..., 0].astype(np.float64), got[..., 1].astype(np.float64))
    g = mag_out[mag_in > 1e-3] / mag_in[mag_in > 1e-3]
    hi = np.exp(fm.limit)
    print(f"gains inside [{g.min():.6f}, {g.max():.6f}], limit {hi:.6f}; {np.mean(np.abs(np.log(g)) > 0.999 * fm.limit):.2f} of the bins on it")
    assert g.max() <= hi * (1 + 1e-6) and g.min() >= 1 / hi * (1 - 1e-6) and np.mean(np.abs(np.log(g)) > 0.999 * fm.limit) > 0.2
    info = {}
    want = F.correct(vocs()[0].astype(np.complex128), R.rate_of(STEPS[0]), 30, lim_db, info=info)
    check(got, cplx(want), cplx(F.correct(vocs()[0], R.rate_of(STEPS[0]), 30, lim_db, np.float32)), info["max_abs_L"], "formant, limit 1 dB")


# ---------------------------------------------------------------------------------------------------- 2. rate 1
@pytest.mark.parametrize("order", [30, 7, 512])
def test_a_rate_one_row_keeps_its_bits(order):
    got, src = torch.from_numpy(batch(order)[3]), torch.from_numpy(cplx(vocs()[3]).astype(np.float32))
    assert STEPS[3] == 0 and torch.equal(got, src) and np.array_equal(bits(got.numpy()), bits(src.numpy()))


def test_a_shift_by_zero_with_a_formant_is_the_plain_shift_by_zero():
    x = torch.from_numpy(signals()[3]).cuda()
    assert torch.equal(A.pitch_shift([x], 0, formant=FM)[0], A.pitch_shift([x], 0)[0])


# ---------------------------------------------------------------------------------------------------- 3. each signal is its own
def test_a_signal_alone_equals_the_signal_in_the_ragged_batch():
    for order in (30, 512):
        for i, want in enumerate(batch(order)):
            alone = launch(vocs()[i:i + 1], LENGTHS[i:i + 1], STEPS[i:i + 1], [order])[0][0]
            assert torch.equal(torch.from_numpy(alone), torch.from_numpy(want)), (order, i)
    mixed = launch(vocs(), LENGTHS, STEPS, [30, 7, 512, 30, 7])[0]                  # an order is its row's own
    for i, o in enumerate((30, 7, 512, 30, 7)):
        assert torch.equal(torch.from_numpy(mixed[i]), torch.from_numpy(batch(o)[i])), i
    sigs = [torch.from_numpy(s).cuda() for s in signals()]
    a, b = A.pitch_shift(sigs, list(STEPS), formant=FM), A.pitch_shift(sigs, list(STEPS), formant=FM)
    for i, s in enumerate(sigs):
        assert torch.equal(a[i], b[i]), i                                          # no atomics: two runs are bit-equal
        assert torch.equal(a[i], A.pitch_shift([s], STEPS[i], formant=FM)[0]), i


# ---------------------------------------------------------------------------------------------------- 4. pitch_shift, chain
def test_pitch_shift_with_a_formant_against_the_restatement():
    sigs = [torch.from_numpy(s).cuda() for s in signals()]
    got = A.pitch_shift(sigs, list(STEPS), formant=FM)
    plain = A.pitch_shift(sigs, list(STEPS))
    for i, s in enumerate(signals()):
        info = {}
        want = F.pitch_shift_formant(s, STEPS[i], FM.order, GAIN_DB, info=info)
        twin = F.pitch_shift_formant(s, STEPS[i], FM.order, GAIN_DB, np.float32)
        check(got[i].cpu(), want, twin, info["max_abs_L"], f"pitch_shift(formant) [{i}] len {LENGTHS[i]} n_steps {STEPS[i]}")
        assert torch.equal(got[i], plain[i]) == (STEPS[i] == 0), i                 # the mode changes every shifted signal


@functools.lru_cache(maxsize=None)
def device_chains():
    """The probe note shifted +12 on the device, plain and with the default Formant (shared by the parity and the property test)."""
    x = torch.from_numpy(F.probe()).cuda()
    return A.pitch_shift_chain([x], [12])[0].cpu().numpy(), A.pitch_shift_chain([x], [12], formant=FM)[0].cpu().numpy()


def test_chain_of_twelve_with_a_formant_against_the_restatement():
    """On the signal the plain chains are held to (arranger_ref.probe_signal: a tone over a noise floor, as a sampled note is).  The
    noiseless two-formant probe of the property test is no parity case: between its partials the spectrum is the transform's own rounding
    noise, the logarithm turns that noise into the envelope, and the restatement's float32 twin is then 4.9e-3 off its float64 form after
    three links (the device: 4.6e-3) — the input is ill-conditioned for ANY fp32 evaluation, and the rule's cap of 1e-3 says nothing there."""
    y, info = R.probe_signal(28416, seed=5), {}
    want = F.pitch_shift_chain_formant(y, 12, FM.order, GAIN_DB, FM.track_pitch, info=info)
    twin = F.pitch_shift_chain_formant(y, 12, FM.order, GAIN_DB, FM.track_pitch, dtype=np.float32)
    x = torch.from_numpy(y).cuda()
    got = A.pitch_shift_chain([x], [12], formant=FM)[0]
    check(got.cpu(), want, twin, info["max_abs_L"], "chain +12 with Formant()")
    assert torch.equal(A.pitch_shift_librosa(x, 16000, 12, formant=FM), got)


# ---------------------------------------------------------------------------------------------------- 5. the tree
@pytest.mark.parametrize("track_pitch", [True, False])
def test_tree_equals_the_chains_run_one_by_one(track_pitch):
    fm = A.Formant(order=30, track_pitch=track_pitch)
    xs = [torch.from_numpy(R.probe_signal(n, seed=7 + i)).cuda() for i, n in enumerate((9000, 4097))]
    reqs = [(0, 13), (0, 5), (1, 8), (0, 8), (1, 1), (0, -2), (1, 12), (0, 4), (0, 13)]
    got = A.pitch_shift_chain([xs[i] for i, _ in reqs], [t for _, t in reqs], formant=fm)
    for (i, t), g in zip(reqs, got):
        cur, lo = xs[i], 0
        for s in A.chain_steps(t):
            cur = A.pitch_shift([cur], s, formant=dataclasses.replace(fm, order=fm.node_order(lo)))[0]
            lo += s
        assert torch.equal(g, cur), (i, t)
    signed = A.pitch_shift_chain([xs[0], xs[0], xs[1]], [-9.5, 6, -4], signed=True, formant=fm)
    for (i, t), g in zip([(0, -9.5), (0, 6), (1, -4)], signed):
        cur, lo = xs[i], 0
        for s in A.signed_chain(t):
            cur = A.pitch_shift([cur], s, formant=dataclasses.replace(fm, order=fm.node_order(lo)))[0]
            lo += s
        assert torch.equal(g, cur), (i, t)
    if track_pitch:                                                                # the orders matter: without them the upper links differ
        flat = A.pitch_shift_chain([xs[0]], [13], formant=dataclasses.replace(fm, track_pitch=False))[0]
        assert not torch.equal(flat, got[0])


# ---------------------------------------------------------------------------------------------------- 6. formant=None, wiring
def _tracks(max_notes=6):
    g = load_golden("arranger")
    name = "Ode_to_Joy_Easy_variation"
    msgs = [R.messages(g[f"{name}.t{k}.msgs"]) for k in range(2)]
    tmap = A.tempo_map_of(msgs)
    return [A.Track(t, int(g[name + ".tpb"]), max_notes, pairing="midi", tempo_map=tmap) for t in msgs]


def _notes(tracks, names, perform=None):
    return {(name, s[1]): torch.from_numpy(R.synthetic_note(s[1])).cuda() for name, t in zip(names, tracks) for s in t.schedule(perform=perform)}


def _counted(fn):
    """(fn(), {entry point: calls})."""
    counts, call = {}, L.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return call(name, *args)
    A.L.call = counting
    try:
        return fn(), counts
    finally:
        A.L.call = call


def test_formant_none_is_the_call_without_the_argument():
    sigs = [torch.from_numpy(s).cuda() for s in signals()]
    base, counts = _counted(lambda: A.pitch_shift(sigs, list(STEPS)))
    none, counts_none = _counted(lambda: A.pitch_shift(sigs, list(STEPS), formant=None))
    assert all(torch.equal(a, b) for a, b in zip(base, none)) and counts == counts_none and "ds_pv_formant" not in counts
    _, with_fm = _counted(lambda: A.pitch_shift(sigs, list(STEPS), formant=FM))
    assert with_fm == {**counts, "ds_pv_formant": 1}                               # one more entry point, nothing else changes
    x = sigs[3]
    assert torch.equal(A.pitch_shift_chain([x], [9])[0], A.pitch_shift_chain([x], [9], formant=None)[0])
    tracks, names = _tracks(), ["organ", "string"]
    fn = lambda v, d: R.synthetic_note(d)                                          # noqa: E731
    t = tracks[0]
    plain, counts = _counted(lambda: t.render(fn))
    assert torch.equal(t.render(fn, formant=None), plain) and "ds_pv_formant" not in counts
    got, with_fm = _counted(lambda: t.render(fn, formant=FM))
    assert not torch.equal(got, plain) and got.shape == plain.shape and torch.isfinite(got).all()
    assert with_fm["ds_pv_formant"] == counts["ds_pv_vocode"] == with_fm["ds_pv_vocode"]           # once per level
    for tune in (None, 50.5):                                                      # it composes: only the chains change
        for perform in (None, A.Performance()):
            mst = A.Mastering()
            one = t.render(fn, tune=tune, perform=perform, formant=FM)
            assert torch.equal(t.render(fn, tune=tune, perform=perform, formant=FM, master=mst), A.master(one, mst))
            assert not torch.equal(one, t.render(fn, tune=tune, perform=perform))
    for perform in (None, A.Performance()):
        notes = _notes(tracks, names, perform)
        ds = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi", perform=perform)
        base = ds.arrange(tracks, names, notes)
        assert torch.equal(ds.arrange(tracks, names, notes, formant=None), base)
        got = ds.arrange(tracks, names, notes, formant=FM)
        audios = [tr.render(None, notes={k: notes[(names[i], d)] for k, d, _, _ in tr.schedule(perform=perform)}, perform=perform, formant=FM)
                  for i, tr in enumerate(tracks)]
        want = torch.zeros(max(a.numel() for a in audios), device="cuda")
        for a in audios:
            want[:a.numel()] += a
        assert torch.equal(got, want) and not torch.equal(got, base)
        df = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi", perform=perform, formant=FM)      # the constructor's holds
        assert torch.equal(df.arrange(tracks, names, notes), got) and torch.equal(df.arrange(tracks, names, notes, formant=None), base)
        assert torch.equal(ds.arrange(tracks, names, notes, tune="detect", formant=None), ds.arrange(tracks, names, notes, tune="detect"))
        assert not torch.equal(ds.arrange(tracks, names, notes, tune="detect", formant=FM), ds.arrange(tracks, names, notes, tune="detect"))


# ---------------------------------------------------------------------------------------------------- 7. bounds
def test_nothing_is_written_outside_the_fitting_rows():
    """Row 1 is moved so that it ends behind total_out, row 2 has order 0, row 4 order 513: they read and write nothing, the other rows
    are what they are in the whole batch, and the padding behind voc stays untouched."""
    PV = L.PV
    total = sum(len(v) for v in vocs())

    def edit(tab):
        tab[1, PV["DS_PV_TOFF"]] = total - len(vocs()[1]) + 1                      # one frame too far

    got, pad = launch(vocs(), LENGTHS, STEPS, [30, 30, 0, 30, 513], pad=4 * NB * 2, edit=edit)
    assert len(pad) == 4 * NB * 2 and (pad == np.float32(-777.0)).all()
    for i in (0, 3):
        assert np.array_equal(bits(got[i]), bits(batch(30)[i])), i
    for i in (2, 4):                                                               # order outside [1, DS_PV_ORDER_MAX]: untouched, and row 4's
        assert np.array_equal(bits(got[i]), bits(cplx(vocs()[i]))), i             # frames are the ones the moved row 1 points at
    assert np.array_equal(bits(got[1]), bits(cplx(vocs()[1])))                     # the frames row 1 had: no row owns them now


# ---------------------------------------------------------------------------------------------------- 8. the property, on the device
def test_the_envelope_stays_twice_as_close_to_the_sources_on_the_device():
    y = F.probe()
    plain, formant = device_chains()
    a, b = F.shape_deviation(plain, y), F.shape_deviation(formant, y)
    print(f"chain +12 on the device: plain {a:.2f} dB rms, with correction {b:.2f} dB rms, ratio {b / a:.3f}")
    assert b <= 0.5 * a, (a, b)
