"""CPU suite of the formant-preserving pitch shift: Formant's validation, the per-node orders on both trees, the plan's upload with and
without a Formant, the C entry without a device, the restatement (tests/formant_ref.py) at rate 1, and the property that justifies the
mode: on a two-formant note the spectral envelope of a shifted note stays at least twice as close to the source's as the plain shift's."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import arranger_ref as R
import formant_ref as F
from conftest import ROOT
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A


# ---------------------------------------------------------------------------------------------------- Formant
def test_formant_defaults_and_validation():
    import diffusynth_amd
    assert diffusynth_amd.Formant is A.Formant
    f = A.Formant()
    assert (f.order, f.max_gain_db, f.track_pitch) == (30, 24.0, True)
    assert f.limit == float(np.float32(24.0 * math.log(10.0) / 20.0))
    with pytest.raises(dataclasses_error()):
        f.order = 3                                                                # frozen
    with pytest.raises(TypeError):
        A.Formant(30)                                                              # keyword-only, as Mastering
    assert L.PV["DS_PV_ORDER_MAX"] == 512 and L.PV["DS_PV_GAIN_DB_MAX"] == 60 and L.PV["DS_PV_NI"] == 9
    for ok in (dict(order=1), dict(order=512), dict(order=np.int64(7)), dict(max_gain_db=60), dict(max_gain_db=1e-3), dict(track_pitch=False)):
        A.Formant(**ok)
    for bad in (dict(order=0), dict(order=513), dict(order=30.0), dict(order=True), dict(order=None), dict(order=-4),
                dict(max_gain_db=0), dict(max_gain_db=-3.0), dict(max_gain_db=60.001), dict(max_gain_db=float("nan")), dict(max_gain_db=float("inf")),
                dict(max_gain_db="24"), dict(max_gain_db=True), dict(track_pitch=1), dict(track_pitch=None)):
        with pytest.raises(ValueError, match="Formant"):
            A.Formant(**bad)


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_public_calls_refuse_a_wrong_formant_before_any_device_work():
    """ValueError, not the no-GPU RuntimeError these calls give on CPU tensors: the check comes first."""
    x = torch.zeros(5000)
    for bad in (30, "on", {"order": 30}, True):
        with pytest.raises(ValueError, match="formant"):
            A.pitch_shift([x], 2, formant=bad)
        with pytest.raises(ValueError, match="formant"):
            A.pitch_shift_chain([x], [5], formant=bad)
        with pytest.raises(ValueError, match="formant"):
            A.pitch_shift_librosa(x, 16000, 5, formant=bad)
        with pytest.raises(ValueError, match="formant"):
            A.DiffSynth({}, None, None, None, None, None, "cuda", formant=bad)
        with pytest.raises(ValueError, match="formant"):
            A.DiffSynth({}, None, None, None, None, None, "cuda").arrange([], [], {}, formant=bad)
        with pytest.raises(ValueError, match="formant"):
            A.Track([], 480).render(None, formant=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # a good one goes on to the device check
        A.pitch_shift([x], 2, formant=A.Formant())
    assert A.DiffSynth({}, None, None, None, None, None, "cuda", formant=A.Formant(order=20)).formant.order == 20


class _Mid:
    ticks_per_beat = 480
    tracks = [[], []]


def test_the_keyword_overrides_the_constructors_formant_all_the_way_down(monkeypatch):
    """get_music -> arrange -> Track.render: each hands on what it resolved, so an explicit None switches a constructor's Formant off
    (and a Formant switches a constructor's None on) for that one call; without the keyword the constructor's holds."""
    fm, other = A.Formant(), A.Formant(order=12)
    seen = []

    def render(self, note_fn, sample_rate=16000, return_tensor=True, notes=None, **kw):
        seen.append(kw["formant"])
        return torch.zeros(3)
    monkeypatch.setattr(A.Track, "render", render)
    tracks = [A.Track([], 480), A.Track([], 480)]
    for built, kw, want in ((fm, {}, fm), (fm, {"formant": None}, None), (fm, {"formant": other}, other), (None, {}, None), (None, {"formant": fm}, fm)):
        ds = A.DiffSynth({}, None, None, None, None, None, "cpu", formant=built)
        del seen[:]
        ds.arrange(tracks, ["organ", "string"], {}, **kw)
        assert seen == [want, want], (built, kw)
        del seen[:]
        ds.get_music(_Mid(), ["organ", "string"], return_tensor=True, **kw)     # no events: nothing to sample, arrange runs all the same
        assert seen == [want, want], (built, kw)
    got = {}
    monkeypatch.setattr(A.DiffSynth, "arrange", lambda self, *a, **kw: got.update(kw) or torch.zeros(3))
    A.DiffSynth({}, None, None, None, None, None, "cpu", formant=fm).get_music(_Mid(), ["organ", "string"], formant=None)
    assert "formant" in got and got["formant"] is None                              # arrange is TOLD None, not left to its default


# ---------------------------------------------------------------------------------------------------- per-node orders
def test_node_orders_follow_the_cumulative_shift_a_node_is_entered_at():
    f = A.Formant()
    assert [f.node_order(lo) for lo in (0, 4, 8, 12, 24, 28)] == [30, 23, 18, 15, 7, 5]          # floor(30 * 2^(-lo / 12))
    assert [f.node_order(lo) for lo in (-4, -8, -0.5)] == [30, 30, 30]                           # a downward chain keeps the order
    assert A.Formant(order=30).node_order(48) == 4 and A.Formant(order=6).node_order(12) == 4    # never below 4
    assert [A.Formant(order=30, track_pitch=False).node_order(lo) for lo in (0, 12, 48, -8)] == [30] * 4
    for lo in (0, 4, 5.5, 12, 31, -7):
        assert f.node_order(lo) == F.node_order(30, lo) and 1 <= f.node_order(lo) <= 512         # the restatement's rule


def test_orders_on_the_trees_with_and_without_track_pitch():
    reqs = [("a", 31), ("a", 5), ("b", 8), ("a", 8), ("b", 1), ("a", -2), ("b", 12), ("a", 4)]
    levels = A.shift_tree(reqs)
    f, flat = A.Formant(), A.Formant(track_pitch=False)
    seen = {}
    for i, nodes in enumerate(levels):
        orders = A.node_orders(nodes, f)
        assert orders == [max(4, math.floor(30 * 2.0 ** (-4 * i / 12))) for _ in nodes]          # level i is entered at 4 i semitones
        assert A.node_orders(nodes, flat) == [30] * len(nodes)
        for (k, lo, cum, _), o in zip(nodes, orders):
            assert (k, cum) not in seen                                            # (key, cumulative) still names its node: the sharing is unchanged
            seen[(k, cum)] = o
    assert sum(len(lv) for lv in levels) == len(seen) == 9 + 4
    signed = A.signed_tree([("a", 9.5), ("a", -9.5), ("a", 4), ("b", -4), ("b", 0.01), ("a", 8)])
    got = {(k, cum): o for nodes in signed for (k, lo, cum, _), o in zip(nodes, A.node_orders(nodes, f))}
    assert got == {("a", 4): 30, ("a", 8): 23, ("a", 9.5): 18, ("a", -4): 30, ("a", -8): 30, ("a", -9.5): 30, ("b", -4): 30}


# ---------------------------------------------------------------------------------------------------- the plan
def _todays_buffer(lengths, steps):
    """[rates | tab | step_idx | step_alpha] as the plan packed it before the formant mode existed, from the restatement's pieces."""
    rates, tab, idx, alpha = [], [], [], []
    xoff = foff = toff = soff = 0
    for ln, st in zip(lengths, steps):
        rate = R.rate_of(st)
        nf = 1 + ln // R.HOP
        i0, al = R.time_steps(nf, rate)
        slen = R.stretched_length(ln, rate)
        tab.append((xoff, ln, foff, nf, toff, len(i0), soff, slen, R.resampled_length(slen, rate)))
        rates.append(rate)
        idx.append(i0.astype(np.int32))
        alpha.append(al.astype(np.float32))
        xoff, foff, toff, soff = xoff + ln, foff + nf, toff + len(i0), soff + slen
    return np.concatenate([np.array(rates, np.float64).view(np.int32), np.array(tab, np.int32).reshape(-1), np.concatenate(idx),
                           np.concatenate(alpha).view(np.int32)])


def test_plan_without_a_formant_is_todays_buffer_and_with_one_appends_order_and_warp():
    lengths, steps = [30001, 4097, 1023, 28416, 4097], [4, -3, 0.5, 0, 4]
    want = _todays_buffer(lengths, steps)
    p = A._Plan(lengths, steps)
    assert p.host.dtype == np.int32 and p.host.tobytes() == want.tobytes() and not hasattr(p, "o_order")
    assert A._Plan(lengths, steps, None).host.tobytes() == want.tobytes()
    orders = [30, 7, 512, 4, 23]
    q = A._Plan(lengths, steps, orders)
    n = len(lengths)
    assert q.host[:want.size].tobytes() == want.tobytes() and q.host.size == want.size + 2 * n     # appended, nothing moved
    assert (q.o_order, q.o_warp) == (want.size, want.size + n)
    assert q.host[q.o_order:q.o_order + n].tolist() == orders
    warp = q.host[q.o_warp:q.o_warp + n].view(np.float32)
    assert warp.tolist() == [float(F.warp_of(R.rate_of(s))) for s in steps] and warp[3] == 1.0    # fl32(1 / rate): 1 exactly at rate 1
    assert (q.o_tab, q.o_idx, q.o_alpha, q.total_out, q.max_out) == (p.o_tab, p.o_idx, p.o_alpha, p.total_out, p.max_out)
    with pytest.raises(ValueError, match="orders"):
        A._Plan(lengths, steps, [30, 30])


# ---------------------------------------------------------------------------------------------------- C ABI without a device
def test_entry_is_declared_and_validates_before_any_gpu_work():
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = L.load()
    assert "ds_pv_formant" in set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", text)) and "ds_pv_formant" in L.EXPORTS and hasattr(lib, "ds_pv_formant")
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    lim = A.Formant().limit
    for fn in (lambda: lib.ds_pv_formant(None, p, p, p, lim, 1, 4, 4, None), lambda: lib.ds_pv_formant(p, p, None, p, lim, 1, 4, 4, None),
               lambda: lib.ds_pv_formant(p, p, p, None, lim, 1, 4, 4, None), lambda: lib.ds_pv_formant(p, p, p, p, lim, 0, 4, 4, None),
               lambda: lib.ds_pv_formant(p, p, p, p, lim, 1, 0, 4, None), lambda: lib.ds_pv_formant(p, p, p, p, lim, 1, 4, 0, None),
               lambda: lib.ds_pv_formant(p, p, p, p, lim, 1, 4, 1 << 21, None), lambda: lib.ds_pv_formant(p, p, p, p, lim, 65536, 4, 4, None),
               lambda: lib.ds_pv_formant(p, p, p, p, 0.0, 1, 4, 4, None), lambda: lib.ds_pv_formant(p, p, p, p, -1.0, 1, 4, 4, None),
               lambda: lib.ds_pv_formant(p, p, p, p, float("nan"), 1, 4, 4, None), lambda: lib.ds_pv_formant(p, p, p, p, 7.0, 1, 4, 4, None)):
        assert fn() == -1 and b"pv_formant" in lib.ds_last_error_string(), lib.ds_last_error_string()
    assert lib.ds_pv_formant(p + 4, p, p, p, lim, 1, 4, 4, None) == -3 and b"pv_formant" in lib.ds_last_error_string()
    assert lib.ds_pv_formant(p, p, p + 2, p, lim, 1, 4, 4, None) == -3
    assert A.Formant(max_gain_db=60).limit <= 60 * math.log(10.0) / 20 * (1 + 1e-6)          # the largest limit the package hands over passes


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_at_rate_one_returns_its_input_bit_for_bit():
    V = R.phase_vocoder(R.stft(R.probe_signal(9000, seed=2)), 1.0)
    V[2, 100:140] = 0                                                              # bins at the floor
    for order in (30, 4, 512):
        assert np.array_equal(F.correct(V, 1.0, order, 24.0), V)
        v32 = V.astype(np.complex64)
        got = F.correct(v32, 1.0, order, 24.0, np.float32)
        assert got.dtype == np.complex64 and np.array_equal(got, v32)
    y = R.probe_signal(9000, seed=2)
    assert np.array_equal(F.pitch_shift_formant(y, 0, 30, 24.0), R.pitch_shift(y, 0))


def test_restatement_smoothing_is_a_projection_and_the_twin_is_close():
    y = R.probe_signal(12000, seed=4)
    mag = np.abs(R.stft(y))
    Lg, S = F.smooth_log(mag, 30)
    _, S2 = F.smooth_log(np.exp(S), 30)                                            # smoothing a smooth envelope changes nothing
    assert np.abs(S2 - S).max() < 1e-9
    _, Sfull = F.smooth_log(mag, 2048)                                             # every coefficient kept: the log magnitude itself
    assert np.abs(Sfull - Lg).max() < 1e-9
    V = R.phase_vocoder(R.stft(y), R.rate_of(4))
    info = {}
    want, twin = F.correct(V, R.rate_of(4), 30, 24.0, info=info), F.correct(V.astype(np.complex64), R.rate_of(4), 30, 24.0, np.float32)
    err = np.abs(twin - want).max() / np.abs(want).max()
    print(f"twin against float64: {err:.2e}, max|L| {info['max_abs_L']:.2f}")
    assert err < 1e-4 and 0 < info["max_abs_L"] <= -math.log(1e-6) + 20
    lim = 3.0 * math.log(10.0) / 20.0                                              # the clamp holds bin by bin
    g = np.abs(F.correct(V, R.rate_of(4), 30, 3.0)) / np.maximum(np.abs(V), 1e-300)
    assert g[np.abs(V) > 0].max() <= math.exp(lim) * (1 + 1e-12) and g[np.abs(V) > 0].min() >= math.exp(-lim) * (1 - 1e-12)


# ---------------------------------------------------------------------------------------------------- the property
@functools.lru_cache(maxsize=None)
def _probe():
    return F.probe()


CASES = {"+4": (lambda y: R.pitch_shift(y, 4), lambda y: F.pitch_shift_formant(y, 4, 30, 24.0)),
         "chain +12": (lambda y: R.pitch_shift_chain(y, 12), lambda y: F.pitch_shift_chain_formant(y, 12, 30, 24.0, track_pitch=True)),
         "-4": (lambda y: R.pitch_shift(y, -4), lambda y: F.pitch_shift_formant(y, -4, 30, 24.0))}


@pytest.mark.parametrize("case", list(CASES))
def test_the_envelope_stays_twice_as_close_to_the_sources(case):
    """Measured with the float64 restatement: +4: 13.0 -> 5.0 dB rms (0.38), chain +12: 16.7 -> 4.9 (0.29), -4: 11.6 -> 1.3 (0.11)."""
    y = _probe()
    assert len(y) == 28416 and y.dtype == np.float32 and abs(np.abs(y).max() - 1.0) < 0.05
    plain, formant = CASES[case]
    a, b = F.shape_deviation(plain(y), y), F.shape_deviation(formant(y), y)
    print(f"{case}: plain {a:.2f} dB rms, with correction {b:.2f} dB rms, ratio {b / a:.3f}")
    assert b <= 0.5 * a, (case, a, b)
