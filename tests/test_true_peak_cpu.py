"""CPU suite of the true-peak meter and limiter (diffusynth_amd.true_peak, Mastering(true_peak=)): the interpolator's table,
the restatement (tests/true_peak_ref.py) against a plain convolution and against the analytic fs/4 sine, what the fixtures can see, the
limiter's measured bound on the six signals of §7r, the refusals, the header."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import master_ref as M
import true_peak_ref as R
import diffusynth_amd
from conftest import ROOT
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

TM = importlib.import_module("diffusynth_amd.true_peak")         # (the package's attribute `true_peak` is the function)
TP, F32 = L.TP, np.float32
A0, R0 = M.samples(M.DEFAULTS["lookahead"], M.DEFAULTS["hold"])   # the defaults at 16 kHz: (80, 800)
C = F32(M.DEFAULTS["ceiling"])
BOUND_DB = 0.01                                                   # the condition of DESIGN §7r on the limiter's output, at the defaults


# ---------------------------------------------------------------------------------------------------- the table
def test_table_symmetries_zero_crossings_and_row_sums():
    h = diffusynth_amd.true_peak_coefficients()
    assert h is TM.true_peak_coefficients() and h.shape == (3, 12) and h.dtype == F32 and not h.flags.writeable and h.flags.c_contiguous
    assert np.array_equal(h, R.table())                                            # the restatement's own copy of the formula
    assert np.array_equal(h[2], h[0][::-1]) and np.array_equal(h[1], h[1][::-1])
    for k in range(-6, 7):
        if k:
            assert abs(R.tap(4 * k)) < 1e-15 and abs(TM.tap(4 * k)) < 1e-15
    assert R.tap(0) == 1.0 == TM.tap(0) and R.tap(25) == 0.0 == TM.tap(-25) and TM.tap(24) == 0.0
    for p in (1, 2, 3):                                                             # h[p][k] = c(4 (5 - k) + p)
        for k in range(12):
            assert h[p - 1, k] == F32(R.tap(4 * (5 - k) + p))
    sums = h.astype(np.float64).sum(axis=1)
    print("row sums", sums.tolist())
    assert np.allclose(sums, [1.00048, 1.00090, 1.00048], rtol=0, atol=5e-6)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_equals_the_convolution_of_the_zero_stuffed_signal():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 12, 13, 300):
        x = rng.standard_normal(n).astype(F32)
        o = R.oversampled(x)                                                       # index i is time -1 + i / 4
        v = R.phases(x)
        assert o.shape == (4 * n + 8,) and v.shape == (3, n + 1) and v.dtype == np.float64
        err = max(np.abs(o[p + 1:p + 1 + 4 * (n + 1):4] - v[p]).max() for p in range(3))
        ident = np.abs(o[4:4 + 4 * n:4] - x).max()
        print(f"N = {n}: phases against np.convolve {err:.3e}, identity phase {ident:.3e}")
        assert err <= 1e-12 and ident == 0.0
        # the envelope is the largest magnitude of that waveform at the seven instants i - 3/4 .. i + 3/4
        want = np.array([np.abs(o[4 * i + 1:4 * i + 8]).max() for i in range(n)]).astype(F32)      # times i - 3/4 .. i + 3/4
        assert np.allclose(R.envelope(x), want, rtol=1e-6, atol=0)


def test_quarter_rate_sine_reads_its_analytic_peak():
    t = np.arange(16000)
    x = np.sin(2 * np.pi * t / 4.0 + np.pi / 4.0).astype(F32)
    tp = R.true_peak(x)
    print(f"fs/4 sine at 45 degrees: sample peak {np.abs(x).max():.6f}, true peak {tp:.7f} = {R.db(tp):+.4f} dB")
    assert abs(float(np.abs(x).max()) - math.sqrt(0.5)) < 1e-6
    assert abs(R.db(tp)) <= 0.2
    assert abs(R.db(tp) - 0.1035) <= 1e-3                                           # the value DESIGN §7r records: the window's error at fs/4


def test_envelope_covers_the_samples_and_the_edges_are_zero_padded():
    rng = np.random.default_rng(4)
    x = rng.standard_normal(777).astype(F32)
    e = R.envelope(x)
    assert e.dtype == F32 and e.shape == x.shape and (e >= np.abs(x)).all() and R.true_peak(x) == e.max() and (e > np.abs(x)).any()
    h = R.table().astype(np.float64)
    for n in (1, 2, 30):
        # an impulse at sample j: the waveform at time j + d / 4 is c(d); zero padding adds nothing, so e[i] is the largest |c| at the
        # distances 4 (i - j) - 3 .. 4 (i - j) + 3, whether the impulse is the first or the last sample
        for j in (0, n - 1):
            x = np.zeros(n, F32)
            x[j] = 1.0
            c = np.abs(R.table_full())
            want = np.array([max(c[24 + d] if abs(d) <= 24 else 0.0 for d in range(4 * (i - j) - 3, 4 * (i - j) + 4)) for i in range(n)]).astype(F32)
            assert np.array_equal(R.envelope(x), want), (n, j)
            assert R.true_peak(x) == 1.0 and R.envelope(x)[j] == 1.0
    assert h[0, 5] == F32(R.tap(1)) and R.envelope(np.array([0.0, 1.0], F32))[0] == F32(R.tap(1))


DEFECT_FIXTURES = {"right_interval_only": "impulse_first", "edges_clamped": "dc_short", "half_sample_only": "third_phase", "fp32_accumulate": "noise"}


def defect_fixture(name):
    """impulse_first: the waveform right of an impulse belongs to its right neighbour's envelope too; dc_short: a constant has a large
    edge transient with zeros outside and none with the edge repeated; third_phase: an fs/4 sine whose peak sits a quarter sample off
    the grid; noise: rounding."""
    if name == "impulse_first":
        x = np.zeros(9, F32)
        x[0] = 1.0
        return x
    if name == "dc_short":
        return np.full(40, 0.5, F32)
    if name == "third_phase":
        t = np.arange(64)
        return np.sin(2 * np.pi * (t - 0.25) / 4.0 + np.pi / 2.0).astype(F32)       # peaks at t = 0.25 + 2 k: phase p = 1
    return np.random.default_rng(9).standard_normal(4096).astype(F32)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_model_moves_the_envelope_or_the_true_peak(defect):
    x = defect_fixture(DEFECT_FIXTURES[defect])
    e, tp = R.envelope(x), R.true_peak(x)
    be, btp = R.envelope(x, defect), R.true_peak(x, defect)
    moved = np.abs(be.astype(np.float64) - e).max()
    print(f"{defect} on {DEFECT_FIXTURES[defect]}: envelope moves by {moved:.3e} (in {np.count_nonzero(be != e)} samples), true peak {btp!r} against {tp!r}")
    if defect == "fp32_accumulate":
        assert np.count_nonzero(be != e) > 100                                      # rounding: a bit-for-bit comparison sees it, nothing coarser does
    else:
        assert moved > 1e-3 * float(tp)


# ---------------------------------------------------------------------------------------------------- the limiter's bound, measured
@pytest.fixture(scope="module")
def six():
    out = {}
    for name, x in R.fixtures().items():
        out[name] = (x, R.master(x, A0, R0, target_rms=None, ceiling=C), R.master(x, A0, R0, target_rms=None, ceiling=C, detector="samples"))
    return out


@pytest.mark.parametrize("name", list(R.fixtures()))
def test_limiter_holds_sample_peak_exactly_and_true_peak_within_the_condition(six, name):
    x, tp, sp = six[name]
    over, over_sp = R.db(tp["tp_out"] / float(C)), R.db(sp["tp_out"] / float(C))
    print(f"{name}: sample peak {np.abs(x).max():.4f}, true peak {tp['tp_in']:.4f}; output true peak {tp['tp_out'] / float(C):.6f} c = {over:+.5f} dB with the envelope, "
          f"{sp['tp_out'] / float(C):.4f} c = {over_sp:+.3f} dB with the samples; limited {tp['limited']} / {sp['limited']}")
    assert (A0, R0) == (80, 800) and np.abs(tp["y"]).max() <= C and np.abs(sp["y"]).max() <= C
    assert over <= BOUND_DB
    assert over_sp > 0.1                                                            # not vacuous: the sample-peak limiter leaves it over
    assert (tp["g"] <= tp["r"]).all() and tp["limited"] >= sp["limited"]


def test_without_lookahead_the_bound_does_not_hold(six):
    """The bound rests on the smoothing of the look-ahead (Mastering's docstring says so): with A = 0 the gain steps from sample to sample."""
    x = six["clipped_noise"][0]
    r = R.master(x, 0, 0, target_rms=None, ceiling=C)
    over = R.db(r["tp_out"] / float(C))
    print(f"clipped noise, A = R = 0: output true peak {r['tp_out'] / float(C):.4f} c = {over:+.3f} dB")
    assert np.abs(r["y"]).max() <= C and over > BOUND_DB and over > 1.0
    assert "look-ahead" in A.Mastering.__doc__ and "true_peak" in A.Mastering.__doc__


# ---------------------------------------------------------------------------------------------------- refusals, before any device work
def test_mastering_true_peak_refusals():
    assert A.Mastering().true_peak is False and A.Mastering(true_peak=True).true_peak is True and A.Mastering(true_peak=False) == A.Mastering()
    assert A.Mastering(target_rms=None, target_lufs=-14.0, true_peak=True).samples(16000) == (80, 800)
    assert A.Mastering(target_rms=None, true_peak=True).target_rms is None
    for bad in (None, 0, 1, 1.0, "True", "yes", math.nan, [True]):
        with pytest.raises(ValueError, match="Mastering.*true_peak"):
            A.Mastering(true_peak=bad)
    with pytest.raises(ValueError, match="Mastering.*ceiling"):
        A.Mastering(true_peak=True, ceiling=1.5)
    assert A.MasterStats._fields == ("gain", "rms", "peak", "min_gain", "limited")
    assert A.TruePeak is TM.TruePeak is diffusynth_amd.TruePeak and TM.TruePeak._fields == ("input", "output")


def test_true_peak_and_master_refuse_before_they_ask_for_a_device():
    x = torch.zeros(8000)                                                         # a CPU tensor: a valid call ends in the RuntimeError below
    f = diffusynth_amd.true_peak
    assert f is TM.true_peak and diffusynth_amd.true_peak_coefficients is TM.true_peak_coefficients
    with pytest.raises(ValueError, match="signals.*empty"):
        f([x, torch.zeros(0)])
    with pytest.raises(ValueError, match="signals.*empty"):
        f(torch.zeros(2, 0))
    with pytest.raises(ValueError, match=r"signals.*2\^24"):
        f(torch.zeros(2 ** 24 + 1))
    for bad in ([], torch.zeros(2, 3, 4), [torch.zeros(2, 3)], 5, [x, "x"], None):
        with pytest.raises(ValueError, match="true_peak: signals"):
            f(bad)
    for bad in (None, 1, "yes"):
        with pytest.raises(ValueError, match="return_envelope"):
            f(x, return_envelope=bad)
    with pytest.raises(TypeError):
        f(x, True)                                                                 # keyword only
    for sig in (x, torch.zeros(2, 500), [x, x[:300]]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(sig)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(sig, return_envelope=True)
    m = A.Mastering(true_peak=True)
    for bad in (None, 1, "yes"):
        with pytest.raises(ValueError, match="return_true_peak"):
            A.master(x, m, return_true_peak=bad)
    with pytest.raises(ValueError, match="signals.*empty"):
        A.master([x, torch.zeros(0)], m, return_true_peak=True)
    with pytest.raises(ValueError, match="sample_rate"):
        A.master(x, A.Mastering(target_rms=None, target_lufs=-16.0, true_peak=True), sample_rate=4000)
    with pytest.raises(ValueError, match="lookahead"):
        A.master(x, A.Mastering(true_peak=True, lookahead=1.0, hold=1.0))
    for mm in (m, A.Mastering()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            A.master(x, mm, return_true_peak=True)
    t = A.Track([], 480)
    assert t.last_true_peak is None
    with pytest.raises(ValueError, match="lookahead"):
        t.render(None, master=A.Mastering(true_peak=True, lookahead=1.0, hold=1.0))
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda", master=m)
    assert ds.master == m and ds.last_true_peak is None and ds.last_master is None


# ---------------------------------------------------------------------------------------------------- header, binding, entry points
def test_header_defines_binding_and_exports():
    assert TP == {"DS_TP_TILE": 2048, "DS_TP_PHASES": 3, "DS_TP_TAPS": 12, "DS_TP_NCOEF": 36}
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = f.read()
    assert TP == {k: int(v) for k, v in re.findall(r"^#define\s+(DS_TP_\w+)\s+(\d+)\s*$", text, flags=re.M)}
    assert TP["DS_TP_PHASES"] * TP["DS_TP_TAPS"] == TP["DS_TP_NCOEF"] and TP["DS_TP_TILE"] % 256 == 0
    assert 4 * (TP["DS_TP_TILE"] + 12) + 4 * (TP["DS_TP_TILE"] + 1) <= 64 * 1024     # the two tiles in LDS
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = L.load()
    for name in ("ds_true_peak_ws_bytes", "ds_true_peak", "ds_master_limit_tp"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    assert lib.ds_abi_version() == 1
    with open(os.path.join(ROOT, "DESIGN.md")) as f:                               # the same definition in both places
        design = f.read()
    for phrase in ("c(d) = sinc(d / 4) (1 + cos(2 pi d / 48)) / 2", "h[p][k] = fp32(c(4 (5 - k) + p))", "e[n] = fp32(max(|x[n]|, iv(n - 1), iv(n)))"):
        assert phrase in text and phrase in design, phrase
    ws = lib.ds_true_peak_ws_bytes                                                 # one fp32 per tile of the longest signal, per signal
    T = TP["DS_TP_TILE"]
    assert [ws(1, 1), ws(1, T), ws(1, T + 1), ws(3, 960000), ws(2, 2 ** 24), ws(0, 5), ws(1, 0), ws(1, 2 ** 24 + 1), ws(-1, 5)] == \
        [4, 4, 8, 3 * 469 * 4, 2 * 8192 * 4, 0, 0, 0, 0]


def test_entries_validate_before_any_gpu_work():
    lib = L.load()
    buf = (ctypes.c_double * 256)()
    p, q = ctypes.addressof(buf), ctypes.addressof(buf) + 512
    coef = np.ascontiguousarray(TM.true_peak_coefficients())
    args = (("x", p), ("tab", p), ("n", 1), ("ml", 8000), ("ts", 8000), ("coef", coef.ctypes.data), ("env", q), ("ws", p), ("tp", p), ("st", None))
    meter = lambda **kw: lib.ds_true_peak(*[kw.get(k, v) for k, v in args])        # noqa: E731
    bad = coef.copy()
    bad[1, 7] = math.nan
    inf = coef.copy()
    inf[2, 0] = math.inf
    for kw in ({"x": None}, {"tab": None}, {"coef": None}, {"ws": None}, {"tp": None}, {"n": 0}, {"n": 65536}, {"ml": 0}, {"ml": 2 ** 24 + 1}, {"ts": 0},
               {"ts": (1 << 31) - TP["DS_TP_TILE"]}, {"env": p}, {"coef": bad.ctypes.data}, {"coef": inf.ctypes.data}):
        assert meter(**kw) == -1, kw
        assert b"true_peak" in lib.ds_last_error_string(), kw
    for kw in ({"x": p + 2}, {"tab": p + 1}, {"env": q + 2}, {"ws": p + 2}, {"tp": p + 3}):
        assert meter(**kw) == -3, kw
    largs = (("x", p), ("env", q), ("tab", p), ("n", 1), ("ml", 8000), ("ts", 8000), ("c", 0.5), ("a", 80), ("r", 800), ("stats", p), ("lim", p), ("out", q + 512),
             ("pcm", None), ("st", None))
    limit = lambda **kw: lib.ds_master_limit_tp(*[kw.get(k, v) for k, v in largs])  # noqa: E731
    for kw in ({"x": None}, {"env": None}, {"tab": None}, {"stats": None}, {"lim": None}, {"out": None}, {"n": 0}, {"n": 65536}, {"ml": 0}, {"ml": 2 ** 24 + 1},
               {"ts": 0}, {"ts": 1 << 31}, {"c": 0.0}, {"c": 1.5}, {"c": math.nan}, {"a": -1}, {"a": 1025, "r": 2000}, {"a": 80, "r": 79}, {"r": 8193},
               {"out": p}, {"out": q}):
        assert limit(**kw) == -1, kw
        assert b"master_limit_tp" in lib.ds_last_error_string(), kw
    for kw in ({"x": p + 2}, {"env": q + 2}, {"out": q + 514}, {"pcm": p + 1}):
        assert limit(**kw) == -3, kw
    # the old entry point keeps its name in its messages
    assert lib.ds_master_limit(p, p, 1, 8000, 8000, 0.5, 80, 800, p, p, p, None, None) == -1 and b"master_limit: out may not be x" in lib.ds_last_error_string()
