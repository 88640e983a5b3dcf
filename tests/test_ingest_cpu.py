"""The ingest path without a device: the restatement (tests/ingest_ref.py) pinned to scipy, the package's host filter design and table
builder against the restatement, the refusals and the width / length formula."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ingest_ref as R
from conftest import ROOT
from diffusynth_amd import _lib as L
from diffusynth_amd import ingest as G

PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (32000, 16000), (16000, 48000), (16000, 44100)]
LENGTHS = [1, 2, 441, 2999]
RP = L.RP


def rel(a, b):
    """max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


# ---------------------------------------------------------------------------------------------------- the restatement against scipy
@pytest.mark.parametrize("orig,target", PAIRS, ids=[f"{a}to{b}" for a, b in PAIRS])
def test_restatement_equals_scipy_resample_poly(orig, target):
    signal = pytest.importorskip("scipy.signal")
    up, down, half = R.rate_pair(orig, target)
    for n in LENGTHS:
        x = R.probe_signal(n, seed=n).astype(np.float64)
        want = signal.resample_poly(x, up, down)
        got = R.resample(x, up, down)
        assert got.shape == want.shape == (R.resampled_length(n, up, down),)
        err = rel(got, want)
        print(f"{orig} -> {target} ({up}/{down}), N = {n}: {err:.2e}")
        assert err < 1e-12, (orig, target, n, err)


@pytest.mark.parametrize("orig,target", PAIRS, ids=[f"{a}to{b}" for a, b in PAIRS])
def test_restated_filter_equals_scipy_firwin(orig, target):
    signal = pytest.importorskip("scipy.signal")
    up, down, half = R.rate_pair(orig, target)
    want = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    err = rel(R.design_filter(up, down), want)
    print(f"{orig} -> {target}: {2 * half + 1} taps, {err:.2e}")
    assert err < 1e-12, (orig, target, err)


def test_the_largest_usual_filter_is_11025_to_16000():
    rates = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)
    taps = {(a, 16000): 2 * R.rate_pair(a, 16000)[2] + 1 for a in rates if a != 16000}
    taps.update({(16000, b): 2 * R.rate_pair(16000, b)[2] + 1 for b in rates if b != 16000})
    assert max(taps.values()) == taps[(11025, 16000)] == 12801 <= G.MAX_TAPS == 16384
    for pair in taps:
        assert G.rate_pair(*pair) == R.rate_pair(*pair)


# ---------------------------------------------------------------------------------------------------- the package's filter design
@pytest.mark.parametrize("orig,target", PAIRS, ids=[f"{a}to{b}" for a, b in PAIRS])
def test_package_filter_equals_the_restatement(orig, target):
    up, down, half = G.rate_pair(orig, target)
    assert (up, down, half) == R.rate_pair(orig, target)
    want = R.design_filter(up, down)
    got = G.design_filter(up, down)
    assert got.dtype == np.float64 and rel(got, want) < 1e-12
    bank = G.FilterBank()
    taps = bank.taps(up, down)
    w32 = want.astype(np.float32)
    assert taps.dtype == np.float32 and taps.shape == w32.shape
    ulp = np.spacing(np.abs(w32))
    assert np.all(np.abs(taps.astype(np.float64) - w32.astype(np.float64)) <= ulp)      # equal to 1 ulp
    assert abs(float(want.sum()) - up) < 1e-9 * up                                         # unit gain at DC after the zero stuffing


# ---------------------------------------------------------------------------------------------------- the table builder
def test_plan_tables():
    bank = G.FilterBank()
    lengths = [441, 1000, 300, 2999, 7, 882]
    srs = [44100, 48000, 16000, 44100, 16000, 22050]
    p = G._Plan(lengths, srs, 16000, None, bank)
    assert p.rows == [0, 1, 3, 5] and p.same == [2, 4]                          # equal rates stay out of the launch
    assert p.nres == [160, 334, 300, 1089, 7, 640] == p.olen                   # ceil(N up / down); lengths=None: as it comes
    assert p.ooff == [0, 160, 494, 794, 1883, 1890] and p.total_out == 2530
    t = p.tab
    assert t.dtype == np.int32 and t.shape == (4, RP["DS_RP_NI"])
    assert t[:, RP["DS_RP_XOFF"]].tolist() == [0, 441, 1441, 4440] and p.total_in == 5322          # only the launched signals are packed
    assert t[:, RP["DS_RP_LEN"]].tolist() == [441, 1000, 2999, 882]
    assert t[:, RP["DS_RP_OOFF"]].tolist() == [0, 160, 794, 1890]
    assert t[:, RP["DS_RP_OLEN"]].tolist() == t[:, RP["DS_RP_NRES"]].tolist() == [160, 334, 1089, 640]
    assert t[:, RP["DS_RP_UP"]].tolist() == [160, 1, 160, 320] and t[:, RP["DS_RP_DOWN"]].tolist() == [441, 3, 441, 441]
    assert t[:, RP["DS_RP_HALF"]].tolist() == [4410, 30, 4410, 4410]
    # one filter per distinct pair, shared between rows 0 and 2
    assert t[:, RP["DS_RP_HOFF"]].tolist() == [0, 8821, 0, 8821 + 61] and bank.total == 8821 + 61 + 8821 and len(bank.offsets) == 3
    assert np.array_equal(bank.host()[8821:8821 + 61], G.design_filter(1, 3).astype(np.float32))
    assert p.max_taps == 8821 and p.max_blocks == 2                             # 1089 outputs in blocks of 1024
    for row in t:
        blk, up, down, half = (int(row[RP[k]]) for k in ("DS_RP_BLK", "DS_RP_UP", "DS_RP_DOWN", "DS_RP_HALF"))
        assert 1 <= blk <= G.MAX_BLK and ((blk - 1) * down + 2 * half) // up + 2 <= p.span <= G.MAX_SPAN
    # fix_length targets: longer and shorter than NRES, one value and one per signal
    q = G._Plan(lengths, srs, 16000, [200, 100, 400, 1089, 3, 0], bank)
    assert q.olen == [200, 100, 400, 1089, 3, 0] and q.nres == p.nres and q.rows == [0, 1, 3] and q.total_out == 1792     # a zero-length output is not launched
    assert q.tab[:, RP["DS_RP_OLEN"]].tolist() == [200, 100, 1089] and q.tab[:, RP["DS_RP_NRES"]].tolist() == [160, 334, 1089]
    assert G._Plan(lengths, 44100, 16000, 65280, bank).olen == [65280] * 6 and len(bank.offsets) == 3                      # the bank is reused
    # dense: the input buffer holds every signal (uploads_to_stft normalises all of them into one buffer)
    d = G._Plan(lengths, srs, 16000, 100, bank, dense=True)
    assert d.rows == [0, 1, 3, 5] and d.tab[:, RP["DS_RP_XOFF"]].tolist() == [0, 441, 1741, 4747] and d.total_in == sum(lengths)
    assert d.tab[:, RP["DS_RP_OOFF"]].tolist() == [0, 100, 300, 500] and d.total_out == 600
    # one rate pair per signal, target rates included
    o = G._Plan([100, 100], [16000, 8000], [48000, 16000], None, bank)
    assert o.tab[:, RP["DS_RP_UP"]].tolist() == [3, 2] and o.tab[:, RP["DS_RP_DOWN"]].tolist() == [1, 1] and o.nres == [300, 200]


def test_block_outputs_fit_the_span_for_every_ratio():
    for up, down in [(160, 441), (1, 3), (2, 1), (640, 441), (3, 1), (147, 160), (1, 12), (1, 819), (819, 1), (6, 1), (1, 6), (80, 441)]:
        half = 10 * max(up, down)
        assert 2 * half + 1 <= G.MAX_TAPS
        blk, span = G.block_outputs(up, down, half)
        assert 1 <= blk <= G.MAX_BLK and span <= G.MAX_SPAN
        for m0 in (0, blk, 7 * blk):                                                     # the true span of a block, by the definition
            lo = max(0, -((half - m0 * down) // up))
            hi = (half + (m0 + blk - 1) * down) // up
            assert hi - lo + 1 <= span, (up, down, m0)
    assert G.block_outputs(160, 441, 4410) == (1024, 2876)             # (1023 * 441 + 8820) // 160 + 2


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    bank = G.FilterBank()
    with pytest.raises(ValueError, match=r"15999 Hz -> 16000 Hz.*16384"):
        G.rate_pair(15999, 16000)
    with pytest.raises(ValueError, match=r"15999 Hz -> 16000 Hz.*16384"):
        G._Plan([100], 15999, 16000, None, bank)
    for bad in (0, -44100, 44100.0, "44100", True, None):
        with pytest.raises(ValueError, match="positive int"):
            G._Plan([100], bad if not isinstance(bad, str) and bad is not None else [bad], 16000, None, bank)
        with pytest.raises(ValueError, match="positive int"):
            G.rate_pair(44100, bad)
    with pytest.raises(ValueError, match="empty signal"):
        G._Plan([100, 0], 44100, 16000, None, bank)
    with pytest.raises(ValueError, match="2 values for 3 signals"):
        G._Plan([100, 100, 100], [44100, 48000], 16000, None, bank)
    with pytest.raises(ValueError, match="2 values for 3 signals"):
        G._Plan([100, 100, 100], 44100, 16000, [5, 6], bank)
    with pytest.raises(ValueError, match="non-negative int"):
        G._Plan([100], 44100, 16000, -1, bank)
    with pytest.raises(ValueError, match="non-negative int"):
        G._Plan([100], 44100, 16000, 10.5, bank)
    assert not bank.offsets or set(bank.offsets) == {(160, 441)}
    # stereo, an empty upload and bad rates are refused before anything touches a device
    stereo = np.zeros((1000, 2), np.int16)
    with pytest.raises(ValueError, match="mono"):
        G.uploads_to_stft([(44100, stereo)], 3)
    with pytest.raises(ValueError, match="mono"):
        G.uploads_to_stft([(16000, np.zeros(100, np.float32)), (44100, torch.zeros(2, 1000))], 3)
    with pytest.raises(ValueError, match="empty"):
        G.uploads_to_stft([(44100, np.zeros(0, np.int16))], 3)
    with pytest.raises(ValueError, match="positive int"):
        G.uploads_to_stft([(44100.0, np.zeros(10, np.int16))], 3)
    with pytest.raises(ValueError, match="15999"):
        G.uploads_to_stft([(15999, np.zeros(10, np.int16))], 3)
    with pytest.raises(ValueError, match="no uploads"):
        G.uploads_to_stft([], 3)


def test_cpu_tensors_raise_no_cpu_fallback():
    x = torch.zeros(2, 500)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.resample_poly(x, 44100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.resample_poly([x[0], x[1, :300]], [44100, 48000], 16000, lengths=100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.adjust_audio_length(x[0], 100, 44100, 16000)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            G.uploads_to_stft([(44100, np.ones(100, np.int16))], 3)


# ---------------------------------------------------------------------------------------------------- width and length
def test_width_and_length_formula():
    assert (G.upload_width(3), G.upload_length(3)) == (64, 65280) == (R.upload_width(3), R.upload_length(3))
    assert (G.upload_width(1, 48), G.upload_length(1, 48)) == (6, 5888) == (R.upload_width(1, 48), R.upload_length(1, 48))
    assert (G.upload_width(2.2, 48), G.upload_length(2.2, 48)) == (9, 8960) == (R.upload_width(2.2, 48), R.upload_length(2.2, 48))


def test_restated_ingest_normalises_resamples_and_fits():
    up16 = (np.arange(13230) % 200 - 100).astype(np.int16) * 150
    ups = [(44100, up16), (16000, R.probe_signal(5000, 3))]
    a = R.ingest(ups, 1, time_resolution=48)
    assert a.shape == (2, 5888) and a.dtype == np.float64
    n0 = R.resampled_length(13230, 160, 441)
    assert n0 == 4800 and not a[0, n0:].any() and np.array_equal(a[0, :n0], R.resample(up16.astype(np.float64) / 15000.0, 160, 441))
    x1 = ups[1][1].astype(np.float64)
    assert np.array_equal(a[1, :5000], x1 / np.abs(x1).max()) and not a[1, 5000:].any()      # equal rates: normalised, padded, untouched
    twin = R.ingest(ups, 1, time_resolution=48, dtype=np.float32)
    assert twin.dtype == np.float32 and 0 < rel(twin, a) < 1e-5


# ---------------------------------------------------------------------------------------------------- header, binding, entry point
def test_header_and_binding_declare_the_entry():
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", text))
    lib = L.load()
    assert "ds_resample_poly" in declared and "ds_resample_poly" in L.EXPORTS and hasattr(lib, "ds_resample_poly")
    assert L.RP == {"DS_RP_XOFF": 0, "DS_RP_LEN": 1, "DS_RP_OOFF": 2, "DS_RP_OLEN": 3, "DS_RP_NRES": 4, "DS_RP_UP": 5, "DS_RP_DOWN": 6, "DS_RP_HALF": 7,
                    "DS_RP_HOFF": 8, "DS_RP_BLK": 9, "DS_RP_NI": 10, "DS_RP_MAX_TAPS": 16384, "DS_RP_MAX_SPAN": 20480, "DS_RP_MAX_BLK": 1024}
    assert (G.MAX_TAPS + G.MAX_SPAN) * 4 <= 160 * 1024                           # filter + span fit a CU's LDS


def test_entry_validates_before_any_gpu_work():
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    call = lambda **kw: lib.ds_resample_poly(*[kw.get(k, v) for k, v in (("x", p), ("tab", p), ("filt", p), ("n", 1), ("mb", 1), ("taps", 8821), ("span", 4096),    # noqa: E731
                                                                        ("ti", 1000), ("to", 400), ("tf", 8821), ("out", p), ("st", None))])
    for kw in ({"x": None}, {"tab": None}, {"filt": None}, {"out": None}, {"n": 0}, {"n": 65536}, {"mb": 0}, {"taps": 2}, {"taps": 16385}, {"span": 0},
               {"span": 20481}, {"ti": 0}, {"to": 0}, {"tf": 0}, {"ti": 1 << 31}, {"to": (1 << 31) - 1024}):
        assert call(**kw) == -1, kw
        assert b"resample_poly" in lib.ds_last_error_string(), kw
    assert call(out=p + 2) == -3 and b"resample_poly" in lib.ds_last_error_string()
    with pytest.raises(L.DsError, match="resample_poly"):
        L.call("ds_resample_poly", p, p, p, 1, 1, 16385, 4096, 1000, 400, 8821, p, None)
