"""CPU suite of the loudness meter (diffusynth_amd.loudness, Mastering(target_lufs=)): the coefficients, the restatement
(tests/loudness_ref.py) against scipy and against the standard's own check, what the fixtures can see, the refusals, the header."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import loudness_ref as R
import diffusynth_amd
from conftest import ROOT
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

LM = importlib.import_module("diffusynth_amd.loudness")          # (the package's attribute `loudness` is the function)
LU = L.LU


# ---------------------------------------------------------------------------------------------------- coefficients
def test_kweighting_at_48_khz_is_the_standards_table():
    (b1, a1), (b2, a2) = diffusynth_amd.kweighting(48000)
    got = [b1[0], b1[1], b1[2], a1[1], a1[2], a2[1], a2[2]]
    assert all(v.dtype == np.float64 for v in (b1, a1, b2, a2)) and a1[0] == 1.0 and a2[0] == 1.0 and b2.tolist() == [1.0, -2.0, 1.0]
    for g, w in zip(got, R.TABLE_48K):
        assert abs(g - w) <= 1e-13, (g, w)
    (rb1, ra1), (rb2, ra2) = R.kweighting(48000)                                   # the restatement's own copy of the formulas
    for g, w in zip(got, [rb1[0], rb1[1], rb1[2], ra1[1], ra1[2], ra2[1], ra2[2]]):
        assert abs(g - w) <= 1e-13


def test_hop_and_chunking_at_the_usual_rates():
    assert [LM.hop(fs) for fs in (8000, 11025, 16000, 44100, 48000)] == [800, 1103, 1600, 4410, 4800] == [R.hop(fs) for fs in (8000, 11025, 16000, 44100, 48000)]
    for fs in (8000, 11025, 16000, 22050, 44100, 48000, 96000, 192000):
        h = LM.hop(fs)
        lc, nc, lt = LM.chunking(h)
        assert lc % 2 == 1 and 1 <= nc <= LU["DS_LU_THREADS"] and 1 <= lt <= lc and (nc - 1) * lc + lt == h
        assert LU["DS_LU_MIN_HOP"] <= h <= LU["DS_LU_MAX_HOP"]
        c = LM._coefficients(fs)
        assert c.shape == (LU["DS_LU_NCOEF"],) and c.dtype == np.float64 and np.isfinite(c).all()
        m = LM.transition(fs)
        at = lambda o: c[o:o + 16].reshape(4, 4)                                   # noqa: E731
        np.testing.assert_allclose(at(LU["DS_LU_C_PTAIL"]), np.linalg.matrix_power(m, lt), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(at(LU["DS_LU_C_PSCAN"] + 16 * 3), np.linalg.matrix_power(m, 8 * lc), rtol=1e-9, atol=1e-12)
    # the transition is the recursion's: one zero-input sample of the restatement's filter from each unit state
    (b1, a1), (b2, a2) = R.kweighting(16000)
    m = LM.transition(16000)
    for k in range(4):
        s = [0.0] * 4
        s[k] = 1.0
        y1 = s[0]
        y2 = b2[0] * y1 + s[2]
        nxt = [-a1[1] * y1 + s[1], -a1[2] * y1, (b2[1] * y1 - a2[1] * y2) + s[3], b2[2] * y1 - a2[2] * y2]
        np.testing.assert_allclose(m[:, k], nxt, rtol=0, atol=1e-15)
    assert np.abs(np.linalg.matrix_power(m, 256)).max() > 1.0                       # why the carry is algebraic: 256 samples on, still large


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_equals_lfilter():
    sig = pytest.importorskip("scipy.signal")
    for fs in (16000, 48000):
        x = R.gating_fixture(fs)[:3 * fs]
        (b1, a1), (b2, a2) = R.kweighting(fs)
        want = sig.lfilter(b2, a2, sig.lfilter(b1, a1, x.astype(np.float64)))
        err = np.abs(R.kfilter(x, fs) - want).max()
        print(f"{fs} Hz: restatement against lfilter {err:.3e}")
        assert err <= 1e-12


def test_full_scale_997_hz_sine_reads_minus_3_01():
    r = R.loudness(R.sine(48000, 5.0), 48000)
    print(f"48 kHz: {r['L']:.4f} LUFS, {r['nb']} blocks")
    assert abs(r["L"] - (-3.01)) <= 0.01 and r["nb"] == 47 == r["n2"]
    r16 = R.loudness(R.sine(16000, 5.0), 16000)                                    # this package's value (re-derived coefficients), not the standard's
    print(f"16 kHz: {r16['L']:.4f} LUFS")
    assert abs(r16["L"] - (-2.9700)) <= 1e-3


# ---------------------------------------------------------------------------------------------------- what the fixtures can see
@pytest.fixture(scope="module")
def gating():
    x = R.gating_fixture()
    return x, R.loudness(x, 16000)


def test_both_gates_remove_blocks_on_the_gating_fixture(gating):
    x, r = gating
    print({k: v for k, v in r.items() if k != "z"})
    assert len(x) % 1600 == 837 and r["nb"] == len(x) // 1600 - 3
    assert r["nb"] - r["n1"] >= 1 and r["n1"] - r["n2"] >= 1 and r["n2"] >= 1
    lv = np.array([R.lufs(v) for v in r["z"]])
    assert (lv < -75).any() and (lv > -12).any() and ((lv > -24) & (lv < -22)).any()   # the stretches at about -80, full level and about -15 dB
    assert abs(float(np.mean(x.astype(np.float64))) - 0.1) < 0.01                   # the DC offset the high-pass holds in its state


@pytest.mark.parametrize("defect", ["no_carry", "carry_first_stage_only", "partial_last_block_counted", "gate_in_db_rounded"])
def test_every_defect_model_moves_the_loudness(gating, defect):
    x, r = gating
    bad = R.loudness(x, 16000, **{defect: True})
    print(f"{defect}: L {bad['L']:.5f} against {r['L']:.5f}, blocks {bad['nb']} / {bad['n1']} / {bad['n2']} against {r['nb']} / {r['n1']} / {r['n2']}")
    assert abs(bad["L"] - r["L"]) > 1e-3


def test_no_block_lies_on_a_gate(gating):
    """A condition on the fixtures: with it the gate decisions of the device's float64 chain (1e-9 off at the most) and the restatement's
    are the same."""
    sigs = [(gating[0], 16000, gating[1])]
    for fs in (11025, 16000, 44100, 48000):
        x = R.noise(6 * R.hop(fs) + 11, 1, fs=fs)
        sigs.append((x, fs, R.loudness(x, fs)))
    for x, fs, r in sigs:
        z = r["z"]
        d_abs = np.abs(z / R.Z_ABS - 1.0).min()
        d_rel = np.abs(z / r["z_rel"] - 1.0).min() if r["z_rel"] > 0 else math.inf
        print(f"{fs} Hz, {len(x)} samples: nearest block {d_abs:.2e} from z_abs, {d_rel:.2e} from z_rel")
        assert d_abs > 1e-6 and d_rel > 1e-6


# ---------------------------------------------------------------------------------------------------- refusals, before any device work
def test_mastering_target_lufs_refusals():
    m = A.Mastering(target_rms=None, target_lufs=-14.0)
    assert m.target_lufs == -14.0 and A.Mastering().target_lufs is None and m.samples(16000) == (80, 800)
    assert A.Mastering(target_rms=None, target_lufs=0).target_lufs == 0 and A.Mastering(target_rms=None, target_lufs=-70.0).target_lufs == -70.0
    with pytest.raises(ValueError, match="target_lufs.*target_rms"):
        A.Mastering(target_lufs=-14.0)                                             # target_rms keeps its default: both set
    with pytest.raises(ValueError, match="target_lufs.*target_rms"):
        A.Mastering(target_rms=0.2, target_lufs=-14.0)
    for bad in (math.nan, math.inf, -math.inf, 0.5, -70.5, "-14", True):
        with pytest.raises(ValueError, match="Mastering.*target_lufs"):
            A.Mastering(target_rms=None, target_lufs=bad)
    for sr in (7999, 4000, 1000000):
        with pytest.raises(ValueError, match="sample_rate"):
            m.samples(sr)
    assert A.Mastering().samples(4000) == (20, 200)                                # without a LUFS target a low rate is the RMS form's business


def test_loudness_and_master_refuse_before_they_ask_for_a_device():
    x = torch.zeros(8000)                                                         # a CPU tensor: a valid call ends in the RuntimeError below
    f = diffusynth_amd.loudness
    assert f is LM.loudness and diffusynth_amd.Loudness is LM.Loudness and diffusynth_amd.kweighting is LM.kweighting
    assert LM.Loudness._fields == ("integrated", "momentary_max", "threshold", "blocks", "gated")
    for sr in (0, 7999, -16000, 16000.0, "16000", True, None, 10 ** 6):
        with pytest.raises(ValueError, match="sample_rate"):
            f(x, sr)
        with pytest.raises(ValueError, match="sample_rate"):
            diffusynth_amd.kweighting(sr)
    with pytest.raises(ValueError, match="signals.*empty"):
        f([x, torch.zeros(0)])
    with pytest.raises(ValueError, match="signals.*empty"):
        f(torch.zeros(2, 0))
    with pytest.raises(ValueError, match=r"signals.*2\^24"):
        f(torch.zeros(2 ** 24 + 1))
    for bad in ([], torch.zeros(2, 3, 4), [torch.zeros(2, 3)], 5, [x, "x"], None):
        with pytest.raises(ValueError, match="signals"):
            f(bad)
    for sig in (x, torch.zeros(2, 500), [x, x[:300]]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(sig)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(sig, 48000, return_blocks=True)
    m = A.Mastering(target_rms=None, target_lufs=-16.0)
    with pytest.raises(ValueError, match="sample_rate"):
        A.master(x, m, sample_rate=4000)
    with pytest.raises(ValueError, match="sample_rate"):
        A.master(x, A.Mastering(), sample_rate=4000, return_loudness=True)
    with pytest.raises(ValueError, match="signals.*empty"):
        A.master([x, torch.zeros(0)], m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.master(x, m, return_loudness=True)
    t = A.Track([], 480)
    assert t.last_loudness is None
    with pytest.raises(ValueError, match="sample_rate"):
        t.render(None, sample_rate=4000, master=m)
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda", master=m)
    assert ds.master == m and ds.last_loudness is None and ds.last_master is None
    with pytest.raises(ValueError, match="sample_rate"):
        ds.arrange([t], ["a"], {}, sample_rate=4000)


# ---------------------------------------------------------------------------------------------------- header, binding, entry points
def test_header_defines_binding_and_exports():
    want = {"DS_LU_ENERGY": 0, "DS_LU_INTEGRATED": 1, "DS_LU_MOMENTARY_MAX": 2, "DS_LU_THRESHOLD": 3, "DS_LU_NS": 4, "DS_LU_TAB_BOFF": L.PV["DS_PV_FOFF"],
            "DS_LU_THREADS": 256, "DS_LU_MIN_HOP": 800, "DS_LU_MAX_HOP": 19200, "DS_LU_C_B1": 0, "DS_LU_C_A1": 3, "DS_LU_C_B2": 5, "DS_LU_C_A2": 8, "DS_LU_C_PTAIL": 16,
            "DS_LU_C_PHOP": 32, "DS_LU_C_PSCAN": 48, "DS_LU_SCAN_STEPS": 8, "DS_LU_NCOEF": 176}
    assert LU == want
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = f.read()
    assert LU == {k: int(v) for k, v in re.findall(r"^#define\s+(DS_LU_\w+)\s+(\d+)\s*$", text, flags=re.M)}
    assert LU["DS_LU_C_PSCAN"] + 16 * LU["DS_LU_SCAN_STEPS"] == LU["DS_LU_NCOEF"] and 2 ** LU["DS_LU_SCAN_STEPS"] == LU["DS_LU_THREADS"]
    assert 4 * LU["DS_LU_MAX_HOP"] + 2 * 256 * 32 + 64 <= 160 * 1024               # a hop and the scan's buffers fit a CU's LDS
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = L.load()
    for name in ("ds_loudness_ws_bytes", "ds_loudness", "ds_loudness_gain"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    assert lib.ds_abi_version() == 1
    ws = lib.ds_loudness_ws_bytes                                                  # 9 float64 per hop of the longest signal, per signal
    assert [ws(1, 1, 1600), ws(1, 1600, 1600), ws(3, 960000, 1600), ws(2, 2 ** 24, 800), ws(0, 5, 1600), ws(1, 0, 1600), ws(1, 2 ** 24 + 1, 1600), ws(1, 5, 799),
            ws(1, 5, 19201)] == [72, 72, 3 * 600 * 72, 2 * 20971 * 72, 0, 0, 0, 0, 0]


def test_entries_validate_before_any_gpu_work():
    lib = L.load()
    buf = (ctypes.c_double * 256)()
    p = ctypes.addressof(buf)
    coef = np.ascontiguousarray(LM._coefficients(16000))
    cp = coef.ctypes.data
    args = (("x", p), ("tab", p), ("n", 1), ("ml", 8000), ("ts", 8000), ("coef", cp), ("h", 1600), ("za", R.Z_ABS), ("ws", p), ("lu", p), ("cnt", p), ("blocks", None),
            ("tb", 0), ("st", None))
    meas = lambda **kw: lib.ds_loudness(*[kw.get(k, v) for k, v in args])          # noqa: E731
    nan = coef.copy()
    nan[LU["DS_LU_C_PHOP"] + 5] = math.nan
    for kw in ({"x": None}, {"tab": None}, {"coef": None}, {"ws": None}, {"lu": None}, {"cnt": None}, {"n": 0}, {"n": 65536}, {"ml": 0}, {"ml": 2 ** 24 + 1}, {"ts": 0},
               {"ts": 1 << 31}, {"h": 799}, {"h": 19201}, {"za": -1.0}, {"za": math.nan}, {"za": math.inf}, {"blocks": p, "tb": 0}, {"blocks": p, "tb": 1 << 31},
               {"coef": nan.ctypes.data}):
        assert meas(**kw) == -1, kw
        assert b"loudness" in lib.ds_last_error_string(), kw
    assert meas(x=p + 2) == -3 and meas(ws=p + 4) == -3 and meas(lu=p + 4) == -3 and meas(blocks=p + 4, tb=5) == -3
    gain = lambda **kw: lib.ds_loudness_gain(*[kw.get(k, v) for k, v in (("lu", p), ("n", 1), ("zt", 0.01), ("mg", 10.0), ("stats", p), ("st", None))])   # noqa: E731
    for kw in ({"lu": None}, {"stats": None}, {"n": 0}, {"n": 65536}, {"zt": 0.0}, {"zt": -1.0}, {"zt": math.nan}, {"zt": math.inf}, {"mg": 0.0}, {"mg": math.nan},
               {"mg": math.inf}):
        assert gain(**kw) == -1, kw
        assert b"loudness_gain" in lib.ds_last_error_string(), kw
    assert gain(lu=p + 4) == -3 and gain(stats=p + 2) == -3
