"""The mastering stage without a device: the restatement (tests/master_ref.py) against its own definition and guarantees, the refusals of
Mastering / master / the launchers, the header's defines and the LDS budget."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import master_ref as M
from conftest import ROOT
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A
import diffusynth_amd

MS = L.MS
F32 = np.float32
PAIRS = [(0, 0), (1, 1), (80, 80), (80, 800)]


def probe(A_, R_, n=None, **kw):
    """Four stretches (loud, quiet, loud, quiet) and a bit: the middle spike falls into the second loud one, the last into a quiet one."""
    return M.signal(n or 4 * (R_ + 3 * A_ + 37) + 411, A_, R_, **kw)


# ---------------------------------------------------------------------------------------------------- the restatement itself
def test_windowed_minimum_and_sums_equal_their_definitions():
    x = probe(5, 23, 700)
    u, r = M.required(x, 1.0, M.DEFAULTS["ceiling"])
    for a, h in [(0, 0), (1, 1), (5, 23), (7, 7), (0, 40)]:
        m = M.hold_min(r, a, h)
        assert m.dtype == F32 and m.shape == (len(x) + 2 * a,) and np.array_equal(m, M.hold_min_by_definition(r, a, h))
        s = M.window_sums(m, a)
        assert np.array_equal(s, np.array([math.fsum(m[n:n + 2 * a + 1].tolist()) for n in range(len(x))]))


@pytest.mark.parametrize("a,h", PAIRS, ids=[f"A{a}_R{h}" for a, h in PAIRS])
@pytest.mark.parametrize("gl", [None, 2.0], ids=["own_gain", "gain_2"])
def test_restatement_keeps_its_guarantees(a, h, gl):
    """gl=None: the signal's own gain (3 / rms, below 2); gl=2: the largest the GPU tests allow, the spikes at 2^10 c, the 55 Hz stretches
    far over the ceiling."""
    x = probe(a, h)
    res = M.master(x, a, h, gl=gl, target_rms=3.0, max_gain=2.0)
    c, u, r, g, y = res["c"], res["u"], res["r"], res["g"], res["y"]
    assert res["gain"] <= 2.0 and 10 * float(c) < np.abs(u).max() <= 2 ** 10 * float(c)      # far over the ceiling, inside the exactness range
    assert gl is None or np.abs(u).max() == 2 ** 10 * float(c)                    # and with the largest gain at its edge
    assert np.all(g <= r)                                                         # the limiter's guarantee
    assert np.abs(y).max() <= c
    raw = (g * u).astype(F32)                                                     # before the clamp: at most one ulp over the ceiling
    over = np.abs(raw) > c
    assert np.all(np.abs(raw[over]) <= np.nextafter(c, F32(2)))
    print(f"A={a} R={h}: gL={res['gain']}, {over.sum()} samples one ulp over before the clamp, {res['limited']} limited, min g {res['min_gain']}")
    one = g == F32(1.0)
    assert one.any() and (~one).any() and res["limited"] == np.count_nonzero(~one) and res["min_gain"] == g.min()
    assert np.array_equal(y[one], (res["gain"] * x).astype(F32)[one])             # untouched where nothing within reach is over
    assert g[0] < 1 and g[-1] < 1 and g[len(x) // 2] < 1                          # the spikes at both ends and in the middle
    # the window sums do not depend on their order: forwards, backwards, exactly
    m64 = res["m"].astype(np.float64)
    n_idx = np.unique(np.concatenate([np.arange(0, len(x), 97), np.flatnonzero(~one)[:200], [len(x) - 1]]))
    sums = M.window_sums(res["m"], a)
    for n in n_idx:
        w = m64[n:n + 2 * a + 1]
        fwd = bwd = 0.0
        for v in w:
            fwd += v
        for v in w[::-1]:
            bwd += v
        assert fwd == bwd == math.fsum(w.tolist()) == sums[n]


def test_no_target_is_unit_gain_and_silence_stays_silence():
    x = probe(80, 800)
    res = M.master(x, 80, 800, target_rms=None)
    assert res["gain"] == F32(1.0) and res["gain"].dtype == F32 and np.array_equal(res["u"], x)
    assert np.all(res["g"] <= res["r"]) and np.abs(res["y"]).max() <= res["c"] and res["limited"] > 800      # 55 Hz at 2.5: held down, not ridden
    z = M.master(np.zeros(1000, F32), 80, 800)
    assert z["rms"] == 0.0 and z["gain"] == F32(10.0) and not z["y"].any() and z["limited"] == 0 and z["min_gain"] == 1 and not np.isnan(z["y"]).any()
    q = M.master(1e-4 * probe(80, 800, loud=0.5, ceiling=1e-3), 80, 800)          # a quiet signal: the gain stops at max_gain
    assert q["gain"] == F32(10.0) and q["gain64"] == 10.0
    assert M.samples(0.005, 0.05) == (80, 800) and M.samples(0.0, 0.0) == (0, 0)


# ---------------------------------------------------------------------------------------------------- refusals, before any device work
def test_mastering_refuses_bad_values():
    m = A.Mastering()
    assert (m.target_rms, m.max_gain, m.ceiling, m.lookahead, m.hold) == (0.1, 10.0, 10 ** (-1 / 20), 0.005, 0.05) == tuple(M.DEFAULTS.values())
    assert A.Mastering(target_rms=None).target_rms is None and A.Mastering(ceiling=1.0, lookahead=0.0, hold=0.0).samples(16000) == (0, 0)
    assert m.samples(16000) == (80, 800) and m.samples(44100) == (220, 2205)
    with pytest.raises(TypeError):
        A.Mastering(0.1)                                                           # keyword-only
    with pytest.raises(Exception):
        m.hold = 1.0                                                               # frozen
    bad = [dict(target_rms=0.0), dict(target_rms=-0.1), dict(target_rms=math.nan), dict(target_rms=math.inf), dict(target_rms="0.1"),
           dict(max_gain=0.0), dict(max_gain=-1.0), dict(max_gain=math.inf), dict(max_gain=None), dict(max_gain=True),
           dict(ceiling=0.0), dict(ceiling=-0.5), dict(ceiling=1.0000001), dict(ceiling=math.nan),
           dict(lookahead=-0.001), dict(lookahead=math.nan), dict(lookahead=0.1), dict(hold=0.004), dict(hold=math.inf), dict(lookahead=0.01, hold=0.009)]
    for kw in bad:
        with pytest.raises(ValueError, match="Mastering"):
            A.Mastering(**kw)


def test_master_refuses_before_it_asks_for_a_device():
    x = torch.zeros(1000)                                                         # a CPU tensor: a valid call ends in the RuntimeError below
    with pytest.raises(ValueError, match="lookahead"):
        A.master(x, A.Mastering(lookahead=0.07, hold=0.08))                        # 1120 samples at 16 kHz
    with pytest.raises(ValueError, match="hold"):
        A.master(x, A.Mastering(hold=0.6))                                         # 9600 samples
    with pytest.raises(ValueError, match="hold"):
        A.master(x, sample_rate=192000)                                            # the defaults at 192 kHz: 9600 samples
    with pytest.raises(ValueError, match="signals.*empty"):
        A.master([x, torch.zeros(0)])
    with pytest.raises(ValueError, match="signals.*empty"):
        A.master(torch.zeros(2, 0))
    with pytest.raises(ValueError, match="signals"):
        A.master([])
    with pytest.raises(ValueError, match="signals"):
        A.master(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="signals"):
        A.master([torch.zeros(2, 3)])
    with pytest.raises(ValueError, match=r"signals.*2\^24"):
        A.master(torch.zeros(2 ** 24 + 1))
    for sr in (0, -16000, 16000.0, "16000", True, None):
        with pytest.raises(ValueError, match="sample_rate"):
            A.master(x, sample_rate=sr)
    with pytest.raises(ValueError, match="mastering"):
        A.master(x, None)
    with pytest.raises(ValueError, match="mastering"):
        A.master(x, dict(M.DEFAULTS))
    for sig in (x, torch.zeros(2, 500), [x, x[:300]], torch.zeros(2 ** 24)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            A.master(sig)
    assert diffusynth_amd.master is A.master and diffusynth_amd.Mastering is A.Mastering and diffusynth_amd.MasterStats is A.MasterStats


def test_wiring_refuses_before_it_asks_for_a_device():
    t = A.Track([], 480)
    with pytest.raises(ValueError, match="master"):
        t.render(None, master="loud")
    with pytest.raises(ValueError, match="hold"):
        t.render(None, master=A.Mastering(hold=0.6))
    with pytest.raises(ValueError, match="master"):
        A.DiffSynth({}, None, None, None, None, None, "cuda", master=0.1)
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda", master=A.Mastering())
    assert ds.master == A.Mastering() and ds.last_master is None
    plain = A.DiffSynth({}, None, None, None, None, None, "cuda")
    assert plain.master is None
    with pytest.raises(ValueError, match="pcm16"):
        plain.arrange([t], ["a"], {}, pcm16=True)
    with pytest.raises(ValueError, match="pcm16"):
        ds.arrange([t], ["a"], {}, master=None, pcm16=True)
    with pytest.raises(ValueError, match="pcm16"):
        plain.get_music(None, ["a"], pcm16=True)
    with pytest.raises(ValueError, match="master"):
        plain.arrange([t], ["a"], {}, master="loud")
    with pytest.raises(ValueError, match="sample_rate"):
        ds.arrange([t], ["a"], {}, sample_rate=16000.5)


# ---------------------------------------------------------------------------------------------------- header, binding, entry points
def test_header_defines_and_lds_budget():
    assert MS == {"DS_MS_GAIN": 0, "DS_MS_RMS": 1, "DS_MS_PEAK": 2, "DS_MS_MIN_GAIN": 3, "DS_MS_NS": 4, "DS_MS_TILE": 4096, "DS_MS_MAX_LOOKAHEAD": 1024,
                  "DS_MS_MAX_HOLD": 8192, "DS_MS_MAX_LEN": 2 ** 24, "DS_MS_CHUNK": 2048, "DS_MS_MAX_PARTS": 512}
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = f.read()
    assert MS == {k: int(v) for k, v in re.findall(r"^#define\s+(DS_MS_\w+)\s+(\d+)\s*$", text, flags=re.M)}
    T, a, h = MS["DS_MS_TILE"], MS["DS_MS_MAX_LOOKAHEAD"], MS["DS_MS_MAX_HOLD"]
    assert 4 * (T + h + 3 * a) + 4 * (T + 2 * a) == 86016 <= 160 * 1024            # the two tiles fit a CU's LDS at the caps
    assert a <= h and 2 * a + 1 < 2 ** 12                                         # the exactness range: 12 + 18 + 23 = 53 bits
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = L.load()
    for name in ("ds_master_ws_bytes", "ds_master_gain", "ds_master_limit"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    assert lib.ds_abi_version() == 1
    # the workspace: one (float64, fp32) partial per DS_MS_CHUNK samples of the longest signal, at most DS_MS_MAX_PARTS, per signal
    ws = lib.ds_master_ws_bytes
    assert [ws(1, 1), ws(1, 2048), ws(1, 2049), ws(3, 960000), ws(2, 2 ** 24), ws(0, 5), ws(1, 0), ws(1, 2 ** 24 + 1)] == [12, 12, 24, 3 * 469 * 12, 2 * 512 * 12, 0, 0, 0]


def test_entries_validate_before_any_gpu_work():
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    q = p + 256                                                                   # a second address for out: it may not be x
    gain = lambda **kw: lib.ds_master_gain(*[kw.get(k, v) for k, v in (("x", p), ("tab", p), ("n", 1), ("ml", 100), ("ts", 100), ("t", 0.1), ("mg", 10.0),   # noqa: E731
                                                                        ("ws", p), ("stats", p), ("lim", p), ("st", None))])
    for kw in ({"x": None}, {"tab": None}, {"ws": None}, {"stats": None}, {"lim": None}, {"n": 0}, {"n": 65536}, {"ml": 0}, {"ml": 2 ** 24 + 1}, {"ts": 0},
               {"ts": 1 << 31}, {"mg": 0.0}, {"mg": -1.0}, {"mg": math.nan}, {"mg": math.inf}, {"t": math.nan}, {"t": math.inf}):
        assert gain(**kw) == -1, kw
        assert b"master_gain" in lib.ds_last_error_string(), kw
    assert gain(ws=p + 4) == -3 and gain(x=p + 2) == -3 and b"master_gain" in lib.ds_last_error_string()
    limit = lambda **kw: lib.ds_master_limit(*[kw.get(k, v) for k, v in (("x", p), ("tab", p), ("n", 1), ("ml", 100), ("ts", 100), ("c", 0.89), ("a", 80),   # noqa: E731
                                                                          ("h", 800), ("stats", p), ("lim", p), ("out", q), ("pcm", None), ("st", None))])
    for kw in ({"x": None}, {"tab": None}, {"stats": None}, {"lim": None}, {"out": None}, {"n": 0}, {"n": 65536}, {"ml": 0}, {"ml": 2 ** 24 + 1}, {"ts": 0},
               {"ts": 1 << 31}, {"a": 1025, "h": 2000}, {"a": -1}, {"h": 8193}, {"a": 80, "h": 79}, {"a": 1, "h": 0}, {"c": 0.0}, {"c": -0.5}, {"c": 1.0000002},
               {"c": math.nan}, {"out": p}):
        assert limit(**kw) == -1, kw
        assert b"master_limit" in lib.ds_last_error_string(), kw
    assert limit(out=q + 2) == -3 and limit(pcm=q + 1) == -3 and b"master_limit" in lib.ds_last_error_string()
    with pytest.raises(L.DsError, match="master_limit.*hold"):
        L.call("ds_master_limit", p, p, 1, 100, 100, 0.89, 80, 8193, p, p, q, None, None)
