"""The pitch detector on the GPU (csrc/pitch.hip, diffusynth_amd/pitch.py) against its float64 restatement (tests/pitch_ref.py).

Decisions and values are held apart.  The DECISION of a frame — voiced or not, which integer tau — must be the restatement's on every
frame the restatement does not mark fragile (pitch_ref.fragile: a c(tau) within 1e-3 of the threshold on the way to the pick,
|c(pick + 1) - c(pick)| < 1e-5, or the pick at the end of the search range); fragile frames may fall either way, are left out of the value
comparison, and may be at most 5 % of the set (the final set below: 52 of 1 590 frames, 3.3 %).  The VALUES of the other frames follow the
project's rule: the float32 twin of the restatement against its float64 form on the CPU, the device is allowed 8 x the twin's error, never
less than 2e-6 and never more than 1e-3, through conftest.rel_err; each check prints its figure and its bound.  The median is exact: it is
compared bit for bit with a host selection from the device's own frames.

Device -> host copies are counted by wrapping Tensor.cpu / item / tolist / numpy for CUDA tensors (the package reads results through
nothing else)."""
import functools

import numpy as np
import pytest
import torch

import pitch_ref as P
from conftest import rel_err, rel_errs
from diffusynth_amd import _lib as L
from diffusynth_amd import pitch

pytestmark = pytest.mark.gpu


def bound(twin, want):
    """8 x the twin's error, inside [2e-6, 1e-3]."""
    return min(max(8.0 * max(rel_errs(twin, want)), 2e-6), 1e-3)


def check(got, want, twin, what):
    err, tol = rel_err(got, want), bound(twin, want)
    print(f"{what}: device {err:.2e}, twin {max(rel_errs(twin, want)):.2e}, bound {tol:.2e}")
    assert err < tol, (what, err, tol)
    return tol


@functools.lru_cache(maxsize=None)
def signals():
    """name -> signal: the twelve tones, a vibrato tone, noise, silence, a short tone, and one signal one sample short of a frame."""
    out = {}
    for amps, tag in ((P.STRONG, "strong"), (P.WEAK, "weak")):
        for i, f0 in enumerate(P.TONE_F0):
            out[f"{tag} {f0}"] = P.tone(f0, 30001, seed=i, amps=amps)
    out["vibrato 164.81"] = P.tone(164.81, 28416, seed=20, vib=(0.5, 5.0))
    out["noise"] = P.white_noise(28416, 3)
    out["silence"] = np.zeros(4097, np.float32)
    out["weak 110 short"] = P.tone(110.0, 4097, seed=31, amps=P.WEAK)
    out["one short of a frame"] = P.tone(110.0, P.W + 290 - 1, seed=1)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, **kw):
    """(period64, aper64, picks64, fragile, period32, aper32) of one signal, computed once."""
    x = signals()[name]
    tau_max = P.taus(kw.get("sample_rate", P.SR), kw.get("fmin", P.FMIN), kw.get("fmax", P.FMAX))[1]
    c = P.cmnd(x, kw.get("frame_length", P.W), kw.get("hop", P.HOP), tau_max)
    p64, a64, k64 = P.yin(x, c=c, **kw)
    p32, a32, _ = P.yin(x, dtype=np.float32, **kw)
    return p64, a64, k64, P.fragile(x, c=c, **kw), p32, a32


@functools.lru_cache(maxsize=None)
def device_frames():
    """The whole set as ONE ragged launch: name -> (period, aperiodicity) CUDA tensors."""
    names = list(signals())
    got = pitch.yin([torch.from_numpy(signals()[n]).cuda() for n in names])
    return dict(zip(names, got))


def compare(name, period, aper, ref):
    """Decisions on the non-fragile frames, values on them by the 8 x rule -> (frames, fragile frames, the period's bound)."""
    p64, a64, k64, frag, p32, a32 = ref
    period, aper = period.cpu().numpy(), aper.cpu().numpy()
    assert period.shape == aper.shape == p64.shape, name
    assert not np.isnan(period).any() and not np.isnan(aper).any(), name
    keep = ~frag
    picks = np.floor(period + 0.5).astype(np.int64)
    assert np.array_equal(picks[keep], k64[keep]), (name, np.nonzero(keep & (picks != k64))[0])
    if not keep.any():
        return len(frag), int(frag.sum()), 2e-6
    tol = check(period[keep], p64[keep], p32[keep], f"period [{name}] {int(keep.sum())} of {len(keep)} frames")
    check(aper[keep], a64[keep], a32[keep], f"aperiodicity [{name}]")
    assert np.all(aper[keep][k64[keep] == 0] == 1.0) and not period[keep][k64[keep] == 0].any(), name      # unvoiced: exactly (0, 1)
    return len(frag), int(frag.sum()), tol


# ---------------------------------------------------------------------------------------------------- frames
def test_frames_of_a_ragged_batch_in_one_launch():
    total = fragile = 0
    for name, (period, aper) in device_frames().items():
        n, f, _ = compare(name, period, aper, reference(name))
        total, fragile = total + n, fragile + f
    print(f"fragile frames: {fragile} of {total} ({100.0 * fragile / total:.1f} %)")
    assert total == 12 * 113 + 106 + 106 + 11 + 11 + 0 and fragile <= 0.05 * total
    assert device_frames()["one short of a frame"][0].numel() == 0
    assert not device_frames()["noise"][0].any() and not device_frames()["silence"][0].any()               # both unvoiced on every frame


def test_a_frame_does_not_depend_on_its_batch():
    for name, (period, aper) in device_frames().items():
        x = torch.from_numpy(signals()[name]).cuda()
        (p1, a1), = pitch.yin([x])
        assert torch.equal(p1, period) and torch.equal(a1, aper), name
    x = torch.from_numpy(np.stack([signals()["strong 440.0"], signals()["weak 65.41"]])).cuda()               # the (B, L) form
    p, a = pitch.yin(x)
    assert p.shape == a.shape == (2, 113)
    assert torch.equal(p[0], device_frames()["strong 440.0"][0]) and torch.equal(a[1], device_frames()["weak 65.41"][1])


# ---------------------------------------------------------------------------------------------------- edges
def test_frame_count_edges_and_empty_ends():
    n0 = P.W + 290
    lens = [n0 - 1, n0, n0 + P.HOP - 1, n0 + P.HOP, 100]
    xs = [P.tone(220.0, n, seed=40 + i) for i, n in enumerate(lens)]
    got = pitch.yin([torch.from_numpy(x).cuda() for x in xs])                     # the first and the last signal have no frame
    assert [p.numel() for p, _ in got] == [a.numel() for _, a in got] == [0, 1, 1, 2, 0]
    for x, (p, a) in zip(xs[1:4], got[1:4]):
        p64, a64, k64 = P.yin(x)
        keep = ~P.fragile(x)
        assert np.array_equal(np.floor(p.cpu().numpy() + 0.5)[keep], k64[keep]) and k64.all()
        (p1, a1), = pitch.yin([torch.from_numpy(x).cuda()])
        assert torch.equal(p1, p) and torch.equal(a1, a)
    none = pitch.yin([torch.from_numpy(xs[0]).cuda(), torch.from_numpy(xs[4]).cuda()])                       # nothing to launch at all
    assert [p.numel() for p, _ in none] == [0, 0]
    est = pitch.estimate_pitch([torch.from_numpy(xs[0]).cuda(), torch.from_numpy(xs[4]).cuda()])
    assert np.isnan(est.midi).all() and not est.frames.any() and not est.voiced.any()


def test_largest_lds_image_and_smallest_tau_min():
    """tau_max = 1024 with frame_length = 2048 (12 KB of samples), tau_min = 2, an odd hop; and an odd frame length (the j mod 4 tail)."""
    x = P.tone(65.41, 2048 + 1024 + 2 * 301 + 7, seed=50)
    for kw in (dict(fmin=15.625, fmax=8000.0, frame_length=2048, hop=301), dict(fmin=15.625, fmax=8000.0, frame_length=1023, hop=700)):
        assert P.taus(P.SR, kw["fmin"], kw["fmax"]) == (2, 1024)
        (p, a), = pitch.yin([torch.from_numpy(x).cuda()], fmin=kw["fmin"], fmax=kw["fmax"], frame_length=kw["frame_length"], hop_length=kw["hop"])
        c = P.cmnd(x, kw["frame_length"], kw["hop"], 1024)
        p64, a64, k64 = P.yin(x, c=c, **kw)
        p32, a32, _ = P.yin(x, dtype=np.float32, **kw)
        assert len(p64) == 3 and k64.all()
        n, f, _ = compare(f"W {kw['frame_length']} tau_max 1024", p, a, (p64, a64, k64, P.fragile(x, c=c, **kw), p32, a32))
        assert f < n


def test_argument_errors_are_errors_not_launches():
    x = torch.zeros(5000, device="cuda")
    tab = torch.tensor([0, 5000, 0, 4], dtype=torch.int32, device="cuda")
    out = torch.full((2, 4), -7.0, device="cuda")
    def call(**kw):                                                               # noqa: E306
        a = dict(n=1, mf=4, ts=5000, tf=4, W=1024, hop=256, tmin=16, tmax=290, thr=0.1)
        a.update(kw)
        L.call("ds_yin_frames", x.data_ptr(), tab.data_ptr(), a["n"], a["mf"], a["ts"], a["tf"], a["W"], a["hop"], a["tmin"], a["tmax"], a["thr"],
               out[0].data_ptr(), out[1].data_ptr(), L.current_stream())
    for kw in (dict(tmax=1025), dict(W=2049), dict(tmin=1), dict(thr=1.0), dict(hop=0), dict(mf=0)):
        with pytest.raises(L.DsError, match="yin_frames"):
            call(**kw)
    with pytest.raises(L.DsError, match="pitch_median"):
        L.call("ds_pitch_median", out[0].data_ptr(), tab.data_ptr(), 1, 8193, 4, out[1].data_ptr(), tab.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    assert torch.all(out == -7.0)                                                 # nothing ran
    # a table that promises more than the buffers hold: the rows are skipped, nothing is read or written
    bad = torch.tensor([0, 6000, 0, 4, 0, 5000, 2, 4], dtype=torch.int32, device="cuda")
    L.call("ds_yin_frames", x.data_ptr(), bad.data_ptr(), 2, 4, 5000, 4, 1024, 256, 16, 290, 0.1, out[0].data_ptr(), out[1].data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    assert torch.all(out == -7.0)
    with pytest.raises(ValueError, match="^signals"):
        pitch.estimate_pitch([torch.zeros(1314 + 8192, device="cuda")], hop_length=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pitch.yin(torch.zeros(1, 5000))


# ---------------------------------------------------------------------------------------------------- median
def device_median(periods):
    """ds_pitch_median on period buffers written straight to the device -> (median fp32 array, voiced int array)."""
    nf = [len(p) for p in periods]
    tab = np.zeros((len(nf), L.YIN["DS_YIN_NI"]), np.int32)
    tab[:, L.YIN["DS_YIN_NF"]] = nf
    tab[1:, L.YIN["DS_YIN_FOFF"]] = np.cumsum(nf)[:-1]
    flat = torch.from_numpy(np.concatenate(periods).astype(np.float32)).cuda()
    dtab = torch.from_numpy(tab.reshape(-1)).cuda()
    med = torch.full((len(nf),), float("nan"), device="cuda")
    cnt = torch.full((len(nf),), -1, dtype=torch.int32, device="cuda")
    L.call("ds_pitch_median", flat.data_ptr(), dtab.data_ptr(), len(nf), max(nf), flat.numel(), med.data_ptr(), cnt.data_ptr(), L.current_stream())
    return med.cpu().numpy(), cnt.cpu().numpy()


def test_median_is_an_exact_selection():
    rng = np.random.default_rng(7)
    big = rng.integers(20, 60, 8192).astype(np.float32) + rng.integers(0, 4, 8192).astype(np.float32) * np.float32(0.25)    # ties by the hundred
    big[rng.random(8192) < 0.3] = 0
    cases = [np.array([0, 5.5, 3.25, 0, 9.0, 7.0, 4.0], np.float32),             # five voiced
             np.array([4.0, 0, 2.0, 8.0, 16.0], np.float32),                      # four: the LOWER of the two middle ones
             np.array([0, 0, 33.3, 0], np.float32),                               # one
             np.zeros(6, np.float32),                                             # none
             np.array([7.0], np.float32), big, big[:257], np.full(300, 41.5, np.float32)]
    med, cnt = device_median(cases)
    for i, p in enumerate(cases):
        want, n = P.lower_median(p)
        assert cnt[i] == n and med[i] == want and (n == 0 or med[i] in p), i
    assert med[:5].tolist() == [5.5, 4.0, np.float32(33.3), 0.0, 7.0] and cnt[:5].tolist() == [5, 4, 1, 0, 1]
    # and from the device's own frames
    names = [n for n in device_frames() if device_frames()[n][0].numel()]
    med, cnt = device_median([device_frames()[n][0].cpu().numpy() for n in names])
    for i, n in enumerate(names):
        want, nv = P.lower_median(device_frames()[n][0].cpu().numpy())
        assert med[i] == want and cnt[i] == nv, n


# ---------------------------------------------------------------------------------------------------- estimate_pitch
class CopyCounter:
    """Counts device -> host reads of CUDA tensors while active."""
    NAMES = ("cpu", "item", "tolist", "numpy")

    def __init__(self, monkeypatch):
        self.count = 0
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)

            def wrapped(t, *a, _orig=orig, **kw):
                if t.is_cuda:
                    self.count += 1
                return _orig(t, *a, **kw)
            monkeypatch.setattr(torch.Tensor, name, wrapped)


def test_estimate_pitch(monkeypatch):
    names = list(signals())
    xs = [torch.from_numpy(signals()[n]).cuda() for n in names]
    frames = {n: (p.cpu().numpy(), a.cpu().numpy()) for n, (p, a) in device_frames().items()}
    torch.cuda.synchronize()
    counter = CopyCounter(monkeypatch)
    est = pitch.estimate_pitch(xs)
    assert counter.count == 1                                                     # one copy for the whole batch
    monkeypatch.undo()
    assert est.f0.dtype == est.midi.dtype == np.float64 and est.voiced.dtype.kind == est.frames.dtype.kind == "i"
    for i, name in enumerate(names):
        p64, a64, k64, frag, p32, a32 = reference(name)
        period = frames[name][0]
        med, nv = P.lower_median(period)
        assert est.frames[i] == len(p64) and est.voiced[i] == nv and est.period[i] == float(med), name       # the device's own frames, exactly
        f0, midi, voiced, n = P.estimate(signals()[name])
        if name in ("noise", "silence", "one short of a frame"):
            assert np.isnan(est.f0[i]) and np.isnan(est.midi[i]) and np.isnan(midi), name
            continue
        assert est.f0[i] == P.SR / float(med) and est.midi[i] == 69.0 + 12.0 * np.log2(est.f0[i] / 440.0), name
        if np.array_equal(np.floor(period + 0.5).astype(np.int64), k64):          # where every pick agrees (test_frames: all but fragile frames)
            keep = ~frag
            tol = bound(p32[keep], p64[keep])
            cents = abs(est.midi[i] - midi) * 100
            print(f"estimate [{name}]: {est.midi[i]:.6f} for {midi:.6f}, {cents:.2e} cents, bound {1200 * np.log2(1 + tol):.2e}")
            assert cents <= 1200 * np.log2(1 + tol), name
        else:
            print(f"estimate [{name}]: a fragile frame decided differently; held to the device's own frames only")
    agree = [n for n in names if not reference(n)[3].any()]
    assert len(agree) >= 8                                                        # the value check above is not vacuous
    i = names.index("weak 110.0")                                                # no fragile frame: every frame voiced on the device, too
    assert est.voiced[i] == est.frames[i] and pitch.estimate_pitch([xs[i]], min_voiced=1.0).midi[0] == est.midi[i]
    one = pitch.estimate_pitch(torch.from_numpy(signals()["strong 440.0"]).cuda()[None])                     # (1, L): what shares the batch does not matter
    assert one.midi[0] == est.midi[names.index("strong 440.0")]
