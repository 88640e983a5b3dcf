"""Restatement (numpy) of the pitch detector: what diffusynth_amd/pitch.py and csrc/pitch.hip are held to.

    yin             YIN (de Cheveigne & Kawahara 2002) per frame as include/diffusynth_hip.h states it: the difference function as
                    differences, the cumulative-mean-normalised form (1 where the running sum is 0), the first tau under the threshold,
                    the walk down the dip, the parabola.  No global-minimum fallback: a frame without a tau under the threshold is unvoiced
                    (period 0, aperiodicity 1).
    lower_median    the element of rank (n_voiced - 1) // 2 among the periods > 0
    estimate        f0 = sample_rate / median period, midi = 69 + 12 log2(f0 / 440), nan below min_voiced

dtype float64 is the semantics; float32 is the "twin" the GPU tolerances are derived from: the same operations in fp32 in the kernel's
order (four interleaved accumulators j mod 4 walked in j order and summed as (a0 + a1) + (a2 + a3); the running sum in tau order).  The
twin rounds each square before it adds it where the kernel uses a fused multiply-add; that difference is inside the 8 x rule.

fragile() marks the frames whose DECISION (voiced or not, which integer tau) hangs on rounding in the float64 form; tone() is the test
signal."""
import math

import numpy as np

SR, FMIN, FMAX, W, HOP, THRESHOLD = 16000, 55.0, 1000.0, 1024, 256, 0.1


def taus(sample_rate=SR, fmin=FMIN, fmax=FMAX):
    """(tau_min, tau_max) as the package computes them."""
    return max(2, int(sample_rate / fmax)), int(sample_rate // fmin)


def frame_count(n, frame_length, tau_max, hop):
    return max(0, (n - frame_length - tau_max) // hop + 1)


def cmnd(x, frame_length=W, hop=HOP, tau_max=290, dtype=np.float64):
    """(n_frames, tau_max + 1) cumulative-mean-normalised difference function of every frame of x."""
    x = np.asarray(x, dtype)
    nf = frame_count(len(x), frame_length, tau_max, hop)
    if nf == 0:
        return np.ones((0, tau_max + 1), dtype)
    fr = x[np.arange(nf)[:, None] * hop + np.arange(frame_length + tau_max)[None, :]]
    d = np.zeros((nf, tau_max + 1), dtype)
    head = fr[:, :frame_length]
    pad = (-frame_length) % 4
    for tau in range(tau_max + 1):
        e = head - fr[:, tau:tau + frame_length]
        sq = e * e
        if dtype == np.float32:
            sq = np.concatenate([sq, np.zeros((nf, pad), dtype)], axis=1).reshape(nf, -1, 4)
            a = np.cumsum(sq, axis=1, dtype=dtype)[:, -1, :]                   # cumsum adds in order: four sequential accumulators
            d[:, tau] = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])
        else:
            d[:, tau] = sq.sum(axis=1)
    c = np.ones_like(d)
    run = np.cumsum(d[:, 1:], axis=1, dtype=dtype)
    t = np.arange(1, tau_max + 1).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        c[:, 1:] = np.where(run > 0, (d[:, 1:] * t[None, :]) / np.where(run > 0, run, 1), dtype(1))
    return c


def pick_of(c, tau_min, tau_max, threshold):
    """Integer pick of one frame's c, or 0 for unvoiced."""
    below = np.nonzero(c[tau_min:tau_max] < threshold)[0]
    if len(below) == 0:
        return 0
    t = tau_min + int(below[0])
    while t + 1 < tau_max and c[t + 1] < c[t]:
        t += 1
    return t


def yin(x, sample_rate=SR, fmin=FMIN, fmax=FMAX, frame_length=W, hop=HOP, threshold=THRESHOLD, dtype=np.float64, c=None):
    """-> (period, aperiodicity, pick) per frame: dtype, dtype, int64 (pick 0 = unvoiced)."""
    tau_min, tau_max = taus(sample_rate, fmin, fmax)
    if c is None:
        c = cmnd(x, frame_length, hop, tau_max, dtype)
    thr, half, two = dtype(threshold), dtype(0.5), dtype(2.0)
    nf = c.shape[0]
    period, aper, picks = np.zeros(nf, dtype), np.ones(nf, dtype), np.zeros(nf, np.int64)
    for f in range(nf):
        t = pick_of(c[f], tau_min, tau_max, thr)
        if t == 0:
            continue
        a, b, cc = c[f, t - 1], c[f, t], c[f, t + 1]
        den = (a - two * b) + cc
        off = half * (a - cc) / den if (den > 0 and b <= a and b <= cc) else dtype(0)
        period[f], aper[f], picks[f] = dtype(t) + off, b, t
    return period, aper, picks


def fragile(x, sample_rate=SR, fmin=FMIN, fmax=FMAX, frame_length=W, hop=HOP, threshold=THRESHOLD, c=None):
    """bool per frame: the float64 decision hangs on rounding — some c(tau) with tau in [tau_min, pick + 1] (an unvoiced frame: the whole
    search range) within 1e-3 of the threshold, |c(pick + 1) - c(pick)| < 1e-5, or the pick is tau_max - 1."""
    tau_min, tau_max = taus(sample_rate, fmin, fmax)
    if c is None:
        c = cmnd(x, frame_length, hop, tau_max)
    out = np.zeros(c.shape[0], bool)
    for f in range(c.shape[0]):
        t = pick_of(c[f], tau_min, tau_max, threshold)
        hi = t + 2 if t else tau_max
        near = np.abs(c[f, tau_min:hi] - threshold) < 1e-3
        out[f] = near.any() or (t != 0 and (abs(c[f, t + 1] - c[f, t]) < 1e-5 or t == tau_max - 1))
    return out


def lower_median(period):
    """(the element of rank (n - 1) // 2 among the periods > 0, n); (0, 0) when nothing is voiced."""
    v = np.sort(np.asarray(period)[np.asarray(period) > 0])
    return (v[(len(v) - 1) // 2], len(v)) if len(v) else (np.asarray(period).dtype.type(0), 0)


def midi_of(f0):
    return 69.0 + 12.0 * math.log2(f0 / 440.0)


def estimate(x, sample_rate=SR, fmin=FMIN, fmax=FMAX, frame_length=W, hop=HOP, threshold=THRESHOLD, min_voiced=0.25, dtype=np.float64):
    """-> (f0, midi, voiced, frames); f0 = midi = nan for a signal without frames or with voiced < min_voiced * frames."""
    period, _, _ = yin(x, sample_rate, fmin, fmax, frame_length, hop, threshold, dtype)
    med, voiced = lower_median(period)
    frames = len(period)
    if frames == 0 or voiced == 0 or voiced < min_voiced * frames:
        return float("nan"), float("nan"), voiced, frames
    f0 = float(sample_rate) / float(med)
    return f0, midi_of(f0), voiced, frames


def cents(midi_a, midi_b):
    return 100.0 * (midi_a - midi_b)


# ---------------------------------------------------------------------------------------------------- seeded inputs
STRONG = (1.0, 0.5, 0.33, 0.25, 0.2)
WEAK = (0.15, 1.0, 0.6, 0.3, 0.2)                       # a weak fundamental under a strong octave: the octave trap
TONE_F0 = (65.41, 110.0, 164.81, 155.0, 440.0, 830.6)


def tone(f0, n, seed=0, amps=STRONG, noise=0.01, vib=None, sr=SR):
    """A decaying 5-harmonic tone (float32): 20 ms linear attack, exp(-1.5 t) decay, random partial phases, additive Gaussian noise.
    vib = (depth in rad, rate in Hz): phase modulation of the fundamental (harmonic h gets h times the depth)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    ph = 2 * np.pi * f0 * t
    if vib is not None:
        ph = ph + vib[0] * np.sin(2 * np.pi * vib[1] * t)
    y = sum(a * np.sin((h + 1) * ph + rng.uniform(0, 2 * np.pi)) for h, a in enumerate(amps))
    y = y * np.minimum(1.0, t / 0.02) * np.exp(-1.5 * t) + noise * rng.standard_normal(n)
    return y.astype(np.float32)


def white_noise(n, seed=0):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32) * np.float32(0.3)


class Msg:
    """A mido-like note message."""
    is_meta, tempo = False, 500000

    def __init__(self, time, note, velocity):
        self.type, self.time, self.note, self.velocity = "note_on", time, note, velocity


TPB = 480                                                # at the default tempo a tick is 1 / 960 s


def note_messages(events, gap=240):
    """events: (note, duration in ticks) -> messages of a monophonic line, `gap` ticks between notes (overlapping tails: a note's sample
    outlasts its event)."""
    out = []
    for note, dur in events:
        out += [Msg(gap, note, 90), Msg(dur, note, 0)]
    return out
