"""Restatement (numpy, on top of arranger_ref) of the formant-preserving mode of the pitch shifter: what ds_pv_formant and
pitch_shift(formant=...) are held to.  The arithmetic is DEFINED in include/diffusynth_hip.h; this file says it again.

    correct                    one signal's synthesis frames V (frames, 2049) -> V exp(clamp(S(k / rate) - S(k)))
    pitch_shift_formant        arranger_ref.pitch_shift with `correct` between the phase vocoder and the iSTFT
    pitch_shift_chain_formant  the reference's chain with the per-link order of Formant.node_order
    probe, envelope_shape      the two-formant note and the measure of the property that justifies the mode

Every function takes dtype: float64 is the semantics; float32 is the twin the GPU tolerances are derived from (fp32 log, complex64
transforms, fp32 lerp and exp).  q = fl32(k) * fl32(1 / rate) is ONE fp32 product in both forms: that is the definition."""
import math

import numpy as np

import arranger_ref as R

N_FFT, NB = R.N_FFT, R.N_FFT // 2 + 1
FLOOR = 1e-6


def smooth_log(mag, order, dtype=np.float64):
    """(frames, 2049) magnitudes -> (L, S): the floored log magnitude and its cepstral smoothing of `order` quefrency samples."""
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    L = np.log(np.maximum(mag.astype(dtype), dtype(FLOOR))).astype(dtype)
    full = np.concatenate([L, L[:, NB - 2:0:-1]], axis=1)                       # the even extension to 4096 points
    c = (np.fft.fft(full.astype(ctype), axis=1).astype(ctype) / dtype(N_FFT)).astype(ctype)
    n = np.arange(N_FFT)
    c = np.where(np.minimum(n, N_FFT - n)[None, :] <= order, c, 0).astype(ctype)
    S = (np.fft.ifft(c, axis=1).astype(ctype) * dtype(N_FFT)).real.astype(dtype)
    return L, S[:, :NB]


def warp_of(rate):
    return np.float32(1.0 / rate)


def correct(V, rate, order, max_gain_db, dtype=np.float64, info=None):
    """V (frames, 2049) complex -> V'.  info (a dict): max|L| of the call is kept in info["max_abs_L"] (the tolerance's scale)."""
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    V = np.asarray(V).astype(ctype)
    L, S = smooth_log(np.abs(V), order, dtype)
    if info is not None:
        info["max_abs_L"] = max(info.get("max_abs_L", 0.0), float(np.abs(L).max()))
    q = np.minimum(np.arange(NB, dtype=np.float32) * warp_of(rate), np.float32(N_FFT // 2))      # fp32 in both forms
    i = np.minimum(np.floor(q), N_FFT // 2 - 1).astype(np.int64)
    f = (q - i.astype(np.float32)).astype(dtype)                                                   # (exact in fp32)
    Sq = ((dtype(1.0) - f)[None, :] * S[:, i] + f[None, :] * S[:, i + 1]).astype(dtype)
    lim = dtype(max_gain_db * math.log(10.0) / 20.0)
    d = np.clip((Sq - S).astype(dtype), -lim, lim)
    return (V * np.exp(d).astype(dtype)).astype(ctype)


def pitch_shift_formant(y, n_steps, order, max_gain_db, dtype=np.float64, info=None):
    y = np.asarray(y, dtype)
    rate = R.rate_of(n_steps)
    S = correct(R.phase_vocoder(R.stft(y, dtype), rate, dtype), rate, order, max_gain_db, dtype, info)
    ls = R.stretched_length(len(y), rate)
    ys = R.istft(S, ls, dtype)
    nres = R.resampled_length(ls, rate)
    r = R.resample(ys, rate, min(nres, len(y)), dtype)
    out = np.zeros(len(y), dtype)
    out[:len(r)] = r
    return out


def node_order(order, lo, track_pitch=True):
    """The order of a link entered at cumulative shift `lo`: the period of its input has shrunk by 2^(-lo / 12)."""
    return max(4, int(math.floor(order * min(1.0, 2.0 ** (-lo / 12.0))))) if track_pitch else order


def pitch_shift_chain_formant(y, total, order, max_gain_db, track_pitch=True, step_size=4, dtype=np.float64, info=None):
    cur, lo = y, 0
    for s in R.chain_steps(total, step_size):
        cur = pitch_shift_formant(cur, s, node_order(order, lo, track_pitch), max_gain_db, dtype, info)
        lo += s
    return cur


# ---------------------------------------------------------------------------------------------------- the property
def probe(n=28416, f0=164.8, sr=16000):
    """A two-formant note: harmonics 1 .. 45 of f0 under formants at 700 Hz and 2300 Hz, peak 1, a gentle fade at both ends (float32)."""
    t = np.arange(n) / sr
    y = np.zeros(n)
    for h in range(1, 46):
        fr = h * f0
        amp = math.exp(-((fr - 700.0) / 250.0) ** 2) + 0.5 * math.exp(-((fr - 2300.0) / 400.0) ** 2) + 0.02
        y += amp * np.sin(2 * np.pi * fr * t + h)
    y /= np.abs(y).max()
    return (y * np.hanning(n) ** 0.25).astype(np.float32)


def envelope_shape(y, order=20, lo=76, hi=895):
    """The order-20 envelope of |stft| frames [5:-5], averaged over the frames, bins lo .. hi, its mean removed (nepers)."""
    _, S = smooth_log(np.abs(R.stft(np.asarray(y, np.float64))[5:-5]), order)
    e = S.mean(axis=0)[lo:hi + 1]
    return e - e.mean()


def shape_deviation(y, source):
    """rms over the bins of the difference of the two envelope shapes, in dB."""
    d = envelope_shape(y) - envelope_shape(source)
    return float(np.sqrt(np.mean(d * d)) * 20.0 / math.log(10.0))
