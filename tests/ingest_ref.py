"""Float64 restatement of the ingest path (diffusynth_amd/ingest.py, csrc/resample_poly.hip) and its float32 twin.

The definition is scipy.signal.resample_poly(x, up, down) with its defaults, in closed form (include/diffusynth_hip.h);
tests/test_ingest_cpu.py pins this file to the real scipy function.  numpy only.

  g = gcd(orig_sr, target_sr), up = target_sr / g, down = orig_sr / g, HALF = 10 max(up, down), fc = 1 / max(up, down)
  h[k] = up s[k] w[k] / sum(s w),  s[k] = fc sinc(fc (k - HALF)),  w[k] = I0(5 sqrt(1 - ((k - HALF) / HALF)^2)) / I0(5),  0 <= k <= 2 HALF
  y[m] = sum_n x[n] h[HALF + m down - n up],  0 <= n < N, tap index in [0, 2 HALF],  0 <= m < ceil(N up / down)

dtype=np.float32 is the twin: the fp32-rounded taps, every product and every sum rounded to fp32, in the kernel's order (ascending tap index).
"""
import math

import numpy as np


def rate_pair(orig_sr, target_sr):
    g = math.gcd(orig_sr, target_sr)
    up, down = target_sr // g, orig_sr // g
    return up, down, 10 * max(up, down)


def design_filter(up, down):
    half = 10 * max(up, down)
    fc = 1.0 / max(up, down)
    k = np.arange(2 * half + 1, dtype=np.float64)
    arg = fc * (k - half)
    s = np.ones_like(arg)
    nz = arg != 0
    s[nz] = np.sin(np.pi * arg[nz]) / (np.pi * arg[nz])
    s *= fc
    w = np.i0(5.0 * np.sqrt(np.clip(1.0 - ((k - half) / half) ** 2, 0.0, None))) / np.i0(5.0)
    return up * s * w / np.sum(s * w)


def resampled_length(n, up, down):
    return (n * up + down - 1) // down


def resample(x, up, down, dtype=np.float64, taps=None):
    """y[0 : ceil(N up / down)] in `dtype` arithmetic.  taps: the filter to use (default: design_filter rounded to dtype)."""
    half = 10 * max(up, down)
    h = (design_filter(up, down) if taps is None else np.asarray(taps)).astype(dtype)
    assert h.size == 2 * half + 1
    x = np.asarray(x).astype(dtype)
    n_in = len(x)
    m = np.arange(resampled_length(n_in, up, down), dtype=np.int64)
    t = half + m * down
    q, p = t // up, t % up
    acc = np.zeros(len(m), dtype=dtype)
    for j in range(2 * half // up + 1):                   # tap p + j up meets sample q - j
        k, n = p + j * up, q - j
        ok = (k <= 2 * half) & (n >= 0) & (n < n_in)
        acc[ok] = acc[ok] + x[n[ok]] * h[k[ok]]
    return acc


def fix_length(y, n):
    out = np.zeros(n, dtype=y.dtype)
    out[:min(n, len(y))] = y[:n]
    return out


def resample_fit(x, orig_sr, target_sr, length=None, dtype=np.float64, taps=None):
    """adjust_audio_length: resample unless the rates are equal, then crop or zero-pad to `length` (None: as it comes)."""
    up, down, _ = rate_pair(orig_sr, target_sr)
    y = np.asarray(x).astype(dtype) if (up, down) == (1, 1) else resample(x, up, down, dtype, taps)
    return y if length is None else fix_length(y, length)


def upload_width(duration, time_resolution=256, VAE_scale=4):
    return int(time_resolution * ((duration + 1) / 4) / VAE_scale)


def upload_length(duration, time_resolution=256, VAE_scale=4):
    return 256 * (VAE_scale * upload_width(duration, time_resolution, VAE_scale) - 1)


def peak_normalize(x, dtype=np.float64):
    """x / max|x| of the upload converted to fp32 first (the package's first step), in `dtype` arithmetic."""
    x = np.asarray(x).astype(np.float32).astype(dtype)
    return x / np.max(np.abs(x))


def ingest(uploads, duration, sample_rate=16000, time_resolution=256, VAE_scale=4, dtype=np.float64):
    """The fitted (B, L) audio of uploads_to_stft."""
    n = upload_length(duration, time_resolution, VAE_scale)
    return np.stack([resample_fit(peak_normalize(s, dtype), sr, sample_rate, n, dtype) for sr, s in uploads])


def probe_signal(n, seed):
    """A few partials under a decaying envelope plus a little noise, peak below 1: energy up to the Nyquist frequency of any rate."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    y = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in zip((0.5, 0.3, 0.2, 0.1), (0.0113, 0.0771, 0.2031, 0.4377), rng.uniform(0, 6.28, 4)))
    y = y * np.exp(-t / max(n, 1) * 1.5) + 0.05 * rng.standard_normal(n)
    return (0.8 * y / max(np.max(np.abs(y)), 1e-9)).astype(np.float32)
