"""numpy restatement of the true-peak meter and of the limiter with the envelope as its detector (include/diffusynth_hip.h, "true peak";
DESIGN §7r), in exactly the stated types: fp32 samples and table, float64 products (exact) and sums in ascending tap order, one rounding
per add (numpy's elementwise ufuncs are IEEE and do not contract), fp32 envelope and true peak.  Nothing here shares code with the
package.  The limiter is master_ref's hold_min, smooth and apply with step 2's detector swapped.

Defect models (each a wrong reading of the definition that a test must be able to tell from the right one): right_interval_only,
edges_clamped, half_sample_only, fp32_accumulate."""
import math

import numpy as np

import master_ref as M

F32 = np.float32
TAPS, PHASES, HALF = 12, 3, 24
DEFECTS = ("right_interval_only", "edges_clamped", "half_sample_only", "fp32_accumulate")


def tap(d):
    """c(d), float64."""
    if d == 0:
        return 1.0
    if abs(d) > HALF:
        return 0.0
    t = math.pi * d / 4.0
    return math.sin(t) / t * 0.5 * (1.0 + math.cos(2.0 * math.pi * d / 48.0))


def taps49():
    """c(-24 .. 24), float64."""
    return np.array([tap(d) for d in range(-HALF, HALF + 1)], np.float64)


def table():
    """h[p - 1][k] = fp32(c(4 (5 - k) + p)), p = 1, 2, 3, k = 0 .. 11."""
    return np.array([[tap(4 * (5 - k) + p) for k in range(TAPS)] for p in (1, 2, 3)], np.float64).astype(F32)


def padded(x, defect=None):
    """x over [-6, N + 6): zeros outside the signal (edges_clamped: its first and last sample repeated)."""
    x = np.asarray(x, F32)
    return np.pad(x, 6, mode="edge" if defect == "edges_clamped" else "constant")


def phases(x, defect=None, h=None):
    """v[p - 1][m] = v_p(m - 1), m = 0 .. N: float64 (fp32_accumulate: every product and sum rounded to fp32)."""
    h = table() if h is None else np.asarray(h, F32)
    xp = padded(x, defect)
    n = len(xp) - 12
    t = F32 if defect == "fp32_accumulate" else np.float64
    out = np.empty((PHASES, n + 1), t)
    for p in range(PHASES):
        acc = h[p, 0].astype(t) * xp[0:n + 1].astype(t)          # x[m - 1 - 5 + k] = xp[m + k]
        for k in range(1, TAPS):
            acc = acc + h[p, k].astype(t) * xp[k:k + n + 1].astype(t)
        out[p] = acc
    return out


def intersample(x, defect=None):
    """iv(m - 1), m = 0 .. N, float64."""
    v = np.abs(phases(x, defect).astype(np.float64))
    return v[1] if defect == "half_sample_only" else v.max(axis=0)


def envelope(x, defect=None):
    """e[n], fp32, n = 0 .. N - 1."""
    x = np.asarray(x, F32)
    iv = intersample(x, defect)
    e = np.maximum(np.abs(x).astype(np.float64), iv[1:])
    if defect != "right_interval_only":
        e = np.maximum(e, iv[:-1])
    return e.astype(F32)


def true_peak(x, defect=None):
    return F32(envelope(x, defect).max())


def db(v):
    return 20.0 * math.log10(float(v))


def oversampled(x):
    """The 4x waveform by the definition's other reading, float64: the zero-stuffed signal convolved with the 49 taps; entry 4 n + p is the
    value at time n + p / 4, for 4 n + p = -4 .. 4 N - 1 + 4 (index 0 is time -1)."""
    x = np.asarray(x, F32).astype(np.float64)
    z = np.zeros(4 * len(x), np.float64)
    z[::4] = x
    full = np.convolve(z, table_full())                          # full[i] is time (i - 24) / 4
    return full[HALF - 4:HALF + 4 * len(x) + 4]


def table_full():
    """The 49 taps with the three computed phases rounded to fp32 as the table is, the identity phase exact."""
    c = taps49()
    d = np.arange(-HALF, HALF + 1)
    c = c.astype(F32).astype(np.float64)
    c[d % 4 == 0] = 0.0
    c[HALF] = 1.0
    return c


# ---------------------------------------------------------------------------------------------------- the limiter
def required_tp(x, e, gl, c):
    """(u, r) of step 2 with the envelope as detector: d = fl(gL e), r = fl(c / d) where d > c."""
    x, e, gl, c = np.asarray(x, F32), np.asarray(e, F32), F32(gl), F32(c)
    u = (gl * x).astype(F32)
    d = (gl * e).astype(F32)
    over = d > c
    r = np.ones(len(x), F32)
    r[over] = (c / d[over]).astype(F32)
    return u, r


def master(x, A, R, *, gl=None, target_rms=0.1, max_gain=10.0, ceiling=M.DEFAULTS["ceiling"], detector="envelope"):
    """Steps 1-7 for one signal with the true-peak detector (detector="samples": master_ref.master) -> master_ref's dict plus env, tp_in and
    tp_out, the true peak of y."""
    x = np.asarray(x, F32)
    assert detector in ("envelope", "samples")
    if detector == "samples":
        out = M.master(x, A, R, gl=gl, target_rms=target_rms, max_gain=max_gain, ceiling=ceiling)
        out.update(env=envelope(x), tp_in=true_peak(x), tp_out=true_peak(out["y"]))
        return out
    assert x.ndim == 1 and len(x) >= 1 and 0 <= A <= R
    c = F32(ceiling)
    own, g64, rms, peak = M.gain(x, target_rms, max_gain)
    gl = own if gl is None else F32(gl)
    e = envelope(x)
    u, r = required_tp(x, e, gl, c)
    m = M.hold_min(r, A, R)
    g = M.smooth(m, A)
    y = M.apply(u, g, c)
    env_y = envelope(y)
    return dict(x=x, c=c, gain=gl, own_gain=own, gain64=g64, rms=rms, peak=peak, u=u, r=r, m=m, g=g, y=y, pcm=M.pcm16(y), min_gain=F32(min(g.min(), F32(1.0))),
                limited=int(np.count_nonzero(g < F32(1.0))), env=e, tp_in=F32(e.max()), tp_out=F32(env_y.max()))


# ---------------------------------------------------------------------------------------------------- the six signals of DESIGN §7r
def fixtures(sr=16000, n=16000):
    """name -> fp32 signal of 1 s: the inputs on which a sample-peak limiter leaves the true peak over the ceiling."""
    t = np.arange(n)
    rng = np.random.default_rng(7)
    quarter = np.sin(2 * np.pi * t / 4.0 + np.pi / 4.0)
    burst = np.where((t >= n // 4) & (t < n // 2), 2.0, 0.25) * quarter
    noise = np.clip(rng.standard_normal(n), -1.0, 1.0)
    square = 0.95 * np.where((t * 1000 // (sr // 2)) % 2 == 0, 1.0, -1.0)
    beat = 0.705 * (np.sin(2 * np.pi * 3900.0 * t / sr + np.pi / 8.0) + np.sin(2 * np.pi * 4100.0 * t / sr + np.pi / 8.0))
    a, r = M.samples(M.DEFAULTS["lookahead"], M.DEFAULTS["hold"], sr)
    return {"quarter_sine": (0.99 * quarter).astype(F32), "quarter_burst": burst.astype(F32), "clipped_noise": noise.astype(F32), "square_1k": square.astype(F32),
            "beat_4k": beat.astype(F32), "master_signal": M.signal(n, a, r)}
