"""numpy restatement of the mastering stage (include/diffusynth_hip.h, "mastering"), steps 1-7 in exactly the stated types:
fp32 u, r, m, g, y; float64 squares and sums; the scalars rounded to fp32 once.  Nothing here shares code with the package.

The windowed minimum is van Herk / Gil-Werman over blocks of the window's length (the kernel doubles in place: another algorithm; a
minimum does not depend on either), the window sums are numpy's own over a strided view; tests/test_master_cpu.py holds both against the
two-line definitions on a small case and the sums against math.fsum."""
import math

import numpy as np

F32 = np.float32
DEFAULTS = dict(target_rms=0.1, max_gain=10.0, ceiling=10 ** (-1 / 20), lookahead=0.005, hold=0.05)


def samples(lookahead, hold, sample_rate=16000):
    """(A, R): the arranger's flooring."""
    return int(lookahead * sample_rate), int(hold * sample_rate)


def gain(x, target_rms, max_gain):
    """(gL fp32, gL float64 before its rounding, rms float64, peak fp32).  The sum of the exact float64 squares is math.fsum's: the true sum
    rounded once."""
    x = np.asarray(x, F32)
    rms = math.sqrt(math.fsum((x.astype(np.float64) ** 2).tolist()) / len(x))
    peak = F32(np.max(np.abs(x)))
    if target_rms is None:
        return F32(1.0), 1.0, rms, peak
    t, cap = float(F32(target_rms)), float(F32(max_gain))
    g64 = min(t / rms, cap) if rms > 0 else cap
    return F32(g64), g64, rms, peak


def required(x, gl, c):
    """(u, r) of step 2: fp32 product, IEEE fp32 division where |u| > c."""
    x, gl, c = np.asarray(x, F32), F32(gl), F32(c)
    u = (gl * x).astype(F32)
    au = np.abs(u)
    over = au > c
    r = np.ones(len(x), F32)
    r[over] = (c / au[over]).astype(F32)
    return u, r


def extend(r, A, R):
    """r over [-A - R, N - 1 + 2 A]: ones outside the signal."""
    e = np.ones(len(r) + R + 3 * A, F32)
    e[A + R:A + R + len(r)] = r
    return e


def hold_min(r, A, R):
    """m[j] = min r[j - R .. j + A] for j = -A .. N - 1 + A (N + 2 A values), van Herk / Gil-Werman."""
    e = extend(r, A, R)
    W = R + A + 1
    n_out = len(r) + 2 * A
    nblk = -(-len(e) // W)
    p = np.full(nblk * W, np.inf, F32)
    p[:len(e)] = e
    blocks = p.reshape(nblk, W)
    prefix = np.minimum.accumulate(blocks, axis=1).reshape(-1)
    suffix = np.minimum.accumulate(blocks[:, ::-1], axis=1)[:, ::-1].reshape(-1)
    j = np.arange(n_out)
    return np.minimum(suffix[j], prefix[j + W - 1])


def hold_min_by_definition(r, A, R):
    e = extend(r, A, R)
    return np.array([e[j:j + R + A + 1].min() for j in range(len(r) + 2 * A)], F32)


def window_sums(m, A):
    """float64 sums of m[n .. n + 2 A] (m indexed from j = -A), n = 0 .. N - 1."""
    return np.lib.stride_tricks.sliding_window_view(np.asarray(m, F32).astype(np.float64), 2 * A + 1).sum(axis=1)


def smooth(m, A):
    return (window_sums(m, A) / float(2 * A + 1)).astype(F32)


def apply(u, g, c):
    c = F32(c)
    y = (np.asarray(g, F32) * np.asarray(u, F32)).astype(F32)
    y = np.where(y > c, c, y)
    return np.where(y < -c, -c, y).astype(F32)


def pcm16(y):
    return np.rint(np.asarray(y, F32) * F32(32767)).astype(np.int16)


def master(x, A, R, *, gl=None, target_rms=0.1, max_gain=10.0, ceiling=DEFAULTS["ceiling"]):
    """Steps 1-7 for one signal -> dict.  gl: the gain to evaluate steps 2-7 at (None: this function's own fp32 gL)."""
    x = np.asarray(x, F32)
    assert x.ndim == 1 and len(x) >= 1 and 0 <= A <= R
    c = F32(ceiling)
    own, g64, rms, peak = gain(x, target_rms, max_gain)
    gl = own if gl is None else F32(gl)
    u, r = required(x, gl, c)
    m = hold_min(r, A, R)
    g = smooth(m, A)
    y = apply(u, g, c)
    return dict(x=x, c=c, gain=gl, own_gain=own, gain64=g64, rms=rms, peak=peak, u=u, r=r, m=m, g=g, y=y, pcm=pcm16(y), min_gain=F32(min(g.min(), F32(1.0))),
                limited=int(np.count_nonzero(g < F32(1.0))))


def ulps(a, b):
    """|a - b| in units of fp32 ulps of b, for a an fp32 value and b a float64 one (or both fp32)."""
    return abs(float(a) - float(b)) / float(np.spacing(F32(abs(float(b)))))


# ---------------------------------------------------------------------------------------------------- the test signal
def signal(n, A, R, *, ceiling=DEFAULTS["ceiling"], seed=0, tile=None, sr=16000, loud=2.5):
    """55 Hz plus noise at `loud`, every other stretch of R + 3 A + 37 samples quiet (1e-3 of it: longer than the limiter's reach, so the
    gain is back at exactly 1 inside), spikes of 2^9 c at sample 0, -0.75 2^9 c at the last, 300 c in the middle and, with `tile`, 100 c and
    -200 c at samples tile - 1 and tile.  With a gain of at most 2 this keeps |u| <= 2^10 c."""
    rng = np.random.default_rng(1000 * seed + n)
    t = np.arange(n)
    x = loud * np.sin(2 * np.pi * 55.0 * t / sr) + 0.1 * loud * rng.standard_normal(n)
    x = np.where((t // (R + 3 * A + 37)) % 2 == 1, 1e-3 * x, x)
    c = float(F32(ceiling))
    x[n // 2] = 300 * c
    if tile is not None and n > tile:
        x[tile - 1], x[tile] = 100 * c, -200 * c
    x[n - 1] = -0.75 * 2 ** 9 * c
    x[0] = 2 ** 9 * c
    return x.astype(F32)
