"""Float64 restatement of guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4),
written from its definition, not from diffusynth_amd.  Per sample (row) of N elements, guidance scale s, rescale phi in [0, 1]:

    e   = eps_u + s (eps_c - eps_u)
    g   = phi std(eps_c) / std(e) + (1 - phi)        std over the row, unbiased (N - 1); std(e) == 0 -> the ratio is 1
    out = g e

numpy only.  Rows are the first axis; everything behind it is the row.
"""
import numpy as np


def case_inputs(B, chw, off, seed=0):
    """The kernel test's data: eps_u ~ N(off, 1), eps_c = eps_u + 0.3 N(0, 1), float32 [B][chw].  off = 100 puts the mean a hundred
    standard deviations from zero: a variance taken as E[x^2] - mean^2 in fp32 loses four digits there."""
    rng = np.random.default_rng([seed, B, chw, int(off)])
    u = (off + rng.standard_normal((B, chw))).astype(np.float32)
    c = (u + 0.3 * rng.standard_normal((B, chw))).astype(np.float32)
    return u, c


def combine(eps_u, eps_c, s, dtype=np.float64):
    """e in ``dtype``; with float32 the three operations are rounded one by one, as the step kernels round them."""
    u, c = np.asarray(eps_u, dtype=dtype), np.asarray(eps_c, dtype=dtype)
    d = c - u
    sd = dtype(s) * d
    return u + sd


def row_std(a):
    """Unbiased standard deviation of every row, in float64 about the float64 mean."""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    return np.sqrt(((a - a.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / max(a.shape[1] - 1, 1))


def gain(e, eps_c, phi):
    """g per row from the combined e and the conditional eps."""
    se, sc = row_std(e), row_std(eps_c)
    ratio = np.where(se > 0, sc / np.where(se > 0, se, 1.0), 1.0)
    return float(phi) * ratio + (1.0 - float(phi))


def rescale(eps_u, eps_c, s, phi, combine_dtype=np.float64):
    """(out, g) in float64; ``combine_dtype=np.float32`` takes e as the device forms it (three fp32 operations) and does the rest in
    float64."""
    e = combine(eps_u, eps_c, s, combine_dtype).astype(np.float64)
    g = gain(e, eps_c, phi)
    return g.reshape((-1,) + (1,) * (e.ndim - 1)) * e, g
