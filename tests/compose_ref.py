"""Restatement of weighted multi-prompt guidance, written from its definition, not from diffusynth_amd.  Per sample (one row of
N = C H W elements, column j = i mod W), unconditional eps u, conditional eps c_1 ... c_K, weights a_k(j) (a scalar per condition, or
one value per latent column), guidance scale S and rescale phi in [0, 1]:

    d_k = c_k - u
    acc = a_1(j) d_1 + a_2(j) d_2 + ... + a_K(j) d_K       ascending k, starting from the first product
    p   = u + acc
    e   = u + S acc
    g   = phi std(p) / std(e) + (1 - phi)                  std over the row; std(e) == 0 -> the ratio is 1; phi == 0 -> g = 1
    out = g e                                              phi == 0: out is e itself

numpy only.  u is [B][N], c is [K][B][N]; the statistics are guidance_ref's (float64 about the float64 mean).
"""
import numpy as np

import guidance_ref as G


def case_inputs(B, chw, off, K, seed=0):
    """The kernel test's data: guidance_ref.case_inputs' u, and K conditionals drawn the way it draws its one:
    c_k = u + 0.3 N(0, 1), float32.  Returns u [B][chw], c [K][B][chw]."""
    u, _ = G.case_inputs(B, chw, off, seed)
    c = np.empty((K, B, chw), np.float32)
    for k in range(K):
        rng = np.random.default_rng([seed, B, chw, int(off), 1 + k])
        c[k] = (u + 0.3 * rng.standard_normal((B, chw))).astype(np.float32)
    return u, c


def case_weights(K, W=None, seed=0):
    """(K,) weights — or a (K, W) envelope — in [-0.7, 1.3), float32; from K = 2 on the second condition's are negative."""
    rng = np.random.default_rng([seed, K, 0 if W is None else W])
    a = rng.uniform(-0.7, 1.3, (K,) if W is None else (K, W)).astype(np.float32)
    if K > 1:
        a[1] = -np.abs(a[1])
    return a


def per_element(wt, N, W):
    """a_k of every element of a row: [K][N] (column j = i mod W)."""
    wt = np.asarray(wt)
    if wt.ndim == 1:
        return np.repeat(wt[:, None], N, axis=1)
    assert wt.shape[1] == W and N % W == 0
    return np.tile(wt, (1, N // W))


def mix(eps_u, eps_c, wt, W, s, dtype=np.float64):
    """(p, e) in ``dtype``; with float32 every operation is rounded on its own, in the stated order."""
    u, c = np.asarray(eps_u, dtype=dtype), np.asarray(eps_c, dtype=dtype)
    a = per_element(wt, u.shape[1], W).astype(dtype)
    acc = None
    for k in range(c.shape[0]):
        d = c[k] - u
        t = a[k][None, :] * d
        acc = t if acc is None else acc + t
    p = u + acc
    sa = dtype(s) * acc
    return p, u + sa


def compose(eps_u, eps_c, wt, W, s, phi, combine_dtype=np.float64):
    """(out, g) in float64; ``combine_dtype=np.float32`` takes p and e as the device forms them and does the rest in float64."""
    p, e = mix(eps_u, eps_c, wt, W, s, combine_dtype)
    p, e = p.astype(np.float64), e.astype(np.float64)
    if float(phi) == 0.0:
        return e, np.ones(len(e))
    g = G.gain(e, p, phi)
    return g[:, None] * e, g
