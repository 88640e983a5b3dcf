"""Restatement of text-guided editing by "edit-friendly" DDPM inversion (Huberman-Spiegelglas et al., 2024), written from the
definitions and not from diffusynth_amd.  On a respaced schedule with indices 0 ... N - 1 (the state in front of step i sits at
a_t = alphas_cumprod[i], step i goes to a_p = alphas_cumprod_prev[i]) and start = int(N * strength):

    X_i  = sqrt(a_i) x0 + sqrt(1 - a_i) n_i                      i = start - 1 ... 0, independent noises;  X_{-1} = x0
    cf   = sqrt(1 - a_t), sqrt(a_t), sqrt(a_p), sqrt(1 - a_p - sigma^2), sigma      sigma = sqrt((1 - a_p) / (1 - a_t)) sqrt(1 - a_t / a_p)
    e    = guided eps at (X_i, i)       x^ = (X_i - cf0 e) / cf1       mu = cf2 x^ + cf3 e
    z_i  = (X_{i-1} - mu) / cf4         i = start - 1 ... 1;  z_0 = 0 (cf4 == 0 there)
    step:  x_{i-1} = (cf2 x^ + cf3 e) + cf4 z_i                  the eta = 1 ("ddpm") step with z_i in place of the drawn noise

Everything takes a ``dtype``: numpy rounds every operation of an expression on its own, so dtype=float32 is the form with one rounded
fp32 operation at a time (in the order written here) and dtype=float64 the exact one.  The analytic model is the exact noise
prediction for data N(m, s^2) per element, m the mean of the sample's condition row.
"""
import numpy as np


# ------------------------------------------------------------------------------------------------ coefficients
def coefficients(acp, acp_prev, n):
    """[n][5] float64, row i: the eta = 1 step from index i."""
    a_t, a_p = np.asarray(acp[:n], dtype=np.float64), np.asarray(acp_prev[:n], dtype=np.float64)
    sig = np.sqrt((1 - a_p) / (1 - a_t)) * np.sqrt(1 - a_t / a_p)
    return np.stack([np.sqrt(1 - a_t), np.sqrt(a_t), np.sqrt(a_p), np.sqrt(np.maximum(1 - a_p - sig ** 2, 0.0)), sig], axis=1)


def table_f32(acp, acp_prev, n):
    """The rows as the device receives them: the same expressions by torch's CPU fp32 operations on the fp32-rounded a_t, a_p (torch's
    fp32 sqrt is not numpy's everywhere)."""
    import torch
    a_t = torch.from_numpy(np.asarray(acp[:n], dtype=np.float64)).float()
    a_p = torch.from_numpy(np.asarray(acp_prev[:n], dtype=np.float64)).float()
    sig = 1.0 * torch.sqrt((1 - a_p) / (1 - a_t)) * torch.sqrt(1 - a_t / a_p)
    return torch.stack([torch.sqrt(1. - a_t), torch.sqrt(a_t), torch.sqrt(a_p), torch.sqrt(1 - a_p - sig ** 2), sig], dim=1).numpy()


def q_coefficients(acp, n, dtype=np.float64):
    """[n][2]: sqrt(a_i), sqrt(1 - a_i), float64 rounded once to ``dtype``."""
    a = np.asarray(acp[:n], dtype=np.float64)
    return np.stack([np.sqrt(a), np.sqrt(1 - a)], axis=1).astype(dtype)


# ------------------------------------------------------------------------------------------------ one operation at a time, fp32
def guided_f32(eps, eps_c, scale):
    f = np.float32
    eps = np.asarray(eps, dtype=f)
    if eps_c is None:
        return eps
    d = np.asarray(eps_c, dtype=f) - eps
    sd = f(scale) * d
    return eps + sd


def q_sample_f32(x0, noise, q0, q1):
    f = np.float32
    g0 = f(q0) * np.asarray(x0, dtype=f)
    g1 = f(q1) * np.asarray(noise, dtype=f)
    return g0 + g1


def edit_noise_f32(x, x_prev, eps, eps_c, scale, cf):
    """z of one row: every operation rounded on its own, in the order e, x^, u0, u1, mu, d, z.  cf[4] == 0: zeros."""
    f = np.float32
    x, x_prev = np.asarray(x, dtype=f), np.asarray(x_prev, dtype=f)
    cf = [f(v) for v in cf]
    if cf[4] == 0:
        return np.zeros_like(x)
    e = guided_f32(eps, eps_c, scale)
    t0 = cf[0] * e
    t1 = x - t0
    xh = t1 / cf[1]
    u0 = cf[2] * xh
    u1 = cf[3] * e
    mu = u0 + u1
    d = x_prev - mu
    z = d / cf[4]
    assert z.dtype == f
    return z


# ------------------------------------------------------------------------------------------------ analytic model
class Model:
    """eps = sqrt(1 - a) (x - sqrt(a) m) / (a s^2 + 1 - a), computed as (k1 (x - k3 m)) / k2 from tables rounded once to ``dtype``;
    ``a`` [n]: the cumulative alpha the model sees at index i (that of the full schedule at timestep_map[i])."""

    def __init__(self, a, s, dtype=np.float64):
        a = np.asarray(a, dtype=np.float64)
        self.dtype = dtype
        self.k1, self.k3, self.k2 = np.sqrt(1 - a).astype(dtype), np.sqrt(a).astype(dtype), (a * s * s + 1 - a).astype(dtype)

    def eps(self, x, i, m):
        """m: per sample, broadcastable to x (e.g. (B, 1, 1, 1))."""
        return (self.k1[i] * (x - self.k3[i] * np.asarray(m, dtype=self.dtype))) / self.k2[i]

    def guided(self, x, i, m, m_uncond=None, scale=1.0):
        """The step kernels' combine: e = u + scale (c - u), u the unconditional prediction."""
        c = self.eps(x, i, m)
        if m_uncond is None:
            return c
        u = self.eps(x, i, m_uncond)
        return u + self.dtype(scale) * (c - u)


def condition_means(cond):
    """m of every sample as (B, 1, 1, 1) float64 (a (D,) condition: one sample's)."""
    c = np.asarray(cond, dtype=np.float64)
    return c.mean(axis=-1).reshape(-1, 1, 1, 1)


class AnalyticDevice:
    """The model as a callable on the device: (k1[t] (x - k3[t] m)) / k2[t] from fp32 tables over the FULL schedule, one torch
    operation at a time — Model(dtype=float32)'s operations.  m = condition.mean(1): exact, and so the same as condition_means, when
    the rows hold multiples of 1/8 and D is 8."""

    def __init__(self, acp_full, s):
        import torch
        a = np.asarray(acp_full, dtype=np.float64)
        up = lambda v: torch.from_numpy(v.astype(np.float32)).cuda()                               # noqa: E731
        self.k1, self.k3, self.k2 = up(np.sqrt(1 - a)), up(np.sqrt(a)), up(a * s * s + 1 - a)

    def __call__(self, x, t, condition=None):
        v = lambda k: k[t].view(-1, 1, 1, 1)                                                      # noqa: E731
        m = 0.0 if condition is None else condition.float().mean(dim=1).view(-1, 1, 1, 1)
        return (v(self.k1) * (x - v(self.k3) * m)) / v(self.k2)


# ------------------------------------------------------------------------------------------------ inversion and replay
def q_states(x0, noises, acp, start, dtype=np.float64):
    """X[i] for i = 0 ... start - 1; noises[k] belongs to index start - 1 - k (the order they are drawn in)."""
    q = q_coefficients(acp, start, dtype)
    x0 = np.asarray(x0, dtype=dtype)
    return [q[i, 0] * x0 + q[i, 1] * np.asarray(noises[start - 1 - i], dtype=dtype) for i in range(start)]


def invert(X, tab, eps_of):
    """z in step order (z[k] belongs to index start - 1 - k; the last one is zeros) from the states X[0 ... start - 1]; tab [start][5]
    in the dtype of the arithmetic; eps_of(x, i): the guided eps."""
    start, z = len(X), []
    for i in range(start - 1, 0, -1):
        cf, e = tab[i], eps_of(X[i], i)
        xh = (X[i] - cf[0] * e) / cf[1]
        mu = cf[2] * xh + cf[3] * e
        z.append((X[i - 1] - mu) / cf[4])
    z.append(np.zeros_like(X[0]))
    return z


def replay(x_start, z, tab, eps_of):
    """The states x_start, then after every step of start - 1 ... 0 with z[k] in place of the drawn noise (start + 1 entries)."""
    start, x = len(z), x_start
    out = [x]
    for k in range(start):
        i = start - 1 - k
        cf, e = tab[i], eps_of(x, i)
        xh = (x - cf[0] * e) / cf[1]
        x = (cf[2] * xh + cf[3] * e) + cf[4] * z[k]
        out.append(x)
    return out


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def reconstruction_error(states, X):
    """The largest relative distance of replayed state k to the inverted X_{start-1-k}, k < start."""
    start = len(X)
    return max(rel_err(states[k], X[start - 1 - k]) for k in range(start))
