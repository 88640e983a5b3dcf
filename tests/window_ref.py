"""Numpy restatement of windowed sampling (diffusynth_amd/windowed.py, csrc/window.hip): the plan, the split and the blend, in fp32,
one rounded operation at a time, in table order — and RefWindowed, which calls the model once per window with one row and blends on
the host.  Written from the method's description, not from the package's code: the plan here is built window by window."""
import math

import numpy as np
import torch

MAXM = 8


def window_weights(window, weights="hann"):
    if isinstance(weights, str):
        if weights == "hann":
            return np.array([math.sin(math.pi * (c + 0.5) / window) ** 2 for c in range(window)], dtype=np.float64)
        assert weights == "uniform"
        return np.ones(window, dtype=np.float64)
    return np.asarray(weights, dtype=np.float64)


def plan(W, window, stride, loop=False, weights="hann"):
    """(offsets, entries): entries[x] = [(window j, source column c, fp32 coefficient), ...] ascending in j."""
    wt = window_weights(window, weights)
    if loop:
        offsets = [j * stride for j in range(math.ceil(W / stride))]
    else:
        offsets = [min(j * stride, W - window) for j in range(math.ceil((W - window) / stride) + 1)]
    under = [[] for _ in range(W)]
    for j, o in enumerate(offsets):
        for c in range(window):
            x = o + c
            if loop:
                x %= W
            assert 0 <= x < W
            under[x].append((j, c))
    entries = []
    for x in range(W):
        total = sum(float(wt[c]) for _, c in under[x])                  # float64
        entries.append([(j, c, np.float32(float(wt[c]) / total)) for j, c in sorted(under[x])])
    return offsets, entries


def split(x, offsets, window):
    """x (R, C, H, W) -> (R, n, C, H, window): window j of row r holds the columns (offsets[j] + c) mod W."""
    W = x.shape[-1]
    return np.stack([x[..., [(o + c) % W for c in range(window)]] for o in offsets], axis=1)


def merge(eps, entries):
    """eps (R, n, C, H, w) fp32 -> (R, C, H, W) fp32: per column the first product starts the sum, the others are added in order."""
    eps = np.asarray(eps, dtype=np.float32)
    R, _, Cc, H, _ = eps.shape
    out = np.empty((R, Cc, H, len(entries)), dtype=np.float32)
    for x, ent in enumerate(entries):
        acc = None
        for j, c, f in ent:
            t = np.float32(f) * eps[:, j, :, :, c]
            assert t.dtype == np.float32
            acc = t if acc is None else acc + t
        out[..., x] = acc
    return out


class RefWindowed:
    """The model's call contract: one model call per window, one row each, blended on the host (float32 numpy)."""
    cfg_paired_halves = False

    def __init__(self, model, window=64, stride=32, loop=False, weights="hann"):
        self.model, self.window, self.stride, self.loop, self.weights = model, window, stride, loop, weights

    def parameters(self):
        return self.model.parameters()

    @property
    def _engine(self):
        return getattr(self.model, "_engine", None)

    def __call__(self, x, time, condition=None):
        W = x.shape[-1]
        if W <= self.window and not self.loop:
            return self.model(x, time, condition)
        offsets, entries = plan(W, self.window, self.stride, self.loop, self.weights)
        rows = []
        for r in range(x.shape[0]):
            wins = []
            for o in offsets:
                cols = torch.tensor([(o + c) % W for c in range(self.window)], device=x.device)
                e = self.model(x[r:r + 1][..., cols].contiguous(), time[r:r + 1], None if condition is None else condition[r:r + 1])
                wins.append(e[0].cpu().numpy())
            rows.append(np.stack(wins))
        return torch.from_numpy(merge(np.stack(rows), entries)).to(x.device)
