"""Windowed sampling for long and looping sounds (MultiDiffusion, Bar-Tal et al. 2023; with weights: Mixture of Diffusers).

The U-Net was trained at width 64.  ``WindowedUnet(model)`` is a model with the model's call contract that never shows the U-Net a
wider latent: a call on a ``(B, C, H, W)`` state cuts it into ``n`` overlapping windows of the trained width (ds_window_split), runs the
noise predictor on all ``B * n`` windows as one batch — the regime the card is most efficient in — and blends the
predictions back with a partition of unity (ds_window_merge).  With ``loop=True`` the windows wrap around the time axis, so the seam
of a loop is an ordinary interior column.

Merging eps is merging the stepped states: for a fixed state every sampler of this package is linear (affine) in eps — "ddim", "ddpm"
(whose step noise is shared by the windows: it belongs to the full-width state) and "dpmpp_2m" (its history is a linear function of
earlier eps) — and the blend's coefficients sum to one in every column, so stepping each window with its own eps and blending the
results equals blending the eps and stepping once.  Guidance, guidance rescale and the condition mix therefore run unchanged on the
blended, full-width tensors, and so do the sampler, the batcher and serving: a wrapper is all they see.

    net = WindowedUnet(unet, window=64, stride=32)                # or loop=True
    imgs, _ = DiffSynthSampler(..., max_width=1024, noise_strategy="non_repeat").sample(net, (1, 4, 128, 1024), condition=c)
"""
import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib as L

MAXM = L.WM["DS_WM_MAXM"]


class WindowPlan:
    """What ``window_plan`` returns: ``n`` windows of ``window`` columns at ``offsets`` (window j holds the columns
    ``(offsets[j] + c) mod W``), and for every output column x its covering windows ``win[x, m]`` (ascending, -1 padded), their source
    columns ``col[x, m]`` and blend coefficients ``coef[x, m]`` (fp32; 0 in the padding), ``cover[x]`` of them."""

    def __init__(self, W, window, stride, loop, offsets, win, col, coef):
        self.W, self.window, self.stride, self.loop = W, window, stride, loop
        self.offsets, self.win, self.col, self.coef = offsets, win, col, coef
        self.n = len(offsets)
        self.cover = (win >= 0).sum(axis=1)


def _weights(weights, window):
    if isinstance(weights, str):
        if weights == "hann":
            return np.sin(np.pi * (np.arange(window, dtype=np.float64) + 0.5) / window) ** 2
        if weights == "uniform":
            return np.ones(window, dtype=np.float64)
        raise ValueError("weights must be 'hann', 'uniform' or a positive (window,) array, got %r" % (weights,))
    try:
        w = np.array(weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("weights must be 'hann', 'uniform' or a positive (window,) array, got %r" % (weights,)) from None
    if w.shape != (window,):
        raise ValueError("weights must have shape (%d,), got %r" % (window, w.shape))
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError("weights must be finite and positive")
    return w


def window_plan(W, window=64, stride=32, loop=False, weights="hann"):
    """The windows of a width-``W`` latent and their partition of unity (host only).
    Non-loop (``W > window``): ``n = ceil((W - window) / stride) + 1`` windows at ``min(j * stride, W - window)`` — the last one is
    pulled back inside.  Loop (``W >= window``): ``n = ceil(W / stride)`` windows at ``j * stride``, columns taken mod W.
    ``weights``: the window function — "hann" (``sin^2(pi (c + 0.5) / window)``, strictly positive), "uniform", or a positive
    ``(window,)`` array.  The coefficient of window j in column x is its weight there over the sum of the weights of the windows
    that cover x, computed in float64 and rounded once to fp32: a column under one window has exactly 1.0.
    ``ValueError``: ``stride < 1`` or ``> window``, a column under more than DS_WM_MAXM windows, weights that are not positive and
    finite, a loop with ``W < window``, a non-loop with ``W <= window`` (there is nothing to cut)."""
    W, window, stride, loop = int(W), int(window), int(stride), bool(loop)
    if window < 1:
        raise ValueError("window must be >= 1, got %d" % window)
    if stride < 1 or stride > window:
        raise ValueError("stride must be in [1, window=%d], got %d" % (window, stride))
    wt = _weights(weights, window)
    if loop:
        if W < window:
            raise ValueError("a loop of width %d is narrower than the window of %d" % (W, window))
        offsets = np.arange(-(-W // stride), dtype=np.int64) * stride
    else:
        if W <= window:
            raise ValueError("a width of %d fits one window of %d: there is nothing to cut" % (W, window))
        offsets = np.minimum(np.arange(-(-(W - window) // stride) + 1, dtype=np.int64) * stride, W - window)
    n = len(offsets)
    rel = (np.arange(W)[:, None] - offsets[None, :]) % W if loop else np.arange(W)[:, None] - offsets[None, :]      # (W, n)
    covers = (rel >= 0) & (rel < window)
    cover = covers.sum(axis=1)
    if cover.max() > MAXM:
        raise ValueError("a column lies under %d windows, more than DS_WM_MAXM=%d: use a larger stride" % (cover.max(), MAXM))
    assert cover.min() >= 1
    win = np.full((W, MAXM), -1, dtype=np.int32)
    col = np.zeros((W, MAXM), dtype=np.int32)
    coef = np.zeros((W, MAXM), dtype=np.float32)
    for x in range(W):
        js = np.nonzero(covers[x])[0]                   # ascending
        cs = rel[x, js]
        ws = wt[cs]
        win[x, :len(js)], col[x, :len(js)] = js, cs
        coef[x, :len(js)] = (ws / ws.sum()).astype(np.float32)
    return WindowPlan(W, window, stride, loop, offsets.astype(np.int32), win, col, coef)


class _Layout:
    """The row tables of one (batch, paired) call shape: where the windows lie in the window batch, chunk by chunk."""

    def __init__(self, plan, B, paired, max_rows):
        n = plan.n
        Rw = B * n
        # window batch row of (input row r, window j), in the order the model sees the rows
        if max_rows is None or Rw <= max_rows:
            self.chunks = [(0, Rw)]
            order = np.arange(Rw)                       # (input row, window): the halves of a paired batch stay halves
        elif paired:
            per = int(max_rows) // 2
            if per < 1:
                raise ValueError("max_rows=%d is less than the two rows of a paired call" % max_rows)
            half = Rw // 2
            self.chunks, order, pos = [], [], 0
            for a in range(0, half, per):               # the same windows from both halves
                b = min(a + per, half)
                order += list(range(a, b)) + list(range(half + a, half + b))
                self.chunks.append((pos, pos + 2 * (b - a)))
                pos += 2 * (b - a)
            order = np.asarray(order)
        else:
            self.chunks = [(a, min(a + int(max_rows), Rw)) for a in range(0, Rw, int(max_rows))]
            order = np.arange(Rw)
        # order[d] = r * n + j of the window at batch row d
        self.src = (order // n).astype(np.int64)        # input row of batch row d (its time, its condition)
        rows = np.zeros((Rw, L.WS["DS_WS_NI"]), dtype=np.int32)
        rows[:, L.WS["DS_WS_SRC"]] = order // n
        rows[:, L.WS["DS_WS_OFF"]] = plan.offsets[order % n]
        rows[:, L.WS["DS_WS_DST"]] = np.arange(Rw)
        self.rows = rows
        erow = np.zeros(Rw, dtype=np.int32)
        erow[order] = np.arange(Rw)                     # erow[r * n + j]: the batch row of window j of input row r
        self.erow = erow.reshape(B, n)
        self.Rw = Rw


class WindowedUnet(nn.Module):
    """See the module docstring.  ``forward(x, time, condition=None, paired_halves=False)`` is the model's contract.
      * ``W <= window`` without ``loop``: ``model(...)`` itself — short sounds cost nothing extra.
      * Otherwise ``n = rows_per_sample(W)`` windows per row (``window_plan``), in the order (input row, window): the halves of a paired
        (classifier-free guidance) batch stay halves, and ``paired_halves=True`` is passed on.  ``time`` and ``condition`` of a row are
        repeated over its windows.  One model call, or with ``max_rows`` several of at most that many rows (a paired batch then takes
        the same windows from both halves), their results gathered into one buffer for the blend.
    Plans are cached per width and their device tables per (width, device) (the row tables per batch and pairing as well): nothing
    blocking is uploaded per step.  On CPU tensors split and blend are torch code that walks the same tables in the same order with
    separate multiplies and adds (for tests with a stub model; the U-Net itself runs on the GPU only).
    What the sampler and the batcher ask of a model is passed on: ``parameters()``, ``cfg_paired_halves``, ``_engine``,
    ``pin_launch_batch``, ``set_compute_dtype``, ``use_hip_graph``."""

    def __init__(self, model, window=64, stride=32, loop=False, weights="hann", max_rows=None):
        super().__init__()
        if isinstance(model, nn.Module):
            self.model = model
        else:
            object.__setattr__(self, "model", model)    # (any callable with the call contract)
        self.window, self.stride, self.loop = int(window), int(stride), bool(loop)
        self.weights = weights if isinstance(weights, str) else _weights(weights, self.window)
        if max_rows is not None and int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1 or None, got %r" % (max_rows,))
        self.max_rows = None if max_rows is None else int(max_rows)
        window_plan(max(2 * self.window, self.window + 1), self.window, self.stride, self.loop, self.weights)      # the argument checks, now
        self._plans, self._tables, self._layouts = {}, {}, {}

    # ------------------------------------------------------------------ what callers ask of a model
    @property
    def cfg_paired_halves(self):
        return getattr(self.model, "cfg_paired_halves", False)

    @property
    def _engine(self):
        return getattr(self.model, "_engine", None)

    def pin_launch_batch(self, n):
        self.model.pin_launch_batch(n)
        return self

    def set_compute_dtype(self, name):
        self.model.set_compute_dtype(name)
        return self

    def use_hip_graph(self, on=True):
        self.model.use_hip_graph(on)
        return self

    # ------------------------------------------------------------------ plans
    def windowed(self, W):
        return self.loop or int(W) > self.window

    def plan(self, W):
        W = int(W)
        p = self._plans.get(W)
        if p is None:
            p = self._plans[W] = window_plan(W, self.window, self.stride, self.loop, self.weights)
        return p

    def rows_per_sample(self, W):
        """U-Net rows one row of a width-``W`` call takes: the number of windows, or 1 for a pass-through."""
        return self.plan(W).n if self.windowed(W) else 1

    def _column_tables(self, plan, dev):
        """(wcol [MAXM][W][2] int32, wcoef [MAXM][W] fp32) on ``dev``: ds_window_merge's layout, entry-major."""
        key = (plan.W, dev)
        t = self._tables.get(key)
        if t is None:
            wcol = np.ascontiguousarray(np.stack([plan.win.T, plan.col.T], axis=2))
            t = self._tables[key] = (torch.from_numpy(wcol).to(dev), torch.from_numpy(np.ascontiguousarray(plan.coef.T)).to(dev))
        return t

    def _layout(self, plan, B, paired, dev):
        key = (plan.W, B, paired, dev)
        t = self._layouts.get(key)
        if t is None:
            lay = _Layout(plan, B, paired, self.max_rows)
            src = torch.from_numpy(lay.src)
            t = self._layouts[key] = (lay, torch.from_numpy(lay.rows).to(dev), torch.from_numpy(lay.erow).to(dev), src, src.to(dev))
        return t

    # ------------------------------------------------------------------ split / blend
    def _split(self, x, plan, lay, rows_dev):
        B, Cc, H, W = x.shape
        xw = torch.empty((lay.Rw, Cc, H, plan.window), dtype=torch.float32, device=x.device)
        if x.is_cuda:
            p = L.WindowSplitParams(x=x.data_ptr(), out=xw.data_ptr(), rows=rows_dev.data_ptr(), R=lay.Rw, C=Cc, H=H, W=W, w=plan.window,
                                    Bx=B, Bout=lay.Rw)
            with torch.cuda.device(x.device):
                L.call("ds_window_split", C.byref(p), L.current_stream())
            return xw
        for src, off, dst in lay.rows:
            xw[dst] = x[src][:, :, torch.from_numpy((off + np.arange(plan.window)) % W)]
        return xw

    def _merge(self, eps, plan, lay, erow_dev, B, W):
        Rw, Cc, H, w = eps.shape
        out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=eps.device)
        if eps.is_cuda:
            wcol, wcoef = self._column_tables(plan, eps.device)
            p = L.WindowMergeParams(eps=eps.data_ptr(), out=out.data_ptr(), erow=erow_dev.data_ptr(), wcol=wcol.data_ptr(),
                                    wcoef=wcoef.data_ptr(), R=B, n=plan.n, C=Cc, H=H, W=W, w=w, Beps=Rw, Bout=B)
            with torch.cuda.device(eps.device):
                L.call("ds_window_merge", C.byref(p), L.current_stream())
            return out
        erow = torch.from_numpy(lay.erow.astype(np.int64))
        for m in range(MAXM):                           # entry m of every column that has one: a product, then (m > 0) a sum
            xs = np.nonzero(plan.win[:, m] >= 0)[0]
            if len(xs) == 0:
                break
            rows = erow[:, torch.from_numpy(plan.win[xs, m].astype(np.int64))]                  # (B, nx)
            cols = torch.from_numpy(plan.col[xs, m].astype(np.int64))
            vals = eps[rows, :, :, cols[None, :].expand_as(rows)]                               # (B, nx, C, H)
            term = (vals * torch.from_numpy(plan.coef[xs, m])[None, :, None, None]).permute(0, 2, 3, 1)
            xt = torch.from_numpy(xs)
            out[:, :, :, xt] = term if m == 0 else out[:, :, :, xt] + term
        return out

    @torch.no_grad()
    def forward(self, x, time, condition=None, paired_halves=False):
        kw = {"paired_halves": True} if paired_halves else {}
        B, _, _, W = x.shape
        if not self.windowed(W):
            return self.model(x, time, condition, **kw)
        if paired_halves and B % 2:
            raise ValueError("paired_halves=True needs an even batch")
        plan = self.plan(W)
        lay, rows_dev, erow_dev, src_cpu, src_dev = self._layout(plan, B, bool(paired_halves), x.device)
        x = x.contiguous().float()
        xw = self._split(x, plan, lay, rows_dev)
        pick = lambda t: None if t is None else t[src_dev if t.device == x.device else src_cpu.to(t.device)]       # noqa: E731
        tw, cw = pick(time), pick(condition)
        if len(lay.chunks) == 1:
            eps = self.model(xw, tw, cw, **kw).contiguous().float()
        else:
            eps = None
            for a, b in lay.chunks:
                e = self.model(xw[a:b], tw[a:b], None if cw is None else cw[a:b], **kw)
                if eps is None:
                    eps = torch.empty((lay.Rw,) + tuple(e.shape[1:]), dtype=torch.float32, device=e.device)
                eps[a:b] = e
        return self._merge(eps, plan, lay, erow_dev, B, W)
