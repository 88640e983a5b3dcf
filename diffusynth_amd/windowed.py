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

The VQGAN was trained at the same width.  ``WindowedDecoder(decoder)`` decodes the windows of a long latent as one batch and blends them
on the complex spectrum (ds_stft_window_merge), and with ``loop=True`` the vocoder overlap-adds the frames around the circle
(ds_istft_plus_loop): the audio is one period without a seam.  ``WindowedEncoder(encoder)`` is the way back, for editing and
inpainting a long sound.

    audio = latents_to_audio(WindowedDecoder(vae._decoder, loop=True), q)         # (B, 256 * 4 * W): repeats without a click
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


class _Windowed(nn.Module):
    """What the wrappers share: the arguments and their checks, the plans per width (``plan(W, scale)``: the plan of the ``scale`` times
    finer axis — the frames of a latent column), their device tables, the row layouts, the split and the linear blend."""

    def __init__(self, inner, name, window, stride, loop, weights, max_rows):
        super().__init__()
        if isinstance(inner, nn.Module):
            setattr(self, name, inner)
        else:
            object.__setattr__(self, name, inner)       # (any callable with the call contract)
        self.window, self.stride, self.loop = int(window), int(stride), bool(loop)
        self.weights = weights if isinstance(weights, str) else _weights(weights, self.window)
        if max_rows is not None and int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1 or None, got %r" % (max_rows,))
        self.max_rows = None if max_rows is None else int(max_rows)
        window_plan(max(2 * self.window, self.window + 1), self.window, self.stride, self.loop, self.weights)      # the argument checks, now
        self._plans, self._tables, self._layouts = {}, {}, {}

    # ------------------------------------------------------------------ plans
    def windowed(self, W):
        return self.loop or int(W) > self.window

    def plan(self, W, scale=1):
        """The plan of a width of ``W`` columns, or with ``scale`` > 1 of its ``scale * W`` frames: window and stride are scaled, "hann" and
        "uniform" are evaluated at that resolution and an array of weights is repeated, so that the offsets are ``scale`` times the
        column plan's and a column's frames lie under that column's windows."""
        W, scale = int(W), int(scale)
        p = self._plans.get((W, scale))
        if p is None:
            wt = self.weights if isinstance(self.weights, str) else np.repeat(self.weights, scale)
            p = self._plans[(W, scale)] = window_plan(scale * W, scale * self.window, scale * self.stride, self.loop, wt)
        return p

    def rows_per_sample(self, W):
        """Rows of the wrapped module one row of a width-``W`` call takes: the number of windows, or 1 for a pass-through."""
        return self.plan(W).n if self.windowed(W) else 1

    def _column_tables(self, plan, dev):
        """(wcol [MAXM][W][2] int32, wcoef [MAXM][W] fp32) on ``dev``: ds_window_merge's layout, entry-major."""
        key = (plan.W, plan.window, dev)
        t = self._tables.get(key)
        if t is None:
            wcol = np.ascontiguousarray(np.stack([plan.win.T, plan.col.T], axis=2))
            t = self._tables[key] = (torch.from_numpy(wcol).to(dev), torch.from_numpy(np.ascontiguousarray(plan.coef.T)).to(dev))
        return t

    def _layout(self, plan, B, paired, dev):
        key = (plan.W, plan.window, B, paired, dev)
        t = self._layouts.get(key)
        if t is None:
            lay = _Layout(plan, B, paired, self.max_rows)
            src = torch.from_numpy(lay.src)
            t = self._layouts[key] = (lay, torch.from_numpy(lay.rows).to(dev), torch.from_numpy(lay.erow).to(dev), src, src.to(dev))
        return t

    # ------------------------------------------------------------------ split / call / blend
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

    @staticmethod
    def _call_chunks(lay, call):
        """``call(a, b)``: the wrapped module on the window rows [a, b).  One call, or one per chunk gathered into one fp32 buffer."""
        if len(lay.chunks) == 1:
            return call(0, lay.Rw).contiguous().float()
        out = None
        for a, b in lay.chunks:
            e = call(a, b)
            if out is None:
                out = torch.empty((lay.Rw,) + tuple(e.shape[1:]), dtype=torch.float32, device=e.device)
            out[a:b] = e
        return out

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
        for m, xt, vals, coef in _entries(eps, plan, lay):
            term = (vals * coef[None, :, None, None]).permute(0, 2, 3, 1)
            out[:, :, :, xt] = term if m == 0 else out[:, :, :, xt] + term
        return out


def _entries(eps, plan, lay):
    """The CPU walk of a plan's tables: for m = 0, 1, ... (entry m of every column that has one) the columns ``xt``, the windows' values
    there ``vals`` (B, nx, C, H) and the coefficients ``coef`` (nx,)."""
    erow = torch.from_numpy(lay.erow.astype(np.int64))
    for m in range(MAXM):
        xs = np.nonzero(plan.win[:, m] >= 0)[0]
        if len(xs) == 0:
            break
        rows = erow[:, torch.from_numpy(plan.win[xs, m].astype(np.int64))]                  # (B, nx)
        cols = torch.from_numpy(plan.col[xs, m].astype(np.int64))
        yield m, torch.from_numpy(xs), eps[rows, :, :, cols[None, :].expand_as(rows)], torch.from_numpy(plan.coef[xs, m])


class WindowedUnet(_Windowed):
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
        super().__init__(model, "model", window, stride, loop, weights, max_rows)

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
        part = lambda t, a, b: None if t is None else t[a:b]                                                         # noqa: E731
        eps = self._call_chunks(lay, lambda a, b: self.model(xw[a:b], part(tw, a, b), part(cw, a, b), **kw))
        return self._merge(eps, plan, lay, erow_dev, B, W)


# ---------------------------------------------------------------------------------------------------- the audio end
def _stft_decode_cpu(e):
    """(..., 3) fp32 STFT+ values -> (re, im): stft_codec.hpp's decode in torch fp32 (phase 0 for a (0, 0) or non-finite pair)."""
    mag, c, s = torch.expm1(e[..., 0]), e[..., 1], e[..., 2]
    nrm = torch.sqrt(c * c + s * s)
    ok = (nrm > 0) & torch.isfinite(nrm)
    one = torch.ones_like(nrm)
    return mag * torch.where(ok, c / torch.where(ok, nrm, one), one), mag * torch.where(ok, s / torch.where(ok, nrm, one), torch.zeros_like(nrm))


class WindowedDecoder(_Windowed):
    """A VQGAN decoder that never sees a latent wider than it was trained at, and whose output can loop.
    ``forward(q)``: ``(B, C, H, W)`` quantised latents -> ``(B, 3, 4H, up * W)`` STFT+ representation (``up`` = the decoder's output
    frames per latent column, read from its output; 4 in production).
      * ``W <= window`` without ``loop``: ``decoder(q)`` itself.
      * Otherwise the latent is cut by ``plan(W)`` (ds_window_split), the decoder runs once on the ``B * n`` window rows (with
        ``max_rows`` in chunks of at most that many), and the decoded windows are blended by the frame plan ``plan(W, up)`` on the
        complex spectrum (ds_stft_window_merge): (log1p|D|, cos, sin) is no linear space, the spectrum is, and overlap-add is linear in
        it.  A frame under one window keeps the decoder's bits.  The result is in the decoder's own format: the images and the iSTFT read
        it as they are.
    ``loop`` is read by the audio helpers of ``vocoder`` (``latents_to_audio`` ...): with ``loop=True`` they overlap-add the frames
    around the circle (ds_istft_plus_loop) and return one period of ``hop * up * W`` samples.
    Passed on to the decoder: ``parameters()``, ``set_compute_dtype``, ``cfg``.  On CPU tensors split and blend are torch fp32 code over
    the same tables in the same order (for tests with a stub decoder; the decoder itself runs on the GPU only)."""

    def __init__(self, decoder, window=64, stride=32, loop=False, weights="hann", max_rows=None):
        super().__init__(decoder, "decoder", window, stride, loop, weights, max_rows)

    @property
    def cfg(self):
        return self.decoder.cfg

    def set_compute_dtype(self, name):
        self.decoder.set_compute_dtype(name)
        return self

    def _merge_stft(self, encw, fplan, lay, erow_dev, B):
        Rw, three, F, w = encw.shape
        T = fplan.W
        out = torch.empty((B, 3, F, T), dtype=torch.float32, device=encw.device)
        if encw.is_cuda:
            wcol, wcoef = self._column_tables(fplan, encw.device)
            p = L.StftWindowMergeParams(encw=encw.data_ptr(), out=out.data_ptr(), erow=erow_dev.data_ptr(), wcol=wcol.data_ptr(),
                                        wcoef=wcoef.data_ptr(), R=B, n=fplan.n, F=F, T=T, w=w, Bw=Rw, Bout=B)
            with torch.cuda.device(encw.device):
                L.call("ds_stft_window_merge", C.byref(p), L.current_stream())
            return out
        zr, zi = torch.empty((B, F, T)), torch.empty((B, F, T))
        for m, xt, vals, coef in _entries(encw, fplan, lay):        # vals (B, nx, 3, F)
            vals = vals.permute(0, 3, 1, 2)                         # (B, F, nx, 3)
            if m == 0:
                out[:, :, :, xt] = vals.permute(0, 3, 1, 2)         # one entry: the window's bits
            re, im = _stft_decode_cpu(vals)
            tr, ti = re * coef[None, None, :], im * coef[None, None, :]
            zr[:, :, xt], zi[:, :, xt] = (tr, ti) if m == 0 else (zr[:, :, xt] + tr, zi[:, :, xt] + ti)
        many = torch.from_numpy(np.nonzero(fplan.cover > 1)[0])
        zr, zi = zr[:, :, many], zi[:, :, many]
        mag = torch.sqrt(zr * zr + zi * zi)
        pos, one = mag > 0, torch.ones_like(mag)
        safe = torch.where(pos, mag, one)
        out[:, 0, :, many], out[:, 1, :, many], out[:, 2, :, many] = torch.log1p(mag), torch.where(pos, zr / safe, one), torch.where(pos, zi / safe, one - 1)
        return out

    @torch.no_grad()
    def forward(self, q):
        B, _, _, W = q.shape
        if not self.windowed(W):
            return self.decoder(q)
        plan = self.plan(W)
        lay, rows_dev, erow_dev, _, _ = self._layout(plan, B, False, q.device)
        qw = self._split(q.contiguous().float(), plan, lay, rows_dev)
        encw = self._call_chunks(lay, lambda a, b: self.decoder(qw[a:b]))
        if encw.dim() != 4 or encw.shape[1] != 3 or encw.shape[-1] % self.window:
            raise ValueError("the decoder turned windows of %d columns into %r: not (rows, 3, F, a multiple of %d)" % (self.window, tuple(encw.shape), self.window))
        return self._merge_stft(encw, self.plan(W, encw.shape[-1] // self.window), lay, erow_dev, B)


class WindowedEncoder(_Windowed):
    """The mirror image: a VQGAN encoder on a long (or, with ``loop=True``, periodic in its frame axis) STFT+ representation.  ``window``
    and ``stride`` are in LATENT columns.  ``forward(stft_plus)``: ``(B, 3, F, T)`` -> ``(B, emb, F / 4, T / down)`` (``down`` = frames per
    latent column, read from the encoder's output on the first call — that call is at full width —; 4 in production; ``T`` must be a
    multiple of it): the representation is cut by the frame plan ``plan(T / down, down)`` (ds_window_split), the encoder runs once on
    the window rows (``max_rows``: in chunks) and the latents are blended by ``plan(T / down)`` (ds_window_merge) — before the quantiser,
    where the blend is linear.  ``T / down <= window`` without ``loop``: ``encoder(stft_plus)`` itself.  Passed on: ``parameters()``,
    ``set_compute_dtype``, ``cfg``.  CPU tensors: as for WindowedUnet."""

    def __init__(self, encoder, window=64, stride=32, loop=False, weights="hann", max_rows=None):
        super().__init__(encoder, "encoder", window, stride, loop, weights, max_rows)
        self._down = None

    @property
    def cfg(self):
        return self.encoder.cfg

    def set_compute_dtype(self, name):
        self.encoder.set_compute_dtype(name)
        return self

    @torch.no_grad()
    def forward(self, x):
        B, _, _, T = x.shape
        z = None
        if self._down is None:
            z = self.encoder(x)
            if z.shape[-1] < 1 or T % z.shape[-1]:
                raise ValueError("the encoder turned %d frames into %d columns: not a whole number of frames per column" % (T, z.shape[-1]))
            self._down = T // z.shape[-1]
        down = self._down
        if T % down:
            raise ValueError("%d frames are no multiple of the encoder's %d frames per latent column" % (T, down))
        W = T // down
        if not self.windowed(W):
            return z if z is not None else self.encoder(x)
        plan, fplan = self.plan(W), self.plan(W, down)
        lay, rows_dev, erow_dev, _, _ = self._layout(fplan, B, False, x.device)
        xw = self._split(x.contiguous().float(), fplan, lay, rows_dev)
        zw = self._call_chunks(lay, lambda a, b: self.encoder(xw[a:b]))
        if zw.dim() != 4 or zw.shape[-1] != self.window:
            raise ValueError("the encoder turned windows of %d frames into %r: not %d columns" % (fplan.window, tuple(zw.shape), self.window))
        return self._merge(zw, plan, lay, erow_dev, B, W)
