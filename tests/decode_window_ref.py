"""Float64 restatement of windowed decoding (diffusynth_amd/windowed.py WindowedDecoder / WindowedEncoder, csrc/stft_window.hip,
ds_istft_plus_loop): the frame plan, the blend of decoded windows on the complex spectrum, the circular inverse STFT, and the windowed
encoder as one call per window.  Written from the method's description on top of tests/window_ref.py (plans built window by window)
and oracle/vocoder_ref.py (decode_stft, the linear iSTFT), not from the package's code."""
import numpy as np
import torch

import window_ref as R
from oracle import vocoder_ref as V


def frame_plan(W, window, stride, loop, up, weights="hann"):
    """The plan of the ``up * W`` frames of a width-``W`` latent: everything times ``up``, an array of weights repeated."""
    wt = weights if isinstance(weights, str) else np.repeat(np.asarray(weights, dtype=np.float64), up)
    return R.plan(up * W, up * window, up * stride, loop, wt)


def decode(enc):
    """(..., 3, F, T) [log1p|D|, cos, sin] -> complex128 (..., F, T); the pair need not be of unit length, (0, 0) has phase 0."""
    e = np.moveaxis(np.asarray(enc, dtype=np.float64), -3, 0)
    return V.decode_stft(e)


def spectrum(rep):
    """The complex spectrum the tests compare on, expm1(out0) * (out1, out2), as (..., F, T, 2) float64."""
    o = torch.as_tensor(rep).double()
    return torch.stack([torch.expm1(o[..., 0, :, :]) * o[..., 1, :, :], torch.expm1(o[..., 0, :, :]) * o[..., 2, :, :]], dim=-1)


def encode(z):
    """complex (..., F, T) -> (..., 3, F, T) float64 [log1p|z|, z / |z|]; (0, 1, 0) for a zero, as tools.encode_stft gives."""
    mag = np.abs(z)
    safe = np.where(mag > 0, mag, 1.0)
    return np.stack([np.log1p(mag), np.where(mag > 0, z.real / safe, 1.0), np.where(mag > 0, z.imag / safe, 0.0)], axis=-3)


def stft_merge(encw, entries):
    """encw (R, n, 3, F, w) -> float64 (R, 3, F, T): decode, blend, re-encode.  A frame under one window is that window's frame as it
    is; a frame under several is the encoding of the coefficient-weighted sum of their decoded frames."""
    encw = np.asarray(encw, dtype=np.float64)
    d = decode(encw)                                                # (R, n, F, w)
    out = np.zeros((encw.shape[0], 3, encw.shape[3], len(entries)))
    for x, ent in enumerate(entries):
        if len(ent) == 1:
            out[..., x] = encw[:, ent[0][0], :, :, ent[0][1]]
        else:
            out[..., x] = encode(sum(float(f) * d[:, j, :, c] for j, c, f in ent)[..., None])[..., 0]
    return out


def istft_loop(D, hop=256, with_wss=False):
    """The inverse STFT of T frames on a circle of hop * T samples: D (1 + n_fft / 2, T) complex -> one period, float64.  Frame t is
    centred on sample t * hop; periodic Hann, overlap-add modulo the period, division by the window's sum of squares."""
    n_fft, T = 2 * (D.shape[0] - 1), D.shape[1]
    period = hop * T
    win = V.hann_periodic(n_fft)
    sig = np.fft.irfft(D, n=n_fft, axis=0) * win[:, None]
    y, wss = np.zeros(period), np.zeros(period)
    for t in range(T):
        idx = (t * hop - n_fft // 2 + np.arange(n_fft)) % period
        np.add.at(y, idx, sig[:, t])
        np.add.at(wss, idx, win ** 2)
    return (y / wss, wss) if with_wss else y / wss


def windowed_encode(encoder, x, window, stride, loop, down, weights="hann"):
    """One encoder call per window, one row each, blended on the host in fp32 (window_ref.RefWindowed's pattern).  x (B, 3, F, T)."""
    T = x.shape[-1]
    foff, _ = frame_plan(T // down, window, stride, loop, down, weights)
    _, entries = R.plan(T // down, window, stride, loop, weights)
    rows = []
    for r in range(x.shape[0]):
        wins = []
        for o in foff:
            cols = torch.tensor([(o + c) % T for c in range(down * window)], device=x.device)
            wins.append(encoder(x[r:r + 1][..., cols].contiguous())[0].cpu().numpy())
        rows.append(np.stack(wins))
    return torch.from_numpy(R.merge(np.stack(rows), entries))
