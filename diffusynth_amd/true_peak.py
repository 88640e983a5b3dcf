"""True peak (BS.1770 Annex 2: the peak of the waveform between the samples, by 4x oversampling) on the device: true_peak() measures a
1-D CUDA tensor, a (B, L) tensor or a ragged list of 1-D tensors, each signal by itself, with ds_true_peak (include/diffusynth_hip.h,
"true peak", has the arithmetic; DESIGN §7r the launch structure).  master() uses the same kernel's envelope as the limiter's detector
for Mastering(true_peak=True).

The host's part is the interpolator: true_peak_coefficients() computes the three computed phases of libebur128's 49-tap Hann-windowed
sinc in float64 and rounds them to fp32 once.  Mono only; the factor is 4 at every rate."""
import collections
import functools
import math

import numpy as np
import torch

from . import _lib as L

_TP = L.TP


class TruePeak(collections.namedtuple("TruePeak", "input output")):
    """Per signal, as fp32 device tensors (reading them is the caller's copy): the true peak of master()'s input and of its fp32 result
    (before any int16 rounding), linear; dBTP = 20 log10 of it."""
    __slots__ = ()


def tap(d):
    """c(d) of the interpolator, float64: sinc(d / 4) (1 + cos(2 pi d / 48)) / 2 for |d| <= 24, 0 beyond."""
    if d == 0:
        return 1.0
    if abs(d) > 24:
        return 0.0
    t = math.pi * d / 4.0
    return math.sin(t) / t * 0.5 * (1.0 + math.cos(2.0 * math.pi * d / 48.0))


@functools.lru_cache(maxsize=1)
def true_peak_coefficients():
    """ds_true_peak's coef: the (3, 12) fp32 table h[p - 1][k] = fp32(c(4 (5 - k) + p)), p = 1, 2, 3 (host memory, read-only, computed once)."""
    h = np.array([[tap(4 * (5 - k) + p) for k in range(_TP["DS_TP_TAPS"])] for p in range(1, _TP["DS_TP_PHASES"] + 1)], np.float64).astype(np.float32)
    h.setflags(write=False)
    return h


def measure(x, dtab, lengths, want_envelope=False):
    """ds_true_peak on a flat fp32 CUDA tensor x and its uploaded table -> (tp [n] fp32, envelope [x.numel()] fp32 or None)."""
    n, max_len = len(lengths), max(lengths)
    dev = x.device
    ws = torch.empty(L.load().ds_true_peak_ws_bytes(n, max_len) // 4, dtype=torch.float32, device=dev)
    tp = torch.empty(n, dtype=torch.float32, device=dev)
    env = torch.empty(x.numel(), dtype=torch.float32, device=dev) if want_envelope else None
    L.call("ds_true_peak", x.data_ptr(), dtab.data_ptr(), n, max_len, x.numel(), true_peak_coefficients().ctypes.data, L.ptr(env), ws.data_ptr(), tp.data_ptr(),
           L.current_stream())
    return tp, env


@torch.no_grad()
def true_peak(signals, *, return_envelope=False):
    """The true peak (linear, fp32; 20 log10 of it is dBTP) of one 1-D CUDA tensor, a (B, L) tensor or a list of 1-D tensors of different
    lengths, each signal by itself, zero outside it -> an fp32 device tensor of one value per signal; with return_envelope=True
    (true peaks, envelopes in the input's container): e[n] is the largest magnitude of the 4x interpolated waveform on (n - 1, n + 1), so
    e >= |x| and the true peak is its maximum.  One table upload, ds_true_peak, no device -> host copy.  A signal's result is the same
    bits alone and in a batch."""
    from . import arranger as A
    if not isinstance(return_envelope, (bool, np.bool_)):
        raise ValueError(f"true_peak: return_envelope must be True or False, not {return_envelope!r}")
    sigs, lengths, single, was_tensor = A._signals_of(signals, "true_peak")
    tab = A._flat_table(lengths)
    x = sigs[0] if len(sigs) == 1 else torch.cat(sigs)
    dtab = torch.from_numpy(tab.reshape(-1)).to(x.device)
    tp, env = measure(x, dtab, lengths, bool(return_envelope))
    if not return_envelope:
        return tp
    if was_tensor:
        env = env.view(len(sigs), lengths[0])
    elif not single:
        env = [env[o:o + m] for o, m in zip(tab[:, L.PV["DS_PV_XOFF"]].tolist(), lengths)]
    return tp, env
