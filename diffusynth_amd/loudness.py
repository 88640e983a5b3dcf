"""K-weighted gated loudness (BS.1770) on the device: loudness() measures a 1-D CUDA tensor, a (B, L) tensor or a ragged list of 1-D
tensors, each signal by itself, with ds_loudness (include/diffusynth_hip.h, "loudness", has the arithmetic; DESIGN §7q the launch structure).
master() uses the same measurement for Mastering(target_lufs=...).

The host's part is the coefficients: kweighting() re-derives the two biquads for the sample rate in float64, and _coefficients() adds the
powers of the recursion's one-sample transition matrix that the kernels' exact carry needs.  Mono only; no loudness range (true peak: diffusynth_amd/true_peak.py)."""
import collections
import functools
import itertools
import math

import numpy as np
import torch

from . import _lib as L

_LU = L.LU
ABSOLUTE_GATE_LUFS = -70.0
Z_ABS = 10.0 ** ((ABSOLUTE_GATE_LUFS + 0.691) / 10.0)
MAX_SAMPLE_RATE = 10 * _LU["DS_LU_MAX_HOP"] + 4        # the largest rate whose 100 ms hop the kernels stage


class Loudness(collections.namedtuple("Loudness", "integrated momentary_max threshold blocks gated")):
    """Per signal, as device tensors (reading them is the caller's copy): the integrated loudness, the largest momentary (400 ms) loudness
    and the relative gate's threshold in LUFS (float64; -inf where there is nothing to measure), the number of 400 ms blocks and the number
    that passed both gates (int32)."""
    __slots__ = ()


def check_sample_rate(sample_rate, who="loudness"):
    if not isinstance(sample_rate, (int, np.integer)) or isinstance(sample_rate, (bool, np.bool_)) or sample_rate < 8000:
        raise ValueError(f"{who}: sample_rate must be an int >= 8000, not {sample_rate!r}")
    if sample_rate > MAX_SAMPLE_RATE:
        raise ValueError(f"{who}: sample_rate {sample_rate} above {MAX_SAMPLE_RATE} (a hop of at most {_LU['DS_LU_MAX_HOP']} samples)")
    return int(sample_rate)


def hop(sample_rate):
    """The 100 ms hop in samples, libebur128's rounding."""
    return (int(sample_rate) + 5) // 10


def energy_of(lufs):
    """The mean-square energy of a loudness: 10^((lufs + 0.691) / 10)."""
    return 10.0 ** ((float(lufs) + 0.691) / 10.0)


def kweighting(sample_rate):
    """((b, a) of the shelf, (b, a) of the high-pass): float64 arrays of three values each, a[0] = 1."""
    fs = float(check_sample_rate(sample_rate, "kweighting"))
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0], np.float64)
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    d = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0], np.float64)
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d], np.float64)
    return (b1, a1), (b2, a2)


def chunking(h):
    """(Lc, nc, Lt): a hop of h samples as nc chunks of Lc samples, the last of Lt; the kernels derive the same from h."""
    lc = -(-h // _LU["DS_LU_THREADS"]) | 1
    nc = -(-h // lc)
    return lc, nc, h - (nc - 1) * lc


def transition(sample_rate):
    """The one-sample zero-input transition of the state (s1[0], s1[1], s2[0], s2[1]) of the two transposed-form biquads."""
    (b1, a1), (b2, a2) = kweighting(sample_rate)
    return np.array([[-a1[1], 1.0, 0.0, 0.0],
                     [-a1[2], 0.0, 0.0, 0.0],
                     [b2[1] - a2[1] * b2[0], 0.0, -a2[1], 1.0],
                     [b2[2] - a2[2] * b2[0], 0.0, -a2[2], 0.0]], np.float64)


@functools.lru_cache(maxsize=16)
def _coefficients(sample_rate):
    """ds_loudness's coef for a rate (host memory, DS_LU_NCOEF float64), computed once."""
    (b1, a1), (b2, a2) = kweighting(sample_rate)
    h = hop(sample_rate)
    lc, _, lt = chunking(h)
    m = transition(sample_rate)
    c = np.zeros(_LU["DS_LU_NCOEF"], np.float64)
    c[_LU["DS_LU_C_B1"]:_LU["DS_LU_C_B1"] + 3] = b1
    c[_LU["DS_LU_C_A1"]:_LU["DS_LU_C_A1"] + 2] = a1[1:]
    c[_LU["DS_LU_C_B2"]:_LU["DS_LU_C_B2"] + 3] = b2
    c[_LU["DS_LU_C_A2"]:_LU["DS_LU_C_A2"] + 2] = a2[1:]
    c[_LU["DS_LU_C_PTAIL"]:_LU["DS_LU_C_PTAIL"] + 16] = np.linalg.matrix_power(m, lt).reshape(-1)
    c[_LU["DS_LU_C_PHOP"]:_LU["DS_LU_C_PHOP"] + 16] = np.linalg.matrix_power(m, h).reshape(-1)
    p = np.linalg.matrix_power(m, lc)
    for k in range(_LU["DS_LU_SCAN_STEPS"]):
        o = _LU["DS_LU_C_PSCAN"] + 16 * k
        c[o:o + 16] = p.reshape(-1)
        p = p @ p
    c.setflags(write=False)
    return c


def layout(tab, lengths, h):
    """Lay the signals' block energies out back to back: sets the table's BOFF column (HOST table, before its upload) -> (offsets, counts)."""
    nbs = [max(0, n // h - 3) for n in lengths]
    boffs = [0] + list(itertools.accumulate(nbs))[:-1]
    tab[:, _LU["DS_LU_TAB_BOFF"]] = boffs
    return boffs, nbs


def measure(x, dtab, lengths, sample_rate, blocks_layout=None):
    """ds_loudness on a flat fp32 CUDA tensor x and its uploaded table -> (lu [n][DS_LU_NS] float64, cnt [n][3] int32, block energies or
    None); blocks_layout: layout()'s result for the table, where the block energies are wanted."""
    h = hop(sample_rate)
    n, max_len = len(lengths), max(lengths)
    dev = x.device
    ws = torch.empty(L.load().ds_loudness_ws_bytes(n, max_len, h) // 8, dtype=torch.float64, device=dev)
    lu = torch.empty((n, _LU["DS_LU_NS"]), dtype=torch.float64, device=dev)
    cnt = torch.empty((n, 3), dtype=torch.int32, device=dev)
    total_blocks = max(1, sum(blocks_layout[1])) if blocks_layout else 0
    blocks = torch.empty(total_blocks, dtype=torch.float64, device=dev) if blocks_layout else None
    L.call("ds_loudness", x.data_ptr(), dtab.data_ptr(), n, max_len, x.numel(), _coefficients(sample_rate).ctypes.data, h, Z_ABS, ws.data_ptr(), lu.data_ptr(),
           cnt.data_ptr(), L.ptr(blocks), total_blocks, L.current_stream())
    return lu, cnt, blocks


def result(lu, cnt, blocks=None, where=None, single=False):
    """Loudness of measure()'s outputs; with blocks the momentary loudness curve per signal, -0.691 + 10 log10 z_j (a list, or one tensor
    for a single signal)."""
    res = Loudness(lu[:, _LU["DS_LU_INTEGRATED"]], lu[:, _LU["DS_LU_MOMENTARY_MAX"]], lu[:, _LU["DS_LU_THRESHOLD"]], cnt[:, 0], cnt[:, 2])
    if blocks is None:
        return res
    curve = -0.691 + 10.0 * torch.log10(blocks)
    curves = [curve[o:o + m] for o, m in zip(*where)]
    return res, (curves[0] if single else curves)


@torch.no_grad()
def loudness(signals, sample_rate=16000, *, return_blocks=False):
    """Integrated loudness (BS.1770: K-weighting, 400 ms blocks every 100 ms, absolute gate at -70 LUFS, relative gate 10 LU below the mean
    of what passed it) of one 1-D CUDA tensor, a (B, L) tensor or a list of 1-D tensors of different lengths, each signal by itself ->
    Loudness; with return_blocks=True (Loudness, momentary loudness curve per signal).  One table upload, ds_loudness, no device -> host
    copy.  A signal's result is the same bits alone and in a batch.  Mono; this package's re-derived coefficients at rates other than
    48 kHz (libebur128's and pyloudnorm's form)."""
    from . import arranger as A
    sample_rate = check_sample_rate(sample_rate)
    sigs, lengths, single, _ = A._signals_of(signals, "loudness")
    tab = A._flat_table(lengths)
    where = layout(tab, lengths, hop(sample_rate)) if return_blocks else None
    x = sigs[0] if len(sigs) == 1 else torch.cat(sigs)
    dtab = torch.from_numpy(tab.reshape(-1)).to(x.device)
    lu, cnt, blocks = measure(x, dtab, lengths, sample_rate, where)
    return result(lu, cnt, blocks, where, single)
