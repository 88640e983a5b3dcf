"""Pitch detection on the GPU: YIN per frame of a ragged batch (ds_yin_frames), the lower median of each signal's voiced periods
(ds_pitch_median), and the note they name.  What the arranger's tuned mode (arranger.Track.render(tune="detect")) asks where a note
actually sits, instead of assuming MIDI 52.

Everything floored — tau_min, tau_max, the frame counts — is computed here on the host in integers and handed to the kernels as a table;
f0 and the MIDI number are computed on the host in float64 from the median period, which is one of the frames' fp32 periods bit for bit.
No CPU fallback.
"""
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L

_YIN = L.YIN
MAX_FRAMES = L.PITCH_MAX_FRAMES


class PitchEstimate(NamedTuple):
    """Per signal of the batch: f0 in Hz and the MIDI number 69 + 12 log2(f0 / 440) (float64 numpy; nan for an unpitched signal), the voiced
    and the total frame counts (int64 numpy) and the median period in samples (float64 numpy: the fp32 value of one frame, 0 if none)."""
    f0: np.ndarray
    midi: np.ndarray
    voiced: np.ndarray
    frames: np.ndarray
    period: np.ndarray


def _taus(sample_rate, fmin, fmax, frame_length, hop_length, threshold):
    """Validated (frame_length, hop, tau_min, tau_max): ValueError naming the argument, before any device work."""
    if not (isinstance(frame_length, (int, np.integer)) and 1 <= frame_length <= _YIN["DS_YIN_MAX_W"]):
        raise ValueError(f"frame_length: an integer in [1, {_YIN['DS_YIN_MAX_W']}] (got {frame_length!r})")
    if not (isinstance(hop_length, (int, np.integer)) and hop_length >= 1):
        raise ValueError(f"hop_length: a positive integer (got {hop_length!r})")
    if not (isinstance(threshold, (int, float, np.floating)) and 0.0 < float(threshold) < 1.0 and float(np.float32(threshold)) < 1.0):
        raise ValueError(f"threshold: a number in (0, 1) (got {threshold!r})")
    if not (sample_rate > 0 and math.isfinite(sample_rate)):
        raise ValueError(f"sample_rate: a positive number (got {sample_rate!r})")
    if not (isinstance(fmin, (int, float, np.number)) and math.isfinite(fmin) and fmin > 0 and sample_rate // fmin <= _YIN["DS_YIN_MAX_TAU"]):
        raise ValueError(f"fmin: sample_rate // fmin must be at most {_YIN['DS_YIN_MAX_TAU']} samples (got fmin={fmin!r} at {sample_rate} Hz)")
    tau_max = int(sample_rate // fmin)
    if not (isinstance(fmax, (int, float, np.number)) and math.isfinite(fmax) and fmax > 0 and max(2, int(sample_rate / fmax)) < tau_max):
        raise ValueError(f"fmax: max(2, sample_rate / fmax) must lie below sample_rate // fmin = {tau_max} (got fmax={fmax!r})")
    return int(frame_length), int(hop_length), max(2, int(sample_rate / fmax)), tau_max


def frame_count(n, frame_length, tau_max, hop):
    """Frames of a signal of n samples: frame i reads [i hop, i hop + frame_length + tau_max)."""
    return max(0, (n - frame_length - tau_max) // hop + 1)


class _Batch:
    """The signals back to back, their table on the device (ONE upload) and the frames of one ds_yin_frames launch."""

    def __init__(self, signals, what, params, frame_limit=None):
        from .arranger import _as_list
        self.W, self.hop, self.tau_min, self.tau_max = params
        self.sigs, self.was_tensor = _as_list(signals, what)
        self.lengths = [s.numel() for s in self.sigs]
        self.frames = [frame_count(n, self.W, self.tau_max, self.hop) for n in self.lengths]
        if frame_limit is not None and self.frames and max(self.frames) > frame_limit:
            raise ValueError(f"signals: a signal of {max(self.lengths)} samples has {max(self.frames)} frames (at most {frame_limit}); raise hop_length")
        self.n = len(self.sigs)
        tab = np.zeros((self.n, _YIN["DS_YIN_NI"]), dtype=np.int64)
        tab[:, _YIN["DS_YIN_LEN"]], tab[:, _YIN["DS_YIN_NF"]] = self.lengths, self.frames
        tab[1:, _YIN["DS_YIN_XOFF"]], tab[1:, _YIN["DS_YIN_FOFF"]] = np.cumsum(self.lengths)[:-1], np.cumsum(self.frames)[:-1]
        self.total_samples, self.total_frames = int(sum(self.lengths)), int(sum(self.frames))
        if self.total_samples >= 2 ** 31:
            raise ValueError(f"signals: {self.total_samples} samples in one batch (at most 2^31 - 1)")
        self.foff = tab[:, _YIN["DS_YIN_FOFF"]].tolist()
        self.host_tab = tab.astype(np.int32)
        self.tab = self.x = self.out = None

    def run_frames(self, threshold):
        """-> the (2, total_frames) fp32 tensor [period; aperiodicity].  Nothing is launched when no signal has a frame."""
        dev = self.sigs[0].device if self.sigs else torch.device("cuda")
        self.out = torch.empty((2, self.total_frames), dtype=torch.float32, device=dev)
        if self.total_frames == 0:
            return self.out
        self.x = self.sigs[0] if self.n == 1 else torch.cat(self.sigs)
        self.tab = torch.from_numpy(self.host_tab.reshape(-1)).to(dev)
        L.call("ds_yin_frames", self.x.data_ptr(), self.tab.data_ptr(), self.n, max(self.frames), self.total_samples, self.total_frames, self.W, self.hop,
               self.tau_min, self.tau_max, float(threshold), self.out[0].data_ptr(), self.out[1].data_ptr(), L.current_stream())
        return self.out


@torch.no_grad()
def yin(signals, sample_rate=16000, fmin=55.0, fmax=1000.0, frame_length=1024, hop_length=256, threshold=0.1):
    """YIN per frame.  signals: a (B, L) CUDA tensor or a list of 1-D CUDA tensors of different lengths (arranger.pitch_shift's conventions
    and errors) -> for a tensor the pair (period, aperiodicity) of (B, n_frames) fp32 CUDA tensors, for a list one such pair of 1-D tensors
    per signal.  period is in samples (f0 = sample_rate / period), 0 for an unvoiced frame (aperiodicity 1: no tau in
    [tau_min, tau_max) = [max(2, int(sample_rate / fmax)), int(sample_rate // fmin)) has a normalised difference under `threshold`).
    A signal has max(0, (len - frame_length - tau_max) // hop_length + 1) frames.  One table upload, one launch."""
    params = _taus(sample_rate, fmin, fmax, frame_length, hop_length, threshold)
    b = _Batch(signals, "yin", params)
    out = b.run_frames(threshold)
    if b.was_tensor:
        return out[0].view(b.n, -1), out[1].view(b.n, -1)
    return [(out[0, o:o + f], out[1, o:o + f]) for o, f in zip(b.foff, b.frames)]


@torch.no_grad()
def estimate_pitch(signals, sample_rate=16000, fmin=55.0, fmax=1000.0, frame_length=1024, hop_length=256, threshold=0.1, min_voiced=0.25):
    """The pitch of every signal of a batch (same forms as yin): the lower median of its voiced frames' periods -> PitchEstimate.  A signal
    without frames, or with fewer than min_voiced * frames voiced ones (noise, percussion, silence), is unpitched: f0 = midi = nan.
    Two launches and ONE device -> host copy (a period and a count per signal) for the whole batch; a signal may have at most
    MAX_FRAMES frames."""
    params = _taus(sample_rate, fmin, fmax, frame_length, hop_length, threshold)
    if not (isinstance(min_voiced, (int, float, np.floating)) and 0.0 <= float(min_voiced) <= 1.0):
        raise ValueError(f"min_voiced: a share in [0, 1] (got {min_voiced!r})")
    b = _Batch(signals, "estimate_pitch", params, frame_limit=MAX_FRAMES)
    frames = np.array(b.frames, dtype=np.int64)
    med, voiced = np.zeros(b.n, np.float64), np.zeros(b.n, np.int64)
    out = b.run_frames(threshold)
    if b.total_frames > 0:
        res = torch.empty((2, b.n), dtype=torch.int32, device=out.device)      # [median period (fp32 bits); voiced count]
        L.call("ds_pitch_median", out[0].data_ptr(), b.tab.data_ptr(), b.n, max(b.frames), b.total_frames, res[0].data_ptr(), res[1].data_ptr(),
               L.current_stream())
        host = res.cpu().numpy()
        med, voiced = host[0].view(np.float32).astype(np.float64), host[1].astype(np.int64)
    pitched = (frames > 0) & (voiced > 0) & (voiced >= float(min_voiced) * frames)
    f0 = np.full(b.n, np.nan)
    f0[pitched] = float(sample_rate) / med[pitched]
    midi = np.full(b.n, np.nan)
    midi[pitched] = 69.0 + 12.0 * np.log2(f0[pitched] / 440.0)
    return PitchEstimate(f0, midi, voiced, frames, med)
