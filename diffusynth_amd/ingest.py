"""A user's sound into the model, on the GPU: sample-rate conversion, fit to the model's length, STFT.

Replaces the front of receive_upload_origin_audio (webUI/natural_language_guided_4/sound2sound_with_text.py:47-104 and
inpaint_with_text.py:67-115): `(sample_rate, samples)` as Gradio hands them over — any rate, int16 or float, any length — is peak-normalised
(ds_peak_normalize), resampled and cropped / zero-padded to 256 (VAE_scale width - 1) samples (tools.adjust_audio_length, tools.py:126-151:
ONE ds_resample_poly launch for the whole batch) and transformed (ds_stft_plus).  The result feeds vocoder.InputBatch2Encode_STFT.  The same
kernel converts outwards: 16 kHz results to 44.1 or 48 kHz.

Different on purpose: the resampler.  The reference calls librosa.resample with its default res_type, soxr_hq, a closed third-party design
(INTEGRATION.md §1).  adjust_audio_length in this package means librosa.resample(res_type="polyphase"), which is
scipy.signal.resample_poly(x, up, down) with its defaults (window ("kaiser", 5.0), padtype "constant"): a published definition, restated
in include/diffusynth_hip.h and pinned to scipy in tests/.  The arranger's ds_resample_sinc (irrational 2^(n/12) rates) is a different
kernel for a different input and is not used here.

The filters are designed here on the host in float64 with numpy alone, rounded to fp32 once per distinct (up, down), kept per device and
shared by every row of that pair; whatever is floored, ceiled or divided (gcd, NRES, the fit length, the outputs per block) is computed here
in integers.  No CPU fallback.
"""
import math

import numpy as np
import torch

from . import _lib as L
from .arranger import _as_list, _flat_table, _per_signal, _require_cuda

_RP = L.RP
MAX_TAPS, MAX_SPAN, MAX_BLK = _RP["DS_RP_MAX_TAPS"], _RP["DS_RP_MAX_SPAN"], _RP["DS_RP_MAX_BLK"]
SPAN_TARGET = 4096          # input samples a block stages (16 KB of LDS) unless one output alone needs more
_NO_GPU = "diffusynth_amd ingest runs on MI355X only (%s); no CPU fallback"


# ---------------------------------------------------------------------------------------------------- the definition, host side
def _check_rate(sr, what):
    if isinstance(sr, (bool, np.bool_)) or not isinstance(sr, (int, np.integer)) or sr <= 0:
        raise ValueError(f"{what}: a sample rate must be a positive int (got {sr!r})")
    return int(sr)


def rate_pair(orig_sr, target_sr):
    """(up, down, HALF) of orig_sr -> target_sr: up / down = target_sr / orig_sr in lowest terms, HALF = 10 max(up, down).  ValueError for
    rates that are not positive ints and for a pair whose 2 HALF + 1 taps exceed DS_RP_MAX_TAPS (no fallback to another resampler)."""
    orig_sr, target_sr = _check_rate(orig_sr, "orig_sr"), _check_rate(target_sr, "target_sr")
    g = math.gcd(orig_sr, target_sr)
    up, down = target_sr // g, orig_sr // g
    half = 10 * max(up, down)
    if 2 * half + 1 > MAX_TAPS:
        raise ValueError(f"resample_poly: {orig_sr} Hz -> {target_sr} Hz is {up}/{down} in lowest terms and needs {2 * half + 1} filter taps; "
                         f"at most {MAX_TAPS} are supported (resample to a rate with a smaller common ratio first)")
    return up, down, half


def design_filter(up, down):
    """scipy.signal.resample_poly's default filter, firwin(2 HALF + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up, in closed form and
    float64: h[k] = up s[k] w[k] / sum(s w), s[k] = fc sinc(fc (k - HALF)), w[k] = I0(5 sqrt(1 - ((k - HALF) / HALF)^2)) / I0(5)."""
    half = 10 * max(up, down)
    fc = 1.0 / max(up, down)
    t = np.arange(-half, half + 1, dtype=np.float64)
    s = fc * np.sinc(fc * t)
    w = np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (t / half) ** 2))) / np.i0(5.0)
    h = s * w
    return up * h / h.sum()


def resampled_length(n, up, down):
    """ceil(n up / down), in integers."""
    return -((-n * up) // down)


def upload_width(duration, time_resolution=256, VAE_scale=4):
    """The latent width of a sound of `duration` (the reference's int(time_resolution * ((duration + 1) / 4) / VAE_scale))."""
    return int(time_resolution * ((duration + 1) / 4) / VAE_scale)


def upload_length(duration, time_resolution=256, VAE_scale=4):
    """The samples that width stands for: 256 (VAE_scale width - 1)."""
    return 256 * (VAE_scale * upload_width(duration, time_resolution, VAE_scale) - 1)


def block_outputs(up, down, half):
    """(BLK, span): the outputs one block owns and the most input samples they can touch, ((BLK - 1) down + 2 HALF) // up + 2."""
    target = max(SPAN_TARGET, 2 * half // up + 2)
    blk = max(1, min(MAX_BLK, ((target - 2) * up - 2 * half) // down + 1))
    return blk, ((blk - 1) * down + 2 * half) // up + 2


class FilterBank:
    """The fp32 taps of every rate pair seen so far, back to back: one per distinct (up, down), on the host and (once asked) on one device."""

    def __init__(self):
        self.offsets, self.parts, self.total, self._dev, self._dev_total = {}, [], 0, None, -1

    def offset(self, up, down):
        """Where the pair's 2 HALF + 1 taps start (designed and rounded on first use)."""
        if (up, down) not in self.offsets:
            h = design_filter(up, down).astype(np.float32)
            self.offsets[(up, down)] = self.total
            self.parts.append(h)
            self.total += h.size
        return self.offsets[(up, down)]

    def taps(self, up, down):
        """The pair's fp32 taps as the kernel reads them."""
        o = self.offset(up, down)
        return self.host()[o:o + 20 * max(up, down) + 1]

    def host(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, np.float32)

    def device(self, dev):
        """The bank on `dev`; uploaded again only after a new pair was added."""
        if self._dev is None or self._dev_total != self.total:
            self._dev, self._dev_total = torch.from_numpy(self.host()).to(dev), self.total
        return self._dev


_BANKS = {}


def filter_bank(device):
    """The FilterBank of a CUDA device."""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _BANKS:
        _BANKS[key] = FilterBank()
    return _BANKS[key]


class _Plan:
    """Host side of one ds_resample_poly launch: the signal table (int32 [rows][DS_RP_NI]) and the launch sizes.  A signal whose rate is the
    target's is left out of the launch (`same`); `ooff[i]`, `olen[i]` place EVERY signal's output in one buffer of `total_out` samples.
    The input buffer holds the launched signals back to back, or (dense=True) every signal, launched or not."""

    def __init__(self, lengths, orig_sr, target_sr, out_lengths, bank, dense=False):
        n = len(lengths)
        srs, targets = _per_signal(orig_sr, n, "resample_poly (orig_sr)"), _per_signal(target_sr, n, "resample_poly (target_sr)")
        pairs = [rate_pair(sr, tr) for sr, tr in zip(srs, targets)]
        for ln in lengths:
            if ln < 1:
                raise ValueError("resample_poly: an empty signal")
        self.nres = [resampled_length(ln, up, down) for ln, (up, down, _) in zip(lengths, pairs)]
        if out_lengths is None:
            self.olen = list(self.nres)
        else:
            self.olen = _per_signal(out_lengths, n, "resample_poly (lengths)")
            for v in self.olen:
                if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0:
                    raise ValueError(f"resample_poly: a length must be a non-negative int (got {v!r})")
            self.olen = [int(v) for v in self.olen]
        self.ooff = [0] * n
        self.same, self.rows = [], []
        rows, xoff, ooff = [], 0, 0
        self.max_blocks = self.max_taps = self.span = 0
        for i, (ln, (up, down, half)) in enumerate(zip(lengths, pairs)):
            self.ooff[i] = ooff
            if (up, down) == (1, 1):
                self.same.append(i)
            elif self.olen[i] > 0:
                blk, span = block_outputs(up, down, half)
                rows.append((xoff, ln, ooff, self.olen[i], self.nres[i], up, down, half, bank.offset(up, down), blk))
                self.rows.append(i)
                xoff += 0 if dense else ln
                self.max_blocks = max(self.max_blocks, -(-self.olen[i] // blk))
                self.max_taps, self.span = max(self.max_taps, 2 * half + 1), max(self.span, span)
            xoff += ln if dense else 0
            ooff += self.olen[i]
        self.total_in, self.total_out = xoff, ooff
        if max(self.total_in, self.total_out) >= 2 ** 31 - MAX_BLK:
            raise ValueError(f"resample_poly: {max(self.total_in, self.total_out)} samples in one batch (at most 2^31 - 1 - {MAX_BLK})")
        self.tab = np.array(rows, dtype=np.int32).reshape(len(rows), _RP["DS_RP_NI"])


def _run(sigs, orig_sr, target_sr, lengths):
    """sigs: fp32 1-D CUDA tensors -> (the buffer holding every signal's output, the plan)."""
    dev = sigs[0].device
    bank = filter_bank(dev)
    p = _Plan([s.numel() for s in sigs], orig_sr, target_sr, lengths, bank)
    x = tab = None
    if p.rows:
        ins = [sigs[i] for i in p.rows]
        x = ins[0] if len(ins) == 1 else torch.cat(ins)
        tab = torch.from_numpy(p.tab.reshape(-1)).to(dev)
    return _launch(p, x, tab.data_ptr() if p.rows else None, bank, sigs), p


def _launch(p, x, tab_ptr, bank, sigs):
    """The launch of plan p on its input buffer x and its uploaded table, then the signals that stay out of it -> the output buffer."""
    dev = sigs[0].device
    out = torch.empty(p.total_out, dtype=torch.float32, device=dev)
    if p.rows:
        L.call("ds_resample_poly", x.data_ptr(), tab_ptr, bank.device(dev).data_ptr(), len(p.rows), p.max_blocks, p.max_taps, p.span, p.total_in,
               p.total_out, bank.total, out.data_ptr(), L.current_stream())
    for i in p.same:                                   # the input's bits, cropped or zero-padded
        o, n, k = p.ooff[i], p.olen[i], min(p.olen[i], sigs[i].numel())
        out[o:o + k].copy_(sigs[i][:k])
        out[o + k:o + n].zero_()
    return out


# ---------------------------------------------------------------------------------------------------- public
@torch.no_grad()
def resample_poly(signals, orig_sr, target_sr=16000, lengths=None):
    """librosa.resample(y, orig_sr=, target_sr=, res_type="polyphase") — scipy.signal.resample_poly(y, up, down) with its defaults, NOT librosa's
    default soxr_hq (see the module's text) — for a batch, fused with librosa.util.fix_length.

    signals: a (B, L) CUDA tensor or a list of 1-D CUDA tensors of different lengths; orig_sr, target_sr: one positive int each or one
    per signal (the rows of a launch may each have their own rate pair);
    lengths: None = ceil(N up / down) samples each, otherwise the length every output is cropped or zero-padded to (one value or one per
    signal).  -> fp32: a (B, L') tensor for a tensor input whose outputs share one length, else a list of 1-D tensors (views of one buffer).
    One table upload and one launch (plus one filter upload the first time a device meets a rate pair); a signal whose orig_sr is target_sr
    does not enter the launch and comes back bit for bit, cropped or zero-padded.  A signal's output does not depend on what else is in the
    batch.  ValueError: rates that are not positive ints, a pair that needs more than DS_RP_MAX_TAPS filter taps (15999 -> 16000), an empty
    signal, an entry that is not 1-D (stereo)."""
    if isinstance(signals, torch.Tensor):
        _require_cuda(signals, "resample_poly")
        if signals.dim() != 2:
            raise ValueError("resample_poly: expected a (B, L) tensor or a list of 1-D tensors")
        sigs, was_tensor = list(signals.detach().float().contiguous()), True
    else:
        sigs, was_tensor = _as_list(signals, "resample_poly")
    if not sigs:
        return signals
    out, p = _run(sigs, orig_sr, target_sr, lengths)
    if was_tensor and len(set(p.olen)) == 1:
        return out.view(len(sigs), p.olen[0])
    return [out[o:o + n] for o, n in zip(p.ooff, p.olen)]


def adjust_audio_length(audio, desired_length, original_sample_rate, target_sample_rate):
    """tools.adjust_audio_length (tools.py:126) for one 1-D CUDA signal: resample (polyphase, see resample_poly) unless the rates are equal,
    then crop or zero-pad to desired_length.  -> fp32 CUDA tensor of desired_length samples."""
    _require_cuda(audio, "adjust_audio_length")
    if audio.dim() != 1:
        raise ValueError("adjust_audio_length: expected one 1-D (mono) signal")
    return resample_poly([audio], original_sample_rate, target_sample_rate, lengths=desired_length)[0]


def _mono(samples, i):
    """An upload's samples as a 1-D tensor on whatever device they are on; ValueError for anything that is not mono."""
    t = torch.from_numpy(np.ascontiguousarray(samples)) if isinstance(samples, np.ndarray) else torch.as_tensor(samples)
    if t.dim() != 1:
        raise ValueError(f"uploads_to_stft: upload {i} has shape {tuple(t.shape)}; mono (1-D) samples only, mix a stereo upload down first")
    if t.numel() == 0:
        raise ValueError(f"uploads_to_stft: upload {i} is empty")
    return t


@torch.no_grad()
def uploads_to_stft(uploads, duration, sample_rate=16000, time_resolution=256, VAE_scale=4, pad_mode="constant"):
    """The front of receive_upload_origin_audio for a batch.  uploads: a list of (sr, samples) as Gradio gives them — numpy int16 / float
    arrays or tensors, on either device, mono.  The reference's steps in its order: to fp32; x / max|x| (ds_peak_normalize; SILENCE YIELDS
    NaN, as numpy's 0 / 0 does — not checked, a check would cost a device -> host sync); width = int(time_resolution ((duration + 1) / 4) /
    VAE_scale); resample to sample_rate (polyphase, see resample_poly) and crop / zero-pad to 256 (VAE_scale width - 1) samples in one
    launch; audio_to_stft_representation.

    -> (enc, audio): enc (B, 3, 512, max(time_resolution, VAE_scale width)) fp32, ready for
    vocoder.InputBatch2Encode_STFT(encoder, enc, quantizer=...); audio the fitted (B, L) fp32 tensor."""
    from .vocoder import audio_to_stft_representation
    uploads = list(uploads)
    if not uploads:
        raise ValueError("uploads_to_stft: no uploads")
    srs = [_check_rate(sr, f"uploads_to_stft (upload {i})") for i, (sr, _) in enumerate(uploads)]
    raw = [_mono(samples, i) for i, (_, samples) in enumerate(uploads)]
    for sr in srs:
        rate_pair(sr, sample_rate)
    length = upload_length(duration, time_resolution, VAE_scale)
    if length < 1:
        raise ValueError(f"uploads_to_stft: duration {duration!r} leaves no samples at time_resolution {time_resolution}, VAE_scale {VAE_scale}")
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU % "uploads_to_stft")
    sigs = [t.detach().cuda().float().contiguous() for t in raw]
    dev, n, lengths = sigs[0].device, len(sigs), [s.numel() for s in sigs]
    bank = filter_bank(dev)
    p = _Plan(lengths, srs, sample_rate, length, bank, dense=True)
    pv = _flat_table(lengths)
    tables = torch.from_numpy(np.concatenate([pv.reshape(-1), p.tab.reshape(-1)])).to(dev)       # both kernels' tables in ONE upload
    x = sigs[0] if n == 1 else torch.cat(sigs)
    ws = torch.empty(max(1, L.load().ds_peak_normalize_ws_bytes(n, max(lengths)) // 4), dtype=torch.float32, device=dev)
    normed = torch.empty_like(x)
    L.call("ds_peak_normalize", x.data_ptr(), tables.data_ptr(), n, max(lengths), x.numel(), ws.data_ptr(), normed.data_ptr(), L.current_stream())
    offs = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    out = _launch(p, normed, tables.data_ptr() + 4 * pv.size, bank, [normed[o:o + k] for o, k in zip(offs, lengths)])
    audio = out.view(n, length)
    return audio_to_stft_representation(audio, time_resolution, pad_mode=pad_mode), audio
