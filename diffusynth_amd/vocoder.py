"""Latent -> audio tail: VQGAN decoder output -> ISTFT+ -> inverse STFT, on the GPU.

Replaces the audio branch of encodeBatch2GradioOutput_STFT
(webUI/natural_language_guided_4/utils.py:219-245: decoder -> .cpu().numpy() -> per-sample
tools.decode_stft / tools.depad_STFT -> librosa.istft(D, hop_length=256, win_length=1024)) with one
batched kernel pair (ds_istft_plus): the (B,3,512,T) decoder output never leaves HBM and the whole
batch is inverted at once.  The spectrogram / phase images of the two batch helpers are rendered from the same device tensor
(ui_images.stft_images: ds_stft_images) and cross to the host as bytes, one copy per image kind for the whole batch.

librosa is absent offline, so the inverse-STFT stage is parity-unpinned against the reference; it is
checked against the CPU oracle (librosa's documented algorithm, cross-checked with torch.istft /
scipy.signal.istft) in tests/.
"""
import numpy as np
import torch

from . import _lib as L
from .ui_images import stft_images


@torch.no_grad()
def stft_representation_to_audio(enc, hop_length=256, loop=False):
    """enc: (B, 3, F, T) fp32 CUDA tensor [log1p|D|, cos, sin] (F = n_fft/2 rows, DC row implied zero)
    -> (B, hop*(T-1)) fp32 audio.  ``loop=True``: the frames lie on a circle (frame 0 follows frame T-1; ds_istft_plus_loop)
    -> (B, hop*T), one period; T >= n_fft/hop."""
    if not enc.is_cuda:
        raise RuntimeError("diffusynth_amd vocoder runs on MI355X only (ds_istft_plus); no CPU fallback")
    enc = enc.float().contiguous()
    B, three, F, T = enc.shape
    assert three == 3, "expected (B, 3, F, T)"
    ws = torch.empty(L.load().ds_istft_ws_floats(B, F, T), dtype=torch.float32, device=enc.device)
    audio = torch.empty((B, hop_length * (T if loop else T - 1)), dtype=torch.float32, device=enc.device)
    L.call("ds_istft_plus_loop" if loop else "ds_istft_plus", enc.data_ptr(), B, F, T, hop_length, ws.data_ptr(), audio.data_ptr(),
           L.current_stream())
    return audio


def _loops(module):
    """A WindowedDecoder / WindowedEncoder with ``loop=True`` stands for one period of a loop: its audio is that period."""
    return bool(getattr(module, "loop", False))


@torch.no_grad()
def latents_to_audio(decoder, quantized_latents):
    """(B, 4, H, W) quantised latents -> (B, 256*(4W-1)) audio: decoder + ISTFT+ + iSTFT, all on device.  A decoder with ``loop=True``
    (windowed.WindowedDecoder): (B, 256*4W), one period."""
    return stft_representation_to_audio(decoder(quantized_latents), loop=_loops(decoder))


def _image_lists(enc, original_amp=None):
    """Two lists of per-clip (F+1, T, 3) uint8 arrays: one device -> host copy per image kind."""
    spec, phase = stft_images(enc, original_amp)
    return list(spec.cpu().numpy()), list(phase.cpu().numpy())


def _signals(enc, loop=False):
    return [s.astype(np.float64) for s in stft_representation_to_audio(enc, loop=loop).cpu().numpy()]


def encodeBatch2GradioOutput_STFT(decoder, latent_vector_batch, resolution=(512, 256), original_STFT_batch=None):
    """Signature and 6-tuple of utils.py:194: (spectrogram images, phase images, signals, and the same three with the log-magnitude of
    original_STFT_batch in place of the decoder's — empty lists when it is not given).  Images are (F+1, T, 3) uint8 arrays, signals
    float64 arrays like librosa returns them."""
    dev = next(decoder.parameters()).device
    if isinstance(latent_vector_batch, np.ndarray):
        latent_vector_batch = torch.from_numpy(latent_vector_batch)
    rec = decoder(latent_vector_batch.to(dev))
    signals = _signals(rec, _loops(decoder))
    specs, phases = _image_lists(rec)
    specs_amp, phases_amp, with_amp = [], [], []
    if original_STFT_batch is not None:
        orig = torch.as_tensor(original_STFT_batch).to(dev)
        mixed = rec.clone()
        mixed[:, 0] = orig[:, 0]
        with_amp = _signals(mixed, _loops(decoder))
        specs_amp, phases_amp = _image_lists(rec, orig)
    return specs, phases, signals, specs_amp, phases_amp, with_amp


@torch.no_grad()
def audio_to_stft_representation(audio, time_resolution=256, hop_length=256, pad_mode="constant"):
    """(B, L) or (L,) fp32 audio -> (B, 3, 512, T') STFT+ representation, T' = max(time_resolution, 1 + L//hop):
    librosa.stft(n_fft=1024, hop, win 1024) + tools.pad_STFT + tools.encode_stft in one kernel (ds_stft_plus).
    pad_mode "constant" (librosa >= 0.10 default) or "reflect" (older librosa)."""
    if not audio.is_cuda:
        raise RuntimeError("diffusynth_amd STFT runs on MI355X only (ds_stft_plus); no CPU fallback")
    assert pad_mode in ("constant", "reflect")
    a = audio.float().contiguous()
    if a.dim() == 1:
        a = a.unsqueeze(0)
    B, Ln = a.shape
    T = 1 + Ln // hop_length
    T_out = max(T, time_resolution or T)
    enc = torch.empty((B, 3, 512, T_out), dtype=torch.float32, device=a.device)
    L.call("ds_stft_plus", a.data_ptr(), B, Ln, hop_length, 1 if pad_mode == "reflect" else 0, T_out, enc.data_ptr(), L.current_stream())
    return enc


@torch.no_grad()
def InputBatch2Encode_STFT(encoder, STFT_batch, resolution=(512, 256), quantizer=None, squared=True):
    """5-tuple of utils.py:131-191: the spectrogram / phase images and the signals of the INPUT batch, the latents and the quantised
    latents (None without a quantizer)."""
    dev = next(encoder.parameters()).device
    x = STFT_batch.to(dev)
    z = encoder(x)
    q = quantizer(z)[0] if quantizer is not None else None
    specs, phases = _image_lists(x)
    return specs, phases, _signals(x, _loops(encoder)), z, q
