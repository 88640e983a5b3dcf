"""The UI's pictures on the GPU: spectrogram / phase images of an STFT+ batch and the latent image.

Replaces, for whole batches and without leaving HBM, the per-clip numpy chain of the reference's batch helpers
(webUI/natural_language_guided_4/utils.py:172-181, 229-238, 249-259: tools.decode_stft -> tools.depad_STFT -> np.abs / np.angle ->
spectrogram_to_Gradio_image / phase_to_Gradio_image, utils.py:8-86) with ds_stft_images, and latent_representation_to_Gradio_image
(utils.py:89-128) with ds_latent_image.

Two things are defined here that the reference leaves to its host:
  * a third of the phase values leave [0, 255]; the reference casts them with numpy's float -> uint8 conversion, which is undefined there
    and wraps on x86.  The kernel converts to int32 and keeps the low byte, which is what the recorded reference outputs show.
  * the reference's latent image normalises IN PLACE when it is handed a CPU tensor (its caller's latent is overwritten with 0..255).
    Inputs are never written here.
"""
import numpy as np
import torch

from . import _lib as L

_NO_GPU = "diffusynth_amd UI images run on MI355X only (%s); no CPU fallback"


def _device_tensor(x, what):
    """fp32 contiguous CUDA tensor of a tensor / array on either device (CPU inputs are uploaded)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU % what)
        x = x.cuda()
    return x.detach().float().contiguous()


@torch.no_grad()
def stft_images(enc, original_amp=None):
    """enc (B, 3, F, T) [log1p|D|, cos, sin] -> (spectrogram, phase) uint8 CUDA tensors (B, F+1, T, 3): row 0 = the highest bin, the
    last row = the implied zero bin.  original_amp: a (B, >=1, F, T) batch whose channel 0 replaces the log-magnitude (read in place)."""
    enc = _device_tensor(enc, "ds_stft_images")
    assert enc.dim() == 4 and enc.shape[1] == 3, "expected (B, 3, F, T)"
    B, _, F, T = enc.shape
    amp_ptr, amp_stride = None, 0
    if original_amp is not None:
        amp = _device_tensor(original_amp, "ds_stft_images").to(enc.device)
        assert amp.dim() == 4 and amp.shape[0] == B and tuple(amp.shape[2:]) == (F, T), "original batch must be (B, C, F, T) like enc"
        amp_ptr, amp_stride = amp.data_ptr(), amp.stride(0)
    ws = torch.empty(max(1, L.load().ds_stft_images_ws_floats(B, F, T)), dtype=torch.float32, device=enc.device)
    spec = torch.empty((B, F + 1, T, 3), dtype=torch.uint8, device=enc.device)
    phase = torch.empty_like(spec)
    L.call("ds_stft_images", enc.data_ptr(), amp_ptr, amp_stride, B, F, T, ws.data_ptr(), spec.data_ptr(), phase.data_ptr(), L.current_stream())
    return spec, phase


@torch.no_grad()
def latent_images(latents):
    """(B, 4, H, W) latents -> (B, H, W, 4) uint8 CUDA tensor: per (sample, channel) min-max scaling to 0..255, RGBA, flipped vertically,
    not enlarged.  The input is left untouched."""
    lat = _device_tensor(latents, "ds_latent_image")
    assert lat.dim() == 4, "expected (B, 4, H, W)"
    B, C, H, W = lat.shape
    ws = torch.empty(max(1, L.load().ds_latent_image_ws_floats(B, C)), dtype=torch.float32, device=lat.device)
    img = torch.empty((B, H, W, 4), dtype=torch.uint8, device=lat.device)
    L.call("ds_latent_image", lat.data_ptr(), B, C, H, W, ws.data_ptr(), img.data_ptr(), L.current_stream())
    return img


def _enlarge(img, k=8):
    return np.repeat(np.repeat(img, k, axis=0), k, axis=1)       # bytes repeated on the host: exact, and 64 x fewer bytes cross PCIe


def latent_representations_to_Gradio_images(latents):
    """Batch form: (B, 4, H, W) -> list of B (8H, 8W, 4) uint8 arrays, one device -> host copy for the batch."""
    return [_enlarge(im) for im in latent_images(latents).cpu().numpy()]


def latent_representation_to_Gradio_image(latent_representation):
    """Drop-in for utils.py:89: one (4, H, W) tensor or array on either device -> (8H, 8W, 4) uint8 array.  Unlike the reference it does
    not overwrite its argument."""
    x = torch.from_numpy(latent_representation) if isinstance(latent_representation, np.ndarray) else latent_representation
    assert x.dim() == 3, "expected (4, H, W)"
    return latent_representations_to_Gradio_images(x.unsqueeze(0))[0]
