"""GPU tests of the UI images (ds_stft_images, ds_latent_image, their wrappers and the two vocoder helpers) against the reference's
recorded outputs (golden/ui_images.npz) and the float64 restatement of tests/ui_images_ref.py.

Comparison rule (ui_images_ref.compare_images): no pixel differs by more than one level and at most 0.1 % of the pixels of a case
differ at all (phase: modulo 256); blue channels and the implied zero row are exact."""
import numpy as np
import pytest
import torch

import ui_images_ref as R
from conftest import load_golden
from diffusynth_amd import _lib as L
from diffusynth_amd.synth import synth_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vae(vqgan_sd):
    from diffusynth_amd.vqgan import PRODUCTION_CONFIG, VQGAN
    m = VQGAN(**PRODUCTION_CONFIG)
    m.load_state_dict(vqgan_sd)
    m = m.to("cuda")
    m._decoder.set_compute_dtype("fp32")
    m._encoder.set_compute_dtype("fp32")
    return m


def _c_abi_stft_images(enc, amp=None):
    """ds_stft_images through the C ABI on CUDA tensors (enc (B, 3, F, T), amp (B, C, F, T) or None) -> two (B, F+1, T, 3) arrays."""
    B, _, F, T = enc.shape
    lib = L.load()
    ws = torch.empty(max(1, lib.ds_stft_images_ws_floats(B, F, T)), device="cuda")
    spec = torch.full((B, F + 1, T, 3), 7, dtype=torch.uint8, device="cuda")
    phase = torch.full((B, F + 1, T, 3), 7, dtype=torch.uint8, device="cuda")
    L.call("ds_stft_images", enc.data_ptr(), None if amp is None else amp.data_ptr(), 0 if amp is None else amp.stride(0), B, F, T,
           ws.data_ptr(), spec.data_ptr(), phase.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    return spec.cpu().numpy(), phase.cpu().numpy()


def _golden_image(g, case, kind, i):
    red = g[f"{case}_{kind}"][i]
    return np.stack([red, red, np.full_like(red, g[kind + "_blue"])], axis=-1)


def _check_against_restatement(specs, phases, enc, amp=None, what=""):
    for i in range(enc.shape[0]):
        ws, wp = R.stft_images_ref(enc[i], None if amp is None else amp[i, 0])
        R.compare_images(specs[i], ws, what=f"{what}[{i}] spec vs restatement")
        R.compare_images(phases[i], wp, modulo=True, what=f"{what}[{i}] phase vs restatement")


@pytest.mark.parametrize("case", R.STFT_CASES)
def test_stft_images_match_reference(case):
    g = load_golden("ui_images")
    enc, amp = R.stft_case_inputs(case)
    spec, phase = _c_abi_stft_images(torch.from_numpy(enc).cuda(), None if amp is None else torch.from_numpy(amp).cuda())
    for i in range(enc.shape[0]):
        R.compare_images(spec[i], _golden_image(g, case, "spec", i), what=f"{case}[{i}] spec")
        R.compare_images(phase[i], _golden_image(g, case, "phase", i), modulo=True, what=f"{case}[{i}] phase")


@pytest.mark.parametrize("case", R.LATENT_CASES)
def test_latent_image_matches_reference(case):
    from diffusynth_amd import ui_images as U
    g = load_golden("ui_images")
    lat = torch.from_numpy(R.latent_case_input(case)).cuda()
    keep = lat.clone()
    B, (C, H, W) = 1, lat.shape
    lib = L.load()
    ws = torch.empty(lib.ds_latent_image_ws_floats(B, C), device="cuda")
    img = torch.full((B, H, W, 4), 7, dtype=torch.uint8, device="cuda")
    L.call("ds_latent_image", lat.data_ptr(), B, C, H, W, ws.data_ptr(), img.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    assert R.compare_images(img[0].cpu().numpy(), g[case], what=case + " (C ABI)") == 0            # fp32 on both sides: exact
    assert torch.equal(lat, keep)
    big = np.repeat(np.repeat(g[case], 8, axis=0), 8, axis=1)
    for x in (lat, lat.cpu(), lat.cpu().numpy()):                                                  # tensor or array, either device
        got = U.latent_representation_to_Gradio_image(x)
        assert got.shape == (8 * H, 8 * W, 4) and R.compare_images(got, big, what=case + " (drop-in)") == 0
    assert torch.equal(lat, keep)                                                                  # not normalised in place
    both = torch.stack([lat, lat.flip(0)])                                                      # second latent: channels reversed
    imgs = U.latent_representations_to_Gradio_images(both)
    assert len(imgs) == 2 and np.array_equal(imgs[0], big) and np.array_equal(imgs[1], np.ascontiguousarray(big[..., ::-1]))
    assert tuple(U.latent_images(both).shape) == (2, H, W, 4)
    with pytest.raises(L.DsError, match="latent_image"):
        U.latent_images(torch.zeros(1, 3, 8, 8, device="cuda"))


def test_stft_images_misaligned_view_and_single_column():
    """A contiguous view whose storage offset is one float (no 16-byte loads possible) gives the aligned copy's bytes; B = 1, T = 1."""
    from diffusynth_amd import ui_images as U
    enc, _ = R.stft_case_inputs("rand_b2_t64")
    want_s, want_p = U.stft_images(torch.from_numpy(enc).cuda())
    flat = torch.zeros(enc.size + 1, device="cuda")
    flat[1:] = torch.from_numpy(enc).flatten().cuda()
    view = flat[1:].view(enc.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got_s, got_p = _c_abi_stft_images(view)
    assert np.array_equal(got_s, want_s.cpu().numpy()) and np.array_equal(got_p, want_p.cpu().numpy())
    _check_against_restatement(got_s, got_p, enc, what="misaligned view")
    # the original-amplitude source as a misaligned view with its own batch stride
    amp = synth_input("ui_misaligned_amp", (2, 2, 512, 64), R.MAG_SCALE)
    aflat = torch.zeros(amp.numel() + 1, device="cuda")
    aflat[1:] = amp.flatten().cuda()
    aview = aflat[1:].view(amp.shape)
    s2, p2 = _c_abi_stft_images(torch.from_numpy(enc).cuda(), aview)
    _check_against_restatement(s2, p2, enc, amp.numpy(), what="misaligned amp")
    one = synth_input("ui_t1", (1, 3, 512, 1)).numpy()
    s1, p1 = _c_abi_stft_images(torch.from_numpy(one).cuda())
    assert s1.shape == (1, 513, 1, 3)
    _check_against_restatement(s1, p1, one, what="B=1 T=1")


def test_stft_images_of_silence():
    """All-zero log-magnitude: the clip's reference magnitude is the floor itself, so the spectrogram is all 255; phase 0 -> 127."""
    from diffusynth_amd import ui_images as U
    enc = torch.zeros(2, 3, 512, 20)
    enc[1, 1] = 1.0                                     # clip 0: (0, 0, 0), clip 1: the zero-padded column (0, 1, 0) everywhere
    spec, phase = (x.cpu().numpy() for x in U.stft_images(enc))
    assert spec.shape == phase.shape == (2, 513, 20, 3) and spec.dtype == phase.dtype == np.uint8
    assert (spec[..., :2] == 255).all() and (spec[..., 2] == R.SPEC_BLUE).all()
    assert (phase[..., :2] == 127).all() and (phase[..., 2] == R.PHASE_BLUE).all()


def test_encodeBatch2GradioOutput_STFT_fills_all_six_slots(vae):
    from diffusynth_amd.vocoder import encodeBatch2GradioOutput_STFT, latents_to_audio
    B, W = 2, 3
    q = synth_input("ui_e2e_q", (B, 4, 128, W))
    rec = vae._decoder(q.cuda()).cpu().numpy()                         # the same decoder output, pulled to the host
    audio = latents_to_audio(vae._decoder, q.cuda()).cpu().numpy()
    out = encodeBatch2GradioOutput_STFT(vae._decoder, q.numpy())
    assert len(out) == 6 and all(isinstance(s, list) for s in out)
    assert [len(s) for s in out] == [B, B, B, 0, 0, 0]
    for img in out[0] + out[1]:
        assert isinstance(img, np.ndarray) and img.shape == (513, 4 * W, 3) and img.dtype == np.uint8
    _check_against_restatement(out[0], out[1], rec, what="decoder output")
    assert out[2][0].dtype == np.float64 and np.array_equal(np.stack(out[2]), audio.astype(np.float64))
    orig = synth_input("ui_e2e_orig", (B, 3, 512, 4 * W))
    orig[:, 0] = orig[:, 0].abs()
    out2 = encodeBatch2GradioOutput_STFT(vae._decoder, q.cuda(), original_STFT_batch=orig)
    assert [len(s) for s in out2] == [B] * 6
    for img in out2[3] + out2[4]:
        assert img.shape == (513, 4 * W, 3) and img.dtype == np.uint8
    for a, b in zip(out2[0] + out2[1], out[0] + out[1]):
        assert np.array_equal(a, b)
    _check_against_restatement(out2[3], out2[4], rec, orig.numpy(), what="decoder output, original amplitude")
    assert np.array_equal(np.stack(out2[2]), np.stack(out[2])) and out2[5][0].dtype == np.float64 and out2[5][0].shape == out2[2][0].shape


def test_InputBatch2Encode_STFT_fills_images_and_signals(vae):
    from diffusynth_amd.vocoder import InputBatch2Encode_STFT, audio_to_stft_representation, stft_representation_to_audio
    y = synth_input("ui_front_audio", (2, 256 * 40))
    enc = audio_to_stft_representation(y.cuda(), time_resolution=48)                   # 41 frames of signal, 7 zero-padded columns
    assert enc.shape == (2, 3, 512, 48)
    out = InputBatch2Encode_STFT(vae._encoder, enc, quantizer=vae._vq_vae)
    assert len(out) == 5 and len(out[0]) == len(out[1]) == len(out[2]) == 2
    for img in out[0] + out[1]:
        assert img.shape == (513, 48, 3) and img.dtype == np.uint8
    _check_against_restatement(out[0], out[1], enc.cpu().numpy(), what="input batch")
    for i in range(2):
        assert (out[1][i][:, 41:, 0] == 127).all() and (out[0][i][:, 41:, 0] == 0).all()     # padded columns: phi = 0, magnitude floor
    want = stft_representation_to_audio(enc).cpu().numpy()
    for i in range(2):
        assert out[2][i].dtype == np.float64 and np.array_equal(out[2][i], want[i].astype(np.float64))
    assert out[3].shape == (2, 4, 128, 12) and out[4].shape == (2, 4, 128, 12)
    assert torch.isfinite(out[3]).all() and torch.isfinite(out[4]).all()
    assert InputBatch2Encode_STFT(vae._encoder, enc)[4] is None
