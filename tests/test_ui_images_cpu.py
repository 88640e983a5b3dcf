"""CPU suite for the UI images: the float64 restatement of the semantics against the reference's recorded outputs, the C-ABI entries
and their argument validation without a device, and the package's no-fallback error."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ui_images_ref as R
from conftest import ROOT, load_golden
from diffusynth_amd import _lib as L

ENTRIES = ("ds_stft_images_ws_floats", "ds_stft_images", "ds_latent_image_ws_floats", "ds_latent_image")


@pytest.mark.parametrize("case", R.STFT_CASES)
def test_restatement_matches_reference_stft_images(case):
    """The semantics as restated (float64) give the images the reference's own functions produced: cap rule of the image tests
    (at most one level, at most 0.1 % of the pixels; blue and the implied zero row exact).  Expected: no differing pixel."""
    g = load_golden("ui_images")
    enc, amp = R.stft_case_inputs(case)
    assert g[case + "_spec"].shape == (enc.shape[0], enc.shape[2] + 1, enc.shape[3])
    for i in range(enc.shape[0]):
        spec, phase = R.stft_images_ref(enc[i], None if amp is None else amp[i, 0])
        for kind, img, blue in (("spec", spec, g["spec_blue"]), ("phase", phase, g["phase_blue"])):
            want = np.stack([g[f"{case}_{kind}"][i]] * 2 + [np.full_like(g[f"{case}_{kind}"][i], blue)], axis=-1)
            R.compare_images(img, want, modulo=kind == "phase", what=f"{case}[{i}] {kind}")
    assert int(g["spec_blue"]) == R.SPEC_BLUE and int(g["phase_blue"]) == R.PHASE_BLUE


def test_fixture_shows_the_properties_the_cases_were_chosen_for():
    g = load_golden("ui_images")
    assert (g["padded_phase"][0][:, 9:] == R.PHASE_ZERO_ROW).all() and (g["padded_spec"][0][:, 9:] == 0).all()    # zero-padded columns: phi = 0, floor
    for case in R.STFT_CASES:
        assert (g[case + "_phase"][:, -1] == R.PHASE_ZERO_ROW).all() and (g[case + "_spec"][:, -1] == 0).all()   # the implied zero row
        assert g[case + "_spec"].max() == 255
    enc, _ = R.stft_case_inputs("rand_b2_t64")
    assert (enc[:, 0] < 0).mean() > 0.4                                                                         # negative magnitudes: pi turns


@pytest.mark.parametrize("case", R.LATENT_CASES)
def test_restatement_matches_reference_latent_image(case):
    g = load_golden("ui_images")
    lat = R.latent_case_input(case)
    keep = lat.copy()
    got = R.latent_image_ref(lat, enlarge=1)
    assert np.array_equal(lat, keep)
    assert R.compare_images(got, g[case], what=case) == 0                                                       # fp32 on both sides: exact
    assert R.latent_image_ref(lat).shape == (8 * lat.shape[1], 8 * lat.shape[2], 4)
    if case.endswith("const"):
        assert (got[..., 2] == 0).all()


def test_header_and_binding_declare_the_entries():
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", text))
    lib = L.load()
    for name in ENTRIES:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.ds_stft_images_ws_floats(64, 512, 256) == 64 * 32 * 2 and lib.ds_latent_image_ws_floats(3, 4) == 24


def test_entries_validate_before_any_gpu_work():
    """Callable on a machine without a device: bad arguments answer DS_EINVAL (-1) and the message names the entry."""
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for B, F, T in ((0, 512, 16), (2, 0, 16), (2, 512, 0)):
        assert lib.ds_stft_images(p, None, 0, B, F, T, p, p, p, None) == -1
        assert b"stft_images" in lib.ds_last_error_string()
    assert lib.ds_stft_images(None, None, 0, 1, 512, 16, p, p, p, None) == -1 and b"stft_images" in lib.ds_last_error_string()
    for B, C in ((0, 4), (1, 3), (1, 5)):
        assert lib.ds_latent_image(p, B, C, 8, 8, p, p, None) == -1
        assert b"latent_image" in lib.ds_last_error_string()
    with pytest.raises(L.DsError, match="latent_image"):
        L.call("ds_latent_image", p, 1, 3, 8, 8, p, p, None)


def test_images_fail_loudly_without_gpu(monkeypatch):
    from diffusynth_amd import ui_images as U
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.stft_images(torch.zeros(1, 3, 8, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.latent_representation_to_Gradio_image(np.zeros((4, 8, 8), dtype=np.float32))
