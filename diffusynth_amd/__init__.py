"""diffusynth_amd — MI355X-native (gfx950) implementation of diffusynth's text-conditioned
denoising sampling path: DiffSynthSampler.sample() -> ConditionedUnet.forward -> VQ -> VQGAN
decoder -> ISTFT+/iSTFT, as hand-written HIP kernels behind a C-ABI library
(include/diffusynth_hip.h), with Python host code that mirrors the reference's signatures.

Importing the package is cheap and works without a GPU; anything that computes loads
``libdiffusynth_hip.so`` and raises if it is missing (there is no CPU fallback).
"""
__version__ = "0.1.0"

from .clap_text import ClapTextTower  # noqa: E402,F401
from .pitch import PitchEstimate, estimate_pitch, yin  # noqa: E402,F401
from .arranger import Formant, Mastering, MasterStats, Performance, adsr_envelope, master, tempo_map_of  # noqa: E402,F401
from .loudness import Loudness, kweighting, loudness  # noqa: E402,F401
from .true_peak import TruePeak, true_peak, true_peak_coefficients  # noqa: E402,F401
from .ingest import adjust_audio_length, resample_poly, uploads_to_stft  # noqa: E402,F401
from .inpaint_mask import latent_mask_from_layers, zoomed_size  # noqa: E402,F401
