"""CPU suite of the timbre encoder: the plain-torch restatement (tests/timbre_ref.py) against the reference's own outputs
(tests/golden/timbre.npz), the drop-in boundary (state-dict names, checkpoint loading, errors) and the synthetic-weight rule for
nn.LSTM's biases."""
import numpy as np
import pytest
import torch

import timbre_ref as R
from conftest import rel_err
from diffusynth_amd.synth import synth_state_dict, synth_tensor

# The golden is the reference's fp32 run (nn.LSTM), the restatement runs in float64: what separates them is fp32 rounding through up to
# 3 x 64 recurrent steps.  The issue's own measurement of that distance is <= 9.1e-7 (features) and 1.1e-6 (logits); 1e-5 leaves a decade and
# is still three decades below what a wrong gate order, a swapped bias or a transposed weight gives (> 1e-2).
GOLDEN_TOL = 1e-5


@pytest.fixture(scope="module")
def golden():
    return R.golden()


@pytest.mark.parametrize("case,tag", [("prod", f"w{W}") for W in R.PROD_W] + [("small", f"t{T}") for T in R.SMALL_T])
def test_restatement_matches_the_reference_encoder(golden, case, tag):
    sd = synth_state_dict(R.keys(case))
    x = R.prod_input(int(tag[1:])) if case == "prod" else R.small_input(int(tag[1:]))
    got = R.timbre_encoder(sd, x)
    for name, y in zip(R.OUTPUTS, got):
        want = golden[f"{case}.{tag}.{name}"]
        assert tuple(y.shape) == want.shape
        err = rel_err(y, want)
        print(f"{case}.{tag}.{name}: float64 restatement vs reference fp32 {err:.2e}")
        assert err < GOLDEN_TOL, (name, err)
    for y in got[1:4]:
        assert torch.allclose(y.exp().sum(1), torch.ones(y.shape[0], dtype=y.dtype), atol=1e-12)


def test_restatement_matches_the_reference_multi_modal_model(golden):
    sd = synth_state_dict(R.keys("mmm"))
    got = R.mmm(sd, R.prod_input(R.MMM_W), R.text_input(), R.MMM_CONFIG["temperature"])
    for name, y in zip(("timbre_emb", "text_emb", "logits"), got):
        err = rel_err(y, golden["mmm." + name])
        print(f"mmm.{name}: float64 restatement vs reference fp32 {err:.2e}")
        assert err < GOLDEN_TOL, (name, err)
    # the ranking test on the device relies on well separated scores
    logits = np.sort(golden["mmm.logits"], axis=1)
    assert np.diff(logits, axis=1).min() >= 0.1, logits


def test_fp32_restatement_is_close_to_float64():
    """The figure every device tolerance is a multiple of: it must exist (> 0) and be of fp32 rounding size."""
    sd = synth_state_dict(R.keys("small"))
    x = R.small_input(9)
    for a, b in zip(R.timbre_encoder(sd, x, torch.float32), R.timbre_encoder(sd, x)):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert 0 < rel_err(a, b) < 1e-5


def test_state_dict_names_and_shapes_match_reference():
    from diffusynth_amd.timbre import TimbreEncoder, multi_modal_model
    for case, cfg in (("prod", R.PROD_CONFIG), ("small", R.SMALL_CONFIG)):
        got = [(k, tuple(v.shape)) for k, v in TimbreEncoder(**cfg).state_dict().items()]
        assert got == R.keys(case), case
    enc = TimbreEncoder(**R.PROD_CONFIG)
    assert sum(p.numel() for p in enc.parameters()) == 24539779
    m = multi_modal_model(enc, None, **R.MMM_CONFIG)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == R.keys("mmm")
    assert not any(p.requires_grad for p in m.timbre_encoder.parameters()) and not m.training
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        TimbreEncoder(32, 16, 40, 7, 5, 6, 4)


def test_checkpoint_with_a_text_tower_loads_without_one():
    from diffusynth_amd.timbre import TimbreEncoder, multi_modal_model
    cfg = dict(R.MMM_CONFIG, spectrogram_feature_dim=48, text_feature_dim=24, multi_modal_emb_dim=32)
    m = multi_modal_model(TimbreEncoder(**R.SMALL_CONFIG), None, **cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()])
    ckpt = dict(sd)
    ckpt["text_encoder.text_model.embeddings.word_embeddings.weight"] = torch.zeros(5, 3)
    ckpt["text_encoder.text_projection.linear1.bias"] = torch.zeros(3)
    m.timbre_encoder._packed = "stale"
    res = m.load_state_dict(ckpt)
    assert not res.missing_keys and not res.unexpected_keys
    assert m.timbre_encoder._packed is None                # loading through the model drops the encoder's packed weights too
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # with a tower of its own, the same keys are the tower's to take
    class Tower(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(3))
    m2 = multi_modal_model(TimbreEncoder(**R.SMALL_CONFIG), Tower(), **cfg)
    with pytest.raises(RuntimeError, match="text_encoder"):
        m2.load_state_dict(ckpt)
    # loading or converting the encoder by itself drops them as well
    enc = TimbreEncoder(**R.SMALL_CONFIG)
    enc._packed = "stale"
    enc.load_state_dict(synth_state_dict(R.keys("small")))
    assert enc._packed is None
    enc._packed = "stale"
    enc.double()
    assert enc._packed is None


def test_lstm_biases_follow_the_bias_rule():
    n = np.random.Generator(np.random.PCG64(__import__("zlib").crc32(b"lstm.bias_ih_l0"))).standard_normal((8,))
    assert torch.equal(synth_tensor("lstm.bias_ih_l0", (8,)), torch.from_numpy((0.1 * n).astype(np.float32)))
    assert synth_tensor("timbre_encoder.lstm.bias_hh_l2", (4096,)).abs().max() < 0.6
    # unchanged: a plain bias, and a 1-D norm gain
    n = np.random.Generator(np.random.PCG64(__import__("zlib").crc32(b"x.bias"))).standard_normal((8,))
    assert torch.equal(synth_tensor("x.bias", (8,)), torch.from_numpy((0.1 * n).astype(np.float32)))
    n = np.random.Generator(np.random.PCG64(__import__("zlib").crc32(b"x.norm.weight"))).standard_normal((8,))
    assert torch.equal(synth_tensor("x.norm.weight", (8,)), torch.from_numpy((1.0 + 0.2 * n).astype(np.float32)))


def test_training_loss_and_cpu_inputs_raise():
    from diffusynth_amd.timbre import TimbreEncoder, multi_modal_model, rank_by_prompt
    enc = TimbreEncoder(**R.SMALL_CONFIG)
    m = multi_modal_model(enc, None, **dict(R.MMM_CONFIG, spectrogram_feature_dim=48, text_feature_dim=24, multi_modal_emb_dim=32))
    with pytest.raises(NotImplementedError, match="inference only"):
        m(torch.zeros(2, 4, 8, 5), {"input_ids": None})
    x = torch.zeros(2, 4, 8, 5)
    for call in (lambda: enc(x), lambda: enc.features(x), lambda: m.get_timbre_features(x), lambda: m.prompt_scores(torch.zeros(1, 32), x),
                 lambda: rank_by_prompt(m, torch.zeros(32), x), lambda: m.project_text_features(torch.zeros(1, 24))):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    with pytest.raises(RuntimeError, match="without a text encoder"):
        m.get_text_features(torch.zeros(1, 3), None)


def test_library_exports_the_timbre_entry_points():
    import ctypes
    from diffusynth_amd import _lib as L
    lib = L.load()
    for name in ("ds_lstm_ws_floats", "ds_lstm_layer", "ds_timbre_heads"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.ds_lstm_ws_floats(17, 48) == 3 * 17 * 48
    # shapes it does not take are turned away before any device work (callable without a GPU)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.ds_lstm_layer(p, 160, 160, p, 1, 1, 40, None, p, p, None) == -1 and b"H=40" in lib.ds_last_error_string()
    assert lib.ds_lstm_layer(p, 64, 192, p, 1, 1, 48, None, p, p, None) == -1 and b"strides" in lib.ds_last_error_string()
    assert lib.ds_lstm_layer(p, 192, 192, p, 1, 0, 48, None, p, p, None) == -1
    assert lib.ds_timbre_heads(p, 10, 1, 4, 4, 4, 4, None) == -1 and b"columns" in lib.ds_last_error_string()
