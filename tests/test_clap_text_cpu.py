"""CPU suite of the CLAP text tower: the plain-torch restatement (tests/clap_text_ref.py) against the `transformers` library's own outputs on
synthetic weights (tests/golden/clap_text.npz), RoBERTa's position rule, and the drop-in boundary of diffusynth_amd.ClapTextTower
(state-dict names, checkpoint loading, host-side errors, exported entry points).  Nothing here imports `transformers`."""
import ctypes

import pytest
import torch

import clap_text_ref as R
from conftest import rel_err
from diffusynth_amd.synth import synth_state_dict


@pytest.fixture(scope="module")
def golden():
    return R.golden()


@pytest.mark.parametrize("name", R.INPUTS)
def test_fp32_restatement_reproduces_the_library(golden, name):
    """No constant: the golden is an fp32 run with its own distance to float64, and so is the restatement; the two may differ by the sum."""
    case, ids, mask = R.inputs(name)
    sd = synth_state_dict(R.weight_keys(case))
    f64 = R.tower(sd, R.CONFIGS[case], ids, mask)
    f32 = R.tower(sd, R.CONFIGS[case], ids, mask, torch.float32)
    for stage, a, b in zip(R.STAGES, f32, f64):
        gold = golden[f"{name}.{stage}"]
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and tuple(a.shape) == gold.shape
        own, theirs, apart = rel_err(a, b), rel_err(gold, b), rel_err(a, gold)
        print(f"{name}.{stage}: fp32 restatement vs float64 {own:.2e}, golden vs float64 {theirs:.2e}, restatement vs golden {apart:.2e}")
        assert 0 < own < 1e-5 and apart <= theirs + own, (stage, apart, theirs, own)
    assert torch.allclose(f64[3].norm(dim=1), torch.ones(ids.shape[0], dtype=torch.float64), atol=1e-12)


def test_position_ids_follow_input_ids_not_the_mask():
    _, ids, mask = R.inputs("tiny.b2s12")
    assert mask[0, 2] == 0 and ids[0, 2] != R.PAD and mask[1, 2] == 1 and ids[1, 2] == R.PAD          # the two disagree on purpose
    assert R.position_ids(ids).tolist() == [[2, 3, 4, 5, 6, 7, 8, 1, 1, 1, 1, 1], [2, 3, 1, 4, 5, 6, 1, 1, 1, 1, 1, 1]]
    assert R.position_ids(torch.tensor([[1, 1, 5, 1, 6]])).tolist() == [[1, 1, 2, 1, 3]]              # left padding counts from the first word
    assert R.position_ids(torch.tensor([[7, 3]]), pad=3).tolist() == [[4, 3]]


def test_state_dict_names_and_shapes_match_the_library():
    from diffusynth_amd import ClapTextTower
    with torch.device("meta"):                             # names and shapes only: no 500 MB of initial values
        tower = ClapTextTower()
    got = [(k, tuple(v.shape)) for k, v in tower.state_dict().items()]
    assert got == R.weight_keys("prod")
    assert len(R.keys("prod")) == len(got) + 2 and sum(p.numel() for p in tower.parameters()) == 125302016
    assert not tower.training
    for case in ("tiny", "head64", "long", "wide"):
        assert [(k, tuple(v.shape)) for k, v in ClapTextTower(**R.CONFIGS[case]).state_dict().items()] == R.weight_keys(case), case
    with pytest.raises(NotImplementedError, match="head size"):
        ClapTextTower(**dict(R.TINY_CONFIG, num_attention_heads=32))


def test_checkpoints_with_foreign_keys_load_and_missing_keys_fail():
    from diffusynth_amd import ClapTextTower
    sd = synth_state_dict(R.weight_keys("tiny"))
    whole = dict(sd)
    whole.update({k: torch.zeros(s, dtype=torch.int64) for k, s in R.keys("tiny") if k in R.BUFFERS})
    whole["audio_model.audio_encoder.patch_embed.proj.weight"] = torch.zeros(3, 3)
    whole["audio_projection.linear1.bias"] = torch.zeros(3)
    whole["logit_scale_a"] = torch.zeros(())
    whole["logit_scale_t"] = torch.zeros(())
    tower = ClapTextTower(**R.TINY_CONFIG)
    tower._packed = "stale"
    res = tower.load_state_dict(whole)
    assert not res.missing_keys and not res.unexpected_keys and tower._packed is None
    for k, v in tower.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert tower.load_state_dict(sd).missing_keys == []                          # the buffers are never required
    short = {k: v for k, v in whole.items() if k != "text_model.encoder.layer.1.output.dense.bias"}
    with pytest.raises(RuntimeError, match="layer.1.output.dense.bias"):
        tower.load_state_dict(short)
    with pytest.raises(RuntimeError, match="Unexpected"):
        tower.load_state_dict(dict(sd, **{"text_model.pooler.extra": torch.zeros(1)}))


def test_multi_modal_model_keeps_the_towers_half_of_a_checkpoint():
    import timbre_ref as T
    from diffusynth_amd import ClapTextTower
    from diffusynth_amd.timbre import TimbreEncoder, multi_modal_model
    cfg = dict(T.MMM_CONFIG, spectrogram_feature_dim=48, text_feature_dim=32, multi_modal_emb_dim=32)
    m = multi_modal_model(TimbreEncoder(**T.SMALL_CONFIG), ClapTextTower(**R.TINY_CONFIG), **cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()])
    assert "text_encoder.text_model.pooler.dense.weight" in sd
    ckpt = dict(sd)
    ckpt["text_encoder.text_model.embeddings.position_ids"] = torch.zeros(1, 40, dtype=torch.int64)
    ckpt["text_encoder.audio_model.audio_encoder.norm.weight"] = torch.zeros(3)
    ckpt["text_encoder.logit_scale_t"] = torch.zeros(())
    m.text_encoder._packed = "stale"
    res = m.load_state_dict(ckpt)
    assert not res.missing_keys and not res.unexpected_keys and m.text_encoder._packed is None
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert not any(p.requires_grad for p in m.text_encoder.parameters())
    with pytest.raises(RuntimeError, match="text_encoder.text_projection.linear2.bias"):
        m.load_state_dict({k: v for k, v in ckpt.items() if k != "text_encoder.text_projection.linear2.bias"})


def test_inputs_that_are_not_taken():
    from diffusynth_amd import ClapTextTower
    tower = ClapTextTower(**R.TINY_CONFIG)                                       # 40 positions, pad 1: 38 tokens
    ok = torch.zeros(1, 38, dtype=torch.int64)
    for call in (tower, tower.get_text_features):
        with pytest.raises(ValueError, match="S=39"):
            call(torch.zeros(1, 39, dtype=torch.int64))
        with pytest.raises(ValueError, match="all zero"):
            call(torch.tensor([[0, 5, 2], [0, 2, 1]]), torch.tensor([[1, 1, 1], [0, 0, 0]]))
        with pytest.raises(ValueError, match="integers"):
            call(torch.zeros(1, 3))
        with pytest.raises(ValueError, match="vocabulary"):
            call(torch.tensor([[0, 120, 2]]))
        with pytest.raises(ValueError, match="attention_mask"):
            call(ok, torch.ones(1, 37))
        with pytest.raises(ValueError, match=r"\(B, S\)"):
            call(torch.zeros(3, dtype=torch.int64))
        # what passes the checks reaches the device question: the weights are on the CPU here
        with pytest.raises(RuntimeError, match="MI355X only.*no CPU fallback"):
            call(ok, token_type_ids=None, position_ids=None) if call is not tower else call(ok)
    for convert in (tower.half, tower.bfloat16, tower.double):
        with pytest.raises(NotImplementedError, match="fp32 only"):
            convert()
    tower.float()
    assert tower.text_projection.linear2.weight.dtype == torch.float32


def test_library_exports_the_text_tower_entry_points():
    from diffusynth_amd import _lib as L
    lib = L.load()
    for name in ("ds_text_embed", "ds_text_attention", "ds_text_tail"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert L.TAIL == {"DS_TAIL_TANH": 0, "DS_TAIL_RELU": 1, "DS_TAIL_L2NORM": 2} and lib.ds_abi_version() == 1
    # shapes they do not take are turned away before any device work (callable without a GPU)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.ds_text_attention(p, None, 1, 1, 513, 4, 16, p, None) == -1 and b"S=513" in lib.ds_last_error_string()
    assert lib.ds_text_attention(p, None, 1, 1, 0, 4, 16, p, None) == -1
    assert lib.ds_text_attention(p, None, 1, 1, 8, 4, 18, p, None) == -1 and b"d=18" in lib.ds_last_error_string()
    assert lib.ds_text_attention(p, None, 1, 1, 8, 1, 132, p, None) == -1 and b"d=132" in lib.ds_last_error_string()
    assert lib.ds_text_attention(p, p, 2, 1, 8, 4, 16, p, None) == -1 and b"mask_bytes" in lib.ds_last_error_string()
    assert lib.ds_text_embed(p, 1, 4, 9, p, 10, p, 9, p, p, p, 16, 1e-12, p, None) == -1 and b"pad_id" in lib.ds_last_error_string()
    assert lib.ds_text_tail(p, 1, 16, 3, 0.0, p, None) == -1 and b"unknown op" in lib.ds_last_error_string()
