"""The CLAP text tower on the GPU: ds_text_embed, ds_text_attention, ds_text_tail and diffusynth_amd.ClapTextTower against the float64
restatement of tests/clap_text_ref.py and against the `transformers` library's own outputs (tests/golden/clap_text.npz).

No tolerance here is a constant.  Each comparison measures, in the same run, how far the fp32 CPU restatement lands from the float64 one
(conftest.rel_err: the larger of the max-norm and the rms-relative error) and allows the device four times that distance - the rule of
tests/test_hip_timbre.py and tests/test_hip_solver.py.  Against the golden (an fp32 run itself) the device gets the same allowance on top of
the golden's own distance to float64.  The invariance tests ask for equal bits."""
import pytest
import torch

import clap_text_ref as R
from conftest import rel_err
from diffusynth_amd import _lib as L
from diffusynth_amd.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu


def _check(what, dev, f32, f64, gold=None, exact=False):
    """dev within 4 x (fp32 CPU restatement vs float64) of float64; and of the golden, on top of the golden's own distance.
    ``exact``: a case whose fp32 result is the float64 one (no rounding anywhere), so the measured distance is 0 and so must the device's be."""
    cpu, err = rel_err(f32, f64), rel_err(dev.cpu(), f64)
    print(f"[clap_text] {what}: device vs float64 {err:.3e}, fp32 CPU restatement vs float64 {cpu:.3e}")
    assert tuple(dev.shape) == tuple(f64.shape), what
    assert (cpu == 0 if exact else cpu > 0) and err <= 4 * cpu, (what, err, cpu)
    if gold is not None:
        g64, eg = rel_err(gold, f64), rel_err(dev.cpu(), gold)
        print(f"[clap_text] {what}: device vs golden {eg:.3e}, golden vs float64 {g64:.3e}")
        assert eg <= g64 + 4 * cpu, (what, eg, g64, cpu)
    return err, cpu


@pytest.fixture(scope="module")
def golden():
    return R.golden()


_TOWERS = {}


def _tower(case):
    """(state dict, tower on the device) of a config of clap_text_ref.CONFIGS, built once per module run."""
    if case not in _TOWERS:
        from diffusynth_amd import ClapTextTower
        sd = synth_state_dict(R.weight_keys(case))
        t = ClapTextTower(**R.CONFIGS[case])
        t.load_state_dict(sd)
        _TOWERS[case] = (sd, t.cuda())
    return _TOWERS[case]


# ------------------------------------------------------------------------------------------------ the kernels alone
def _embed(sd, cfg, ids):
    B, S = ids.shape
    e = lambda k: sd["text_model.embeddings." + k].cuda().contiguous()                                   # noqa: E731
    word, pos, type0 = e("word_embeddings.weight"), e("position_embeddings.weight"), e("token_type_embeddings.weight")[0].contiguous()
    g, b = e("LayerNorm.weight"), e("LayerNorm.bias")
    out = torch.full((B * S, word.shape[1]), 7.0, device="cuda")
    d_ids = ids.cuda()
    L.call("ds_text_embed", d_ids.data_ptr(), B, S, cfg["pad_token_id"], word.data_ptr(), word.shape[0], pos.data_ptr(), pos.shape[0], type0.data_ptr(),
           g.data_ptr(), b.data_ptr(), word.shape[1], cfg["layer_norm_eps"], out.data_ptr(), L.current_stream())
    return out.view(B, S, -1)


@pytest.mark.parametrize("name", ["tiny.b3s7", "tiny.b1s1", "tiny.b2s12"])
def test_text_embed_kernel(name):
    case, ids, _ = R.inputs(name)
    sd, cfg = synth_state_dict(R.weight_keys(case)), R.CONFIGS[case]
    _check(f"ds_text_embed {name}", _embed(sd, cfg, ids), R.embed(sd, cfg, ids, torch.float32), R.embed(sd, cfg, ids))


def test_text_embed_marks_ids_outside_its_tables():
    """An id past the vocabulary, a negative id, and a position past the table: NaN rows, every other row as if nothing had happened."""
    case, ids, _ = R.inputs("tiny.b3s7")
    sd, cfg = synth_state_dict(R.weight_keys(case)), R.CONFIGS[case]
    want = _embed(sd, cfg, ids)
    bad = ids.clone()
    bad[0, 1], bad[2, 6] = 120, -1
    got = _embed(sd, cfg, bad)
    nan = torch.zeros(3, 7, dtype=torch.bool)
    nan[0, 1] = nan[2, 6] = True
    assert torch.equal(got.isnan().all(dim=2).cpu(), nan) and torch.equal(got.isnan().any(dim=2).cpu(), nan)
    assert torch.equal(got[~nan.cuda()], want[~nan.cuda()])                    # 120 and -1 are not pads: the rows behind them keep their positions
    short = dict(sd)                                                          # 7 tokens need positions up to 8: a table of 6 serves the first 4
    short["text_model.embeddings.position_embeddings.weight"] = sd["text_model.embeddings.position_embeddings.weight"][:6]
    got = _embed(short, cfg, ids)
    assert torch.equal(got[2].isnan().any(dim=1).cpu(), torch.tensor([False] * 4 + [True] * 3)) and torch.equal(got[2, :4], want[2, :4])


def _attention(q, k, v, mask, mask_dtype=torch.uint8):
    """q, k, v (B, heads, S, d) on the CPU -> ctx (B, heads, S, d) from the device kernel, through the stacked [B S][3H] layout."""
    B, heads, S, d = q.shape
    rows = lambda t: t.transpose(1, 2).reshape(B * S, heads * d)                                         # noqa: E731
    qkv = torch.cat([rows(q), rows(k), rows(v)], dim=1).contiguous().cuda()
    m = None if mask is None else mask.to(mask_dtype).contiguous().cuda()
    ctx = torch.full((B * S, heads * d), float("nan"), device="cuda")
    L.call("ds_text_attention", qkv.data_ptr(), L.ptr(m), 1 if mask_dtype == torch.uint8 else 4, B, S, heads, d, ctx.data_ptr(), L.current_stream())
    return ctx.view(B, S, heads, d).transpose(1, 2)


def _mask(kind, B, S):
    if kind == "none":
        return None
    m = torch.ones(B, S, dtype=torch.int64)
    if kind == "prefix":                                   # sample b keeps its first keys: a different length per sample, never zero
        for b in range(B):
            m[b, max(1, S - S // 3 - 2 * b):] = 0
    elif S > 1:                                            # hole: one key in the middle of every sample, and the last one of sample 0
        m[:, S // 2] = 0
        m[0, S - 1] = 0 if S > 2 else 1
    return m


@pytest.mark.parametrize("kind", ["prefix", "hole", "none"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 16), (2, 7, 4, 16), (2, 65, 2, 64), (1, 130, 12, 64), (1, 512, 4, 16)])
def test_text_attention_kernel(shape, kind):
    """S = 1; a ragged query tile; one key past a 64-key chunk at the production head size; three chunks and twelve heads; the longest row."""
    B, S, heads, d = shape
    q, k, v = (synth_input(f"text_attn_{n}:{shape}", (B, heads, S, d)) for n in "qkv")
    mask = _mask(kind, B, S)
    got = _attention(q, k, v, mask, torch.int32 if kind == "hole" else torch.uint8)
    _check(f"ds_text_attention {shape} {kind}", got, R.attention(q, k, v, mask), R.attention(q.double(), k.double(), v.double(), mask),
           exact=S == 1)                                   # one key: its probability is 1 and the output is v, in any precision


def test_text_attention_kernel_on_peaked_rows():
    """q and k scaled by 4: scores sixteen times as large, rows that put nearly all their weight on a few keys."""
    shape = (2, 65, 2, 64)
    q, k, v = (synth_input(f"text_attn_{n}:{shape}", shape[:1] + (2, 65, 64), scale=s) for n, s in (("q", 4.0), ("k", 4.0), ("v", 1.0)))
    mask = _mask("prefix", 2, 65)
    want = R.attention(q.double(), k.double(), v.double(), mask)
    top = torch.softmax((q.double() @ k.double().transpose(2, 3)) / 8.0, -1).amax(-1)
    assert top.median() > 0.9                              # the rows are peaked indeed
    _check("ds_text_attention peaked", _attention(q, k, v, mask), R.attention(q, k, v, mask), want)


@pytest.mark.parametrize("D", [32, 512])
def test_text_tail_kernel(D):
    B = 5
    x = synth_input(f"text_tail:{D}", (B, D), scale=2.0)
    x[3] = 0.0                                             # an all-zero row: its norm is clamped, the result is 0 and not NaN
    x[4] *= 1e-3

    def tail(op, eps=0.0, inplace=False):
        d = x.cuda()
        out = d if inplace else torch.full((B, D), float("nan"), device="cuda")
        L.call("ds_text_tail", d.data_ptr(), B, D, L.TAIL[op], eps, out.data_ptr(), L.current_stream())
        return out
    _check(f"ds_text_tail tanh D={D}", tail("DS_TAIL_TANH"), torch.tanh(x), torch.tanh(x.double()))
    assert torch.equal(tail("DS_TAIL_RELU").cpu(), torch.relu(x))
    unit = tail("DS_TAIL_L2NORM", 1e-12)
    _check(f"ds_text_tail l2 D={D}", unit, R.l2_normalize(x), R.l2_normalize(x.double()))
    assert torch.equal(unit[3].cpu(), torch.zeros(D))
    for op in ("DS_TAIL_TANH", "DS_TAIL_RELU", "DS_TAIL_L2NORM"):
        assert torch.equal(tail(op, 1e-12, inplace=True), tail(op, 1e-12)), op


# ------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("name", R.INPUTS)
def test_tower_all_stages(golden, name):
    case, ids, mask = R.inputs(name)
    sd, tower = _tower(case)
    f64, f32 = R.tower(sd, R.CONFIGS[case], ids, mask), R.tower(sd, R.CONFIGS[case], ids, mask, torch.float32)
    got = tower(ids, mask)
    assert len(got) == 3 and all(t.is_cuda and t.dtype == torch.float32 for t in got)
    got = got + (tower.get_text_features(input_ids=ids, attention_mask=mask),)
    for k, stage in enumerate(R.STAGES):
        _check(f"{name} {stage}", got[k], f32[k], f64[k], golden[f"{name}.{stage}"])
    # ids and mask on the device, int32 ids, a bool mask: the same bits
    again = tower(ids.cuda().int(), mask.cuda().bool())
    assert all(torch.equal(a, b) for a, b in zip(again, got[:3]))


def test_one_production_width_layer():
    """H 768, 12 heads of 64, intermediate 3072: the real K, O and strides of every ds_linear of the tower, the pooler's S H row stride."""
    case, ids, mask = R.inputs("wide.b2s8")
    sd, tower = _tower(case)
    f64, f32 = R.tower(sd, R.CONFIGS[case], ids, mask), R.tower(sd, R.CONFIGS[case], ids, mask, torch.float32)
    got = tower(ids, mask) + (tower.get_text_features(ids, mask),)
    for k, stage in enumerate(R.STAGES):
        _check(f"wide.b2s8 {stage}", got[k], f32[k], f64[k])


def test_a_prompt_does_not_depend_on_its_batch_or_its_padding():
    """Row 0 of the B = 3, S = 7 batch holds 5 tokens: alone at S = 5, inside the batch, and padded to S = 12 beside another prompt."""
    case, ids, mask = R.inputs("tiny.b3s7")
    _, tower = _tower(case)
    n = int(mask[0].sum())
    assert n == 5 and ids.shape[1] == 7
    alone_h, alone_p, alone_e = tower(ids[:1, :n])                             # no mask: all ones
    alone_f = tower.get_text_features(ids[:1, :n])
    batch_h, batch_p, batch_e = tower(ids, mask)
    batch_f = tower.get_text_features(ids, mask)
    wide_ids = torch.full((2, 12), R.PAD, dtype=torch.int64)
    wide_ids[0, :7], wide_ids[1, :n] = ids[2], ids[0, :n]
    wide_mask = (wide_ids != R.PAD).long()
    wide_h, wide_p, wide_e = tower(wide_ids, wide_mask)
    wide_f = tower.get_text_features(wide_ids, wide_mask)
    for what, a, b, c in (("last_hidden_state", alone_h[0], batch_h[0, :n], wide_h[1, :n]), ("pooler_output", alone_p[0], batch_p[0], wide_p[1]),
                          ("text_embeds", alone_e[0], batch_e[0], wide_e[1]), ("text_features", alone_f[0], batch_f[0], wide_f[1])):
        assert torch.equal(a, b) and torch.equal(a, c), what
    assert torch.equal(batch_f[2], wide_f[0])                                  # the unpadded row, padded
    assert torch.equal(tower.get_text_features(ids, mask), batch_f)            # two calls, the same bits


def test_text_features_have_unit_rows():
    """The device's row norms against 1 under the measured rule.  The fp32 CPU norms can land on 1.0 exactly; half an ulp of 1 (2^-24) is the
    nearest a rounded fp32 result is promised to be, so the measured distance is not taken below it."""
    for name in ("tiny.b3s7", "head64.b17s5"):
        case, ids, mask = R.inputs(name)
        sd, tower = _tower(case)
        f32 = R.tower(sd, R.CONFIGS[case], ids, mask, torch.float32)[3]
        one = torch.ones(ids.shape[0], dtype=torch.float64)
        cpu = max(rel_err(f32.norm(dim=1), one), 2.0 ** -24)
        err = rel_err(tower.get_text_features(ids, mask).double().norm(dim=1).cpu(), one)
        print(f"[clap_text] {name} row norms: device vs 1 {err:.3e}, fp32 CPU restatement vs 1 {cpu:.3e}")
        assert err <= 4 * cpu, (name, err, cpu)


def test_fp32_only_and_stale_weights():
    from diffusynth_amd import ClapTextTower
    sd = synth_state_dict(R.weight_keys("tiny"))
    tower = ClapTextTower(**R.TINY_CONFIG).cuda()
    _, ids, mask = R.inputs("tiny.b3s7")
    before = tower.get_text_features(ids, mask)
    tower.load_state_dict(sd)                                                  # the packed q | k | v follow the new weights
    assert not torch.equal(before, tower.get_text_features(ids, mask))
    assert torch.equal(tower.get_text_features(ids, mask), _tower("tiny")[1].get_text_features(ids, mask))
    with pytest.raises(NotImplementedError, match="fp32 only"):
        tower.half()


# ------------------------------------------------------------------------------------------------ the wiring
def _mmm():
    import timbre_ref as T
    from diffusynth_amd import ClapTextTower
    from diffusynth_amd.timbre import TimbreEncoder, multi_modal_model
    cfg = dict(T.MMM_CONFIG, spectrogram_feature_dim=48, text_feature_dim=32, multi_modal_emb_dim=32)
    m = multi_modal_model(TimbreEncoder(**T.SMALL_CONFIG), ClapTextTower(**R.TINY_CONFIG), **cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()])
    return m, sd


def test_multi_modal_model_runs_from_token_ids():
    """A ClapModel-shaped checkpoint (audio tower, logit scales and index buffers under text_encoder.) loads through multi_modal_model, and
    get_text_features is the projection head over the tower's feature, bit for bit."""
    import timbre_ref as T
    m, sd = _mmm()
    ckpt = dict(sd)
    ckpt["text_encoder.text_model.embeddings.position_ids"] = torch.arange(40).view(1, 40)
    ckpt["text_encoder.text_model.embeddings.token_type_ids"] = torch.zeros(1, 40, dtype=torch.int64)
    ckpt["text_encoder.audio_model.audio_encoder.norm.weight"] = torch.zeros(3)
    ckpt["text_encoder.audio_projection.linear1.weight"] = torch.zeros(3, 3)
    ckpt["text_encoder.logit_scale_a"] = torch.zeros(())
    res = m.load_state_dict(ckpt)
    assert not res.missing_keys and not res.unexpected_keys
    m.cuda()
    _, ids, mask = R.inputs("tiny.b3s7")
    got = m.get_text_features(ids, mask)
    feature = m.text_encoder.get_text_features(ids, mask)
    assert got.is_cuda and tuple(got.shape) == (3, 32) and torch.equal(got, m.project_text_features(feature))
    # and against float64: the tower's weights sit under text_encoder., the head's under text_projection.
    f64 = T.projection_head(sd, "text_projection", R.tower(sd, R.TINY_CONFIG, ids, mask, prefix="text_encoder.")[3])
    f32 = T.projection_head(sd, "text_projection", R.tower(sd, R.TINY_CONFIG, ids, mask, torch.float32, prefix="text_encoder.")[3], torch.float32)
    _check("mmm.get_text_features", got, f32, f64)


def test_diffsynth_takes_its_condition_from_the_tower():
    from diffusynth_amd.arranger import DiffSynth
    _, tower = _tower("tiny")
    calls = []

    def tokenizer(texts, padding=True, return_tensors="pt"):
        calls.append((texts, padding, return_tensors))
        return {"input_ids": torch.tensor([[0, 2]]), "attention_mask": torch.tensor([[1, 1]]), "token_type_ids": torch.tensor([[0, 0]])}
    synth = DiffSynth({}, None, None, None, tower, tokenizer, "cuda")
    cond = synth._condition()
    assert calls == [([""], True, "pt")] and cond.is_cuda and tuple(cond.shape) == (1, 32)
    assert torch.equal(cond, tower.get_text_features(torch.tensor([[0, 2]])))
