"""Restatement of CLAP's text tower (RoBERTa encoder, first-token pooler, two-layer projection) in plain torch ops (test infrastructure),
written from the arithmetic and not from any library's code: every tensor is cast to ``dtype`` first, so the same function is the float64
yardstick and the fp32 CPU figure the device's distance is measured against.  Driven by state dicts with Hugging Face's names; pinned
against ClapTextModelWithProjection's own outputs on synthetic weights by tests/golden/clap_text.npz (tools/gen_golden_clap_text.py).

The configs and the input ids of every case live here as literals (the long rows as integer formulas), so the generator and the tests
share them and no input is stored."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STAGES = ("last_hidden_state", "pooler_output", "text_embeds", "text_features")
BUFFERS = ("text_model.embeddings.position_ids", "text_model.embeddings.token_type_ids")     # index buffers, not weights

PROD_CONFIG = {"vocab_size": 50265, "hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12, "intermediate_size": 3072,
               "max_position_embeddings": 514, "type_vocab_size": 1, "layer_norm_eps": 1e-12, "projection_dim": 512, "pad_token_id": 1}
TINY_CONFIG = dict(PROD_CONFIG, vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                   max_position_embeddings=40, projection_dim=32)
HEAD64_CONFIG = dict(PROD_CONFIG, vocab_size=300, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=512,
                     max_position_embeddings=80, projection_dim=64)
LONG_CONFIG = dict(TINY_CONFIG, max_position_embeddings=514)
# one production-width layer (the real K, O and strides of the dense layers); no golden: checked against float64 only
WIDE_CONFIG = dict(PROD_CONFIG, vocab_size=1000, num_hidden_layers=1)
CONFIGS = {"tiny": TINY_CONFIG, "head64": HEAD64_CONFIG, "long": LONG_CONFIG, "prod": PROD_CONFIG, "wide": WIDE_CONFIG}
PAD = 1


def _rows(B, S, vocab, lengths):
    """<s> = 0, </s> = 2, pad = 1, words 3 .. vocab - 1 by an integer formula; row b holds lengths[b] tokens, then pads."""
    ids = torch.full((B, S), PAD, dtype=torch.int64)
    for b, n in enumerate(lengths):
        for s in range(n):
            ids[b, s] = 0 if s == 0 else 2 if s == n - 1 and n > 1 else 3 + (37 * s + 101 * b + 11 * s * b) % (vocab - 3)
    return ids


def inputs(name):
    """(case, input_ids int64 (B, S), attention_mask int64 (B, S)) of one named input."""
    if name == "tiny.b3s7":              # right-padded to different lengths, one row unpadded
        ids = torch.tensor([[0, 5, 17, 33, 2, 1, 1], [0, 44, 9, 2, 1, 1, 1], [0, 7, 99, 23, 61, 118, 2]])
        return "tiny", ids, (ids != PAD).long()
    if name == "tiny.b1s1":
        return "tiny", torch.tensor([[0]]), torch.tensor([[1]])
    if name == "tiny.b2s12":             # row 0: a hole in the mask over a real token; row 1: a pad id under a set mask bit
        ids = torch.tensor([[0, 12, 45, 77, 3, 90, 2, 1, 1, 1, 1, 1], [0, 8, 1, 30, 64, 2, 1, 1, 1, 1, 1, 1]])
        mask = torch.tensor([[1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]])
        return "tiny", ids, mask
    if name == "head64.b2s65":           # crosses a 64-key chunk; the second row ends inside the first chunk
        ids = _rows(2, 65, 300, [65, 40])
        return "head64", ids, (ids != PAD).long()
    if name == "head64.b17s5":           # crosses a 16-row tile of the dense layers
        ids = _rows(17, 5, 300, [5 - b % 3 for b in range(17)])
        return "head64", ids, (ids != PAD).long()
    if name == "long.b1s512":
        ids = _rows(1, 512, 120, [512])
        return "long", ids, (ids != PAD).long()
    if name == "wide.b2s8":
        ids = _rows(2, 8, 1000, [8, 5])
        return "wide", ids, (ids != PAD).long()
    raise KeyError(name)


INPUTS = ("tiny.b3s7", "tiny.b1s1", "tiny.b2s12", "head64.b2s65", "head64.b17s5", "long.b1s512")     # the ones with a golden


def keys(case):
    """[(key, shape)] of ClapTextModelWithProjection's state dict for a config of CONFIGS (the two index buffers included)."""
    with open(os.path.join(GOLDEN, "clap_text_keys.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)[case]]


def weight_keys(case):
    return [(k, s) for k, s in keys(case) if k not in BUFFERS]


def golden():
    z = np.load(os.path.join(GOLDEN, "clap_text.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def position_ids(input_ids, pad=PAD):
    """RoBERTa's rule: pad + (number of non-pad tokens up to and including this one) for a non-pad token, pad for a pad token.
    A function of input_ids alone: the attention mask has no say."""
    live = (input_ids != pad).long()
    return torch.cumsum(live, dim=1) * live + pad


def embed(sd, cfg, input_ids, dtype=torch.float64, prefix=""):
    p = lambda k: sd[prefix + "text_model.embeddings." + k].to(dtype)                                    # noqa: E731
    x = p("word_embeddings.weight")[input_ids] + p("position_embeddings.weight")[position_ids(input_ids, cfg["pad_token_id"])] \
        + p("token_type_embeddings.weight")[0]
    return F.layer_norm(x, (x.shape[-1],), p("LayerNorm.weight"), p("LayerNorm.bias"), cfg["layer_norm_eps"])


def attention(q, k, v, mask=None):
    """softmax_k(q . k d^-0.5 + mask_k) v, bidirectional; q, k, v (B, heads, S, d), mask (B, S) of 0 / 1 or None.  A masked key has
    probability exactly 0."""
    s = (q @ k.transpose(2, 3)) * q.shape[-1] ** -0.5
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def l2_normalize(x, eps=1e-12):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)


@torch.no_grad()
def tower(sd, cfg, input_ids, attention_mask=None, dtype=torch.float64, prefix=""):
    """(last_hidden_state (B, S, H), pooler_output (B, H), text_embeds (B, P), text_features (B, P)): the last one is text_embeds with
    unit rows, what get_text_features returns."""
    p = lambda k: sd[prefix + k].to(dtype)                                                               # noqa: E731
    B, S = input_ids.shape
    heads, eps = cfg["num_attention_heads"], cfg["layer_norm_eps"]
    x = embed(sd, cfg, input_ids, dtype, prefix)
    H = x.shape[-1]
    split = lambda t: t.reshape(B, S, heads, H // heads).transpose(1, 2)                                 # noqa: E731
    for n in range(cfg["num_hidden_layers"]):
        lin = lambda name, t: F.linear(t, p(f"text_model.encoder.layer.{n}.{name}.weight"),               # noqa: E731
                                       p(f"text_model.encoder.layer.{n}.{name}.bias"))
        norm = lambda name, t: F.layer_norm(t, (H,), p(f"text_model.encoder.layer.{n}.{name}.weight"),    # noqa: E731
                                            p(f"text_model.encoder.layer.{n}.{name}.bias"), eps)
        ctx = attention(split(lin("attention.self.query", x)), split(lin("attention.self.key", x)), split(lin("attention.self.value", x)),
                        attention_mask)
        x = norm("attention.output.LayerNorm", lin("attention.output.dense", ctx.transpose(1, 2).reshape(B, S, H)) + x)
        x = norm("output.LayerNorm", lin("output.dense", F.gelu(lin("intermediate.dense", x))) + x)
    pooled = torch.tanh(F.linear(x[:, 0], p("text_model.pooler.dense.weight"), p("text_model.pooler.dense.bias")))
    hidden = torch.relu(F.linear(pooled, p("text_projection.linear1.weight"), p("text_projection.linear1.bias")))
    embeds = F.linear(hidden, p("text_projection.linear2.weight"), p("text_projection.linear2.bias"))
    return x, pooled, embeds, l2_normalize(embeds)
