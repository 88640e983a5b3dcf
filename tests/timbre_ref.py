"""Restatement of the timbre encoder and of the multi-modal model's inference paths in plain torch (test infrastructure): the LSTM is an
explicit gate loop (never nn.LSTM), every tensor is cast to ``dtype`` first, so the same code is the float64 yardstick and the fp32 CPU
figure the device's distance is measured against.  Driven by reference-format state dicts (model/timbre_encoder_pretrain.py:50-86,
model/multimodal_model.py:14-47,96-100,114-121); pinned against the reference's own outputs by tests/golden/timbre.npz."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADS = ("instrument", "instrument_family", "velocity", "qualities")
OUTPUTS = ("feature",) + HEADS

PROD_CONFIG = {"input_dim": 512, "feature_dim": 512, "hidden_dim": 1024, "num_instrument_classes": 1006,
               "num_instrument_family_classes": 11, "num_velocity_classes": 128, "num_qualities": 10, "num_layers": 3}
SMALL_CONFIG = {"input_dim": 32, "feature_dim": 16, "hidden_dim": 48, "num_instrument_classes": 7,
                "num_instrument_family_classes": 5, "num_velocity_classes": 6, "num_qualities": 4, "num_layers": 2}
MMM_CONFIG = {"spectrogram_feature_dim": 1024, "text_feature_dim": 512, "multi_modal_emb_dim": 512, "temperature": 0.5,
              "dropout": 0.1, "num_projection_layers": 2}
PROD_W, SMALL_T, MMM_W = (20, 64), (1, 2, 9), 64


def keys(name):
    """[(key, shape)] of one of the reference modules: "prod", "small" (TimbreEncoder) or "mmm" (multi_modal_model, no text tower)."""
    with open(os.path.join(GOLDEN, "timbre_keys.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)[name]]


def golden():
    z = np.load(os.path.join(GOLDEN, "timbre.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def prod_input(W):
    from diffusynth_amd.synth import synth_input
    return synth_input(f"timbre:{W}", (3, 4, 128, W))


def small_input(T):
    from diffusynth_amd.synth import synth_input
    return synth_input(f"timbre_small:{T}", (17, 4, 8, T))


def text_input():
    from diffusynth_amd.synth import synth_input
    return synth_input("timbre_text", (2, 512))


def lstm_layer(pre, w_hh):
    """One layer over a sequence: pre (B, T, 4H) = x W_ih^T + b_ih + b_hh, w_hh (4H, H), gate order i, f, g, o, h0 = c0 = 0.
    Returns (hs (B, T, H), h_last (B, H)) in pre's dtype."""
    B, T, H4 = pre.shape
    H = H4 // 4
    w_hh = w_hh.to(pre.dtype)
    h = c = torch.zeros(B, H, dtype=pre.dtype)
    hs = []
    for t in range(T):
        z = pre[:, t] + h @ w_hh.T if t else pre[:, t]
        i, f, g, o = z.split(H, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    return torch.stack(hs, 1), h


@torch.no_grad()
def timbre_encoder(sd, x, dtype=torch.float64, prefix=""):
    """TimbreEncoder.forward: the 5-tuple (feature, three log-probabilities, qualities)."""
    p = lambda k: sd[prefix + k].to(dtype)                                                                # noqa: E731
    B, T = x.shape[0], x.shape[-1]
    y = F.linear(x.to(dtype).reshape(B, -1, T).permute(0, 2, 1), p("input_layer.weight"), p("input_layer.bias"))
    layer = 0
    while f"{prefix}lstm.weight_ih_l{layer}" in sd:
        pre = F.linear(y, p(f"lstm.weight_ih_l{layer}"), p(f"lstm.bias_ih_l{layer}") + p(f"lstm.bias_hh_l{layer}"))
        y, feature = lstm_layer(pre, p(f"lstm.weight_hh_l{layer}"))
        layer += 1
    out = [feature]
    for name in HEADS:
        z = F.linear(feature, p(name + "_classifier_layer.weight"), p(name + "_classifier_layer.bias"))
        out.append(torch.sigmoid(z) if name == "qualities" else torch.log_softmax(z, dim=1))
    return tuple(out)


def projection_head(sd, prefix, x, dtype=torch.float64):
    """ProjectionHead (eval mode: dropout is the identity)."""
    x = x.to(dtype)
    i = 0
    while f"{prefix}.layers.{i}.projection.weight" in sd:
        p = lambda k: sd[f"{prefix}.layers.{i}.{k}"].to(dtype)                                            # noqa: E731
        projected = F.linear(x, p("projection.weight"), p("projection.bias"))
        h = F.linear(F.gelu(projected), p("fc.weight"), p("fc.bias")) + projected
        x = F.layer_norm(h, (h.shape[-1],), p("layer_norm.weight"), p("layer_norm.bias"), 1e-5)
        i += 1
    return x


@torch.no_grad()
def mmm(sd, latents, text_features, temperature, dtype=torch.float64):
    """(timbre_emb, text_emb, logits) of multi_modal_model: get_timbre_features, text_projection, and forward's logits."""
    timbre_emb = projection_head(sd, "spectrogram_projection", timbre_encoder(sd, latents, dtype, "timbre_encoder.")[0], dtype)
    text_emb = projection_head(sd, "text_projection", text_features, dtype)
    return timbre_emb, text_emb, (text_emb @ timbre_emb.T) / temperature
