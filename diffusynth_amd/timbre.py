"""Timbre encoder and multi-modal scoring on device - drop-in for TimbreEncoder / get_timbre_encoder (model/timbre_encoder_pretrain.py:9-86,
128-152) and for the inference side of multi_modal_model / get_multi_modal_model (model/multimodal_model.py:50-121,144-168; app.py:47-59).
Same constructor arguments and state-dict names; inference only, fp32 only, HIP only.

The encoder reads the latent sample() leaves on the device: (B, 4, 128, W) viewed as (B, 512, W), an LSTM over W.  Per call:

    ds_nchw_to_nhwc            (B, C, W) -> (B, W, C)
    ds_linear                  input_layer over all B W rows
    per LSTM layer             ds_linear (W_ih, b_ih + b_hh over all B W rows), then ds_lstm_layer: one launch per time step, in stream order
    ds_linear + ds_timbre_heads   the four classifiers stacked into one matrix, their log-softmax / sigmoid in one launch

The nn.LSTM is held as the parameter container only (it gives the reference's key names); its forward is never called.  The CLAP text tower
is clap_text.ClapTextTower: given as multi_modal_model's text_encoder it makes get_text_features run end to end on the device."""
import torch
from torch import nn

from . import _lib as L
from .clap_text import ClapTextTower
from .text_head import ProjectionHead

_HEADS = ("instrument", "instrument_family", "velocity", "qualities")


def _device_input(x, what):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"diffusynth_amd {what} runs on MI355X only (ds_linear / ds_lstm_layer); no CPU fallback")
    return x.float().contiguous()


def _linear(x, w, b, rows, K, O):
    y = torch.empty(rows, O, device=x.device, dtype=torch.float32)
    L.call("ds_linear", x.data_ptr(), K, w.data_ptr(), L.ptr(b), rows, K, O, 0, y.data_ptr(), O, L.current_stream())
    return y


class TimbreEncoder(nn.Module):
    def __init__(self, input_dim, feature_dim, hidden_dim, num_instrument_classes, num_instrument_family_classes, num_velocity_classes,
                 num_qualities, num_layers=1):
        super().__init__()
        if hidden_dim % 16:
            raise NotImplementedError(f"diffusynth_amd.TimbreEncoder: hidden_dim={hidden_dim} (ds_lstm_layer takes multiples of 16)")
        self.input_layer = nn.Linear(input_dim, feature_dim)
        self.lstm = nn.LSTM(feature_dim, hidden_dim, num_layers=num_layers, batch_first=True)        # parameter container only
        self.instrument_classifier_layer = nn.Linear(hidden_dim, num_instrument_classes)
        self.instrument_family_classifier_layer = nn.Linear(hidden_dim, num_instrument_family_classes)
        self.velocity_classifier_layer = nn.Linear(hidden_dim, num_velocity_classes)
        self.qualities_classifier_layer = nn.Linear(hidden_dim, num_qualities)
        self.softmax = nn.LogSoftmax(dim=1)
        self._packed = None
        self.eval()

    # the fp32 copies the kernels read (b_ih + b_hh per layer, the four classifiers as one matrix) are made on first use
    # (_load_from_state_dict, not load_state_dict: it also runs when the encoder is loaded as a part of multi_modal_model)
    def _load_from_state_dict(self, *a, **k):
        self._packed = None
        return super()._load_from_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def _weights(self):
        if self._packed is None:
            f = lambda t: t.detach().float().contiguous()                                                # noqa: E731
            layers = [(f(getattr(self.lstm, f"weight_ih_l{k}")), f(getattr(self.lstm, f"weight_hh_l{k}")),
                       f(getattr(self.lstm, f"bias_ih_l{k}")) + f(getattr(self.lstm, f"bias_hh_l{k}"))) for k in range(self.lstm.num_layers)]
            heads = [getattr(self, n + "_classifier_layer") for n in _HEADS]
            self._packed = {"in": (f(self.input_layer.weight), f(self.input_layer.bias)), "layers": layers,
                            "heads": (torch.cat([f(h.weight) for h in heads]).contiguous(), torch.cat([f(h.bias) for h in heads]).contiguous()),
                            "sizes": [h.out_features for h in heads]}
        return self._packed

    @torch.no_grad()
    def features(self, x):
        """The last hidden state of the top LSTM layer, (B, hidden_dim): forward()'s first output without the classifier heads."""
        x = _device_input(x, "TimbreEncoder")
        if x.dim() != 4 or x.shape[1] * x.shape[2] != self.input_layer.in_features or x.shape[0] < 1 or x.shape[3] < 1:
            raise ValueError(f"TimbreEncoder: expected (B, a, b, T) with a * b == {self.input_layer.in_features}, got {tuple(x.shape)}")
        w = self._weights()
        B, T = x.shape[0], x.shape[3]
        C, F, H = self.input_layer.in_features, self.input_layer.out_features, self.lstm.hidden_size
        st = L.current_stream()
        seq = torch.empty(B * T, C, device=x.device, dtype=torch.float32)
        L.call("ds_nchw_to_nhwc", x.data_ptr(), B, C, 1, T, seq.data_ptr(), C, L.DS_F32, st)
        y, K = _linear(seq, w["in"][0], w["in"][1], B * T, C, F), F
        ws = torch.empty(max(1, L.load().ds_lstm_ws_floats(B, H)), device=x.device, dtype=torch.float32)
        feature = torch.empty(B, H, device=x.device, dtype=torch.float32)
        for k, (w_ih, w_hh, bias) in enumerate(w["layers"]):
            pre = _linear(y, w_ih, bias, B * T, K, 4 * H)
            last = k == len(w["layers"]) - 1
            hs = None if last else torch.empty(B * T, H, device=x.device, dtype=torch.float32)
            L.call("ds_lstm_layer", pre.data_ptr(), T * 4 * H, 4 * H, w_hh.data_ptr(), B, T, H, L.ptr(hs), feature.data_ptr(), ws.data_ptr(), st)
            y, K = hs, H
        return feature

    @torch.no_grad()
    def forward(self, x):
        feature = self.features(x)
        w = self._weights()
        B, H = feature.shape
        n = w["sizes"]
        z = _linear(feature, w["heads"][0], w["heads"][1], B, H, sum(n))
        L.call("ds_timbre_heads", z.data_ptr(), sum(n), B, n[0], n[1], n[2], n[3], L.current_stream())
        instrument, family, velocity, qualities = z.split(n, dim=1)
        return feature, instrument, family, velocity, qualities


def get_timbre_encoder(model_Config, load_pretrain=False, model_name=None, device="cuda"):
    timbreEncoder = TimbreEncoder(**model_Config)
    print(f"Model intialized, size: {sum(p.numel() for p in timbreEncoder.parameters() if p.requires_grad)}")
    timbreEncoder.to(device)
    if load_pretrain:
        print(f"Loading weights from models/{model_name}_timbre_encoder.pth")
        checkpoint = torch.load(f"models/{model_name}_timbre_encoder.pth", map_location=device)
        timbreEncoder.load_state_dict(checkpoint["model_state_dict"])
    timbreEncoder.eval()
    return timbreEncoder


class multi_modal_model(nn.Module):
    """Inference side of the contrastive model: sounds and texts in one multi_modal_emb_dim space - the space of the U-Net's ``condition``.
    ``text_encoder`` (the CLAP tower) may be None: callers that hold the tower's 512-d feature use project_text_features().  With a
    clap_text.ClapTextTower, get_text_features(input_ids, attention_mask) runs from token ids to the condition on the device, and a reference
    checkpoint's text_encoder.text_model.* / text_encoder.text_projection.* weights load into it."""

    def __init__(self, timbre_encoder, text_encoder, spectrogram_feature_dim, text_feature_dim, multi_modal_emb_dim, temperature, dropout,
                 num_projection_layers=1, freeze_spectrogram_encoder=True, freeze_text_encoder=True):
        super().__init__()
        self.timbre_encoder = timbre_encoder
        self.text_encoder = text_encoder
        self.multi_modal_emb_dim = multi_modal_emb_dim
        self.text_projection = ProjectionHead(embedding_dim=text_feature_dim, projection_dim=multi_modal_emb_dim, dropout=dropout,
                                              num_layers=num_projection_layers)
        self.spectrogram_projection = ProjectionHead(embedding_dim=spectrogram_feature_dim, projection_dim=multi_modal_emb_dim, dropout=dropout,
                                                     num_layers=num_projection_layers)
        self.temperature = temperature
        for param in self.timbre_encoder.parameters():
            param.requires_grad = not freeze_spectrogram_encoder
        if text_encoder is not None:
            for param in text_encoder.parameters():
                param.requires_grad = not freeze_text_encoder
        self.eval()

    def load_state_dict(self, state_dict, *a, **k):
        if self.text_encoder is None:                      # a reference checkpoint carries the CLAP tower, which lives outside this package
            state_dict = {key: v for key, v in state_dict.items() if not key.startswith("text_encoder.")}
        elif isinstance(self.text_encoder, ClapTextTower):   # the checkpoint holds a whole ClapModel: the tower takes its text half
            keep = ("text_encoder.text_model.", "text_encoder.text_projection.")
            state_dict = ClapTextTower.own_keys({key: v for key, v in state_dict.items() if not key.startswith("text_encoder.") or key.startswith(keep)},
                                                "text_encoder.")
        return super().load_state_dict(state_dict, *a, **k)

    def forward(self, spectrogram_batch, tokenized_text_batch):
        raise NotImplementedError("inference only")

    def get_text_features(self, input_ids, attention_mask):
        """text_projection(text_encoder.get_text_features(...)): with a ClapTextTower every step is a HIP launch, ids may come from the CPU."""
        if self.text_encoder is None:
            raise RuntimeError("multi_modal_model was built without a text encoder: pass the CLAP text feature to project_text_features()")
        return self.text_projection(self.text_encoder.get_text_features(input_ids=input_ids, attention_mask=attention_mask))

    def project_text_features(self, clap_features):
        return self.text_projection(clap_features)

    def get_timbre_features(self, spectrogram_batch):
        return self.spectrogram_projection(self.timbre_encoder.features(spectrogram_batch))

    @torch.no_grad()
    def prompt_scores(self, conditions, latents):
        """(n_text, n_sound) = conditions @ get_timbre_features(latents)^T / temperature (multimodal_model.py:96-100's logits);
        ``conditions``: vectors already in the condition space, (n_text, multi_modal_emb_dim)."""
        cond = _device_input(conditions, "prompt_scores")
        D = self.multi_modal_emb_dim
        if cond.dim() != 2 or cond.shape[1] != D:
            raise ValueError(f"prompt_scores: conditions must be (n_text, {D}), got {tuple(cond.shape)}")
        emb = self.get_timbre_features(latents)
        scores = _linear(cond, emb, None, cond.shape[0], D, emb.shape[0])
        return scores / self.temperature


def get_multi_modal_model(timbre_encoder, text_encoder, model_Config, load_pretrain=False, model_name=None, device="cuda"):
    mmm = multi_modal_model(timbre_encoder, text_encoder, **model_Config)
    print(f"Model intialized, size: {sum(p.numel() for p in mmm.parameters() if p.requires_grad)}")
    mmm.to(device)
    if load_pretrain:
        print(f"Loading weights from models/{model_name}_MMM.pth")
        checkpoint = torch.load(f"models/{model_name}_MMM.pth", map_location=device)
        mmm.load_state_dict(checkpoint["model_state_dict"])
    mmm.eval()
    return mmm


def rank_by_prompt(mmm, condition, latents):
    """(order, scores) on the device: the indices of ``latents`` from best to worst match of one condition vector, and their scores
    in the order of ``latents``."""
    scores = mmm.prompt_scores(condition.reshape(1, -1), latents)[0]
    return torch.argsort(scores, descending=True), scores
