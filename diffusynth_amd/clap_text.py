"""CLAP's text tower on device - drop-in for the `CLAP` object of the reference's UI callbacks, which all start with
``CLAP.get_text_features(**CLAP_tokenizer([prompt], padding=True, return_tensors="pt"))`` (text2sound.py:89-91, inpaint_with_text.py:200-202,
track_maker.py): a 12-layer RoBERTa-base encoder, its first-token pooler and CLAP's two-layer projection, from token ids to the unit-norm
(B, 512) text feature that ProjectionHead turns into the U-Net's ``condition``.  Hugging Face's ClapTextModelWithProjection state-dict names;
inference only, fp32 only, HIP only.  The tokenizer stays outside: ids and mask are inputs.

Per call (8 launches per layer, 7 around them: 103 at 12 layers):

    ds_text_embed              LayerNorm(word + position + type 0) per token, position ids by RoBERTa's rule from input_ids
    per layer                  ds_linear (q | k | v stacked, O = 3H) -> ds_text_attention -> ds_linear (attention.output.dense)
                               -> ds_add_layernorm (+ x) -> ds_linear (intermediate.dense) -> ds_activation (GELU, once)
                               -> ds_linear (output.dense) -> ds_add_layernorm (+ x)
    pooler                     ds_linear over the first-token rows (x_stride = S H), ds_text_tail (tanh)
    projection                 ds_linear, ds_text_tail (ReLU), ds_linear; get_text_features: ds_text_tail (L2 normalise)

Every one of these computes a row from that row's own inputs in an order that does not depend on the batch or on S, and masked keys add
exact zeros (csrc/clap_text.hip), so a prompt alone and the same prompt padded inside a batch give the same bits."""
import torch
from torch import nn

from . import _lib as L

_DROPPED = ("audio_model.", "audio_projection.", "logit_scale_")                                     # the rest of a whole ClapModel
_BUFFERS = ("text_model.embeddings.position_ids", "text_model.embeddings.token_type_ids")            # index buffers, not weights


def _holder(**children):
    m = nn.Module()
    for name, child in children.items():
        m.add_module(name, child)
    return m


def _linear(x, wb, rows, K, O, x_stride=None):
    y = torch.empty(rows, O, device=x.device, dtype=torch.float32)
    L.call("ds_linear", x.data_ptr(), K if x_stride is None else x_stride, wb[0].data_ptr(), wb[1].data_ptr(), rows, K, O, 0, y.data_ptr(), O,
           L.current_stream())
    return y


class ClapTextTower(nn.Module):
    def __init__(self, vocab_size=50265, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-12, projection_dim=512, pad_token_id=1):
        super().__init__()
        H, I = hidden_size, intermediate_size
        d = H // num_attention_heads
        if H % num_attention_heads or d % 4 or d > 128:
            raise NotImplementedError(f"diffusynth_amd.ClapTextTower: head size {H}/{num_attention_heads} (ds_text_attention takes multiples "
                                      "of 4 up to 128)")
        if not 0 <= pad_token_id < max_position_embeddings - 1:
            raise ValueError(f"ClapTextTower: pad_token_id={pad_token_id} leaves no position among {max_position_embeddings}")
        self.heads, self.eps, self.pad_token_id = num_attention_heads, layer_norm_eps, pad_token_id
        self.max_tokens = max_position_embeddings - pad_token_id - 1
        # parameter containers only (they give Hugging Face's key names, in its order); their forward is never called
        norm = lambda: nn.LayerNorm(H, eps=layer_norm_eps)                                           # noqa: E731
        layer = lambda: _holder(                                                                     # noqa: E731
            attention=_holder(self=_holder(query=nn.Linear(H, H), key=nn.Linear(H, H), value=nn.Linear(H, H)),
                              output=_holder(dense=nn.Linear(H, H), LayerNorm=norm())),
            intermediate=_holder(dense=nn.Linear(H, I)), output=_holder(dense=nn.Linear(I, H), LayerNorm=norm()))
        self.text_model = _holder(
            embeddings=_holder(word_embeddings=nn.Embedding(vocab_size, H, padding_idx=pad_token_id),
                               token_type_embeddings=nn.Embedding(type_vocab_size, H), LayerNorm=norm(),
                               position_embeddings=nn.Embedding(max_position_embeddings, H, padding_idx=pad_token_id)),
            encoder=_holder(layer=nn.ModuleList([layer() for _ in range(num_hidden_layers)])),
            pooler=_holder(dense=nn.Linear(H, H)))
        self.text_projection = _holder(linear1=nn.Linear(H, projection_dim), linear2=nn.Linear(projection_dim, projection_dim))
        self._packed = None
        self.eval()

    # ------------------------------------------------------------------------------------------------ weights
    @staticmethod
    def own_keys(state_dict, prefix=""):
        """The entries of a ClapTextModelWithProjection or whole ClapModel state dict (under ``prefix``) that are this tower's weights:
        without audio_model.*, audio_projection.*, logit_scale_* and the two index buffers.  Anything else unknown stays, and fails the load."""
        return {k: v for k, v in state_dict.items()
                if not k.startswith(prefix) or not (k[len(prefix):].startswith(_DROPPED) or k[len(prefix):] in _BUFFERS)}

    def load_state_dict(self, state_dict, *a, **k):
        return super().load_state_dict(self.own_keys(state_dict), *a, **k)

    # the fp32 copies the kernels read (q | k | v as one matrix per layer) are made on first use and dropped by a load or a move
    # (_load_from_state_dict, not load_state_dict: it also runs when the tower is loaded as a part of multi_modal_model)
    def _load_from_state_dict(self, *a, **k):
        self._packed = None
        return super()._load_from_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._packed = None
        r = super()._apply(fn, *a, **k)
        self._fp32_only()
        return r

    def _fp32_only(self):
        dt = self.text_projection.linear2.weight.dtype
        if dt != torch.float32:
            raise NotImplementedError(f"diffusynth_amd.ClapTextTower is fp32 only (its parameters are now {dt}); convert it back with .float()")

    def _weights(self):
        if self._packed is None:
            self._fp32_only()
            f = lambda t: t.detach().float().contiguous()                                            # noqa: E731
            wb = lambda m: (f(m.weight), f(m.bias))                                                  # noqa: E731
            e = self.text_model.embeddings
            layers = []
            for l in self.text_model.encoder.layer:
                s = l.attention.self
                layers.append({"qkv": (torch.cat([f(s.query.weight), f(s.key.weight), f(s.value.weight)]).contiguous(),
                                       torch.cat([f(s.query.bias), f(s.key.bias), f(s.value.bias)]).contiguous()),
                               "attn_out": wb(l.attention.output.dense), "attn_norm": wb(l.attention.output.LayerNorm),
                               "inter": wb(l.intermediate.dense), "out": wb(l.output.dense), "out_norm": wb(l.output.LayerNorm)})
            self._packed = {"word": f(e.word_embeddings.weight), "pos": f(e.position_embeddings.weight),
                            "type0": f(e.token_type_embeddings.weight[0]), "emb_norm": wb(e.LayerNorm), "layers": layers,
                            "pooler": wb(self.text_model.pooler.dense), "linear1": wb(self.text_projection.linear1),
                            "linear2": wb(self.text_projection.linear2)}
        return self._packed

    # ------------------------------------------------------------------------------------------------ inputs
    def _inputs(self, input_ids, attention_mask):
        """Host-side checks (ValueError), then (ids int64, mask uint8 or None) on the weights' device.  CPU tensors - what a tokenizer returns -
        are checked on the host without touching the device; device tensors cost one reduction and one sync."""
        if not torch.is_tensor(input_ids) or input_ids.dim() != 2 or input_ids.shape[0] < 1 or input_ids.shape[1] < 1:
            raise ValueError("ClapTextTower: input_ids must be a (B, S) tensor of token ids")
        if input_ids.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f"ClapTextTower: input_ids must hold integers, got {input_ids.dtype}")
        B, S = input_ids.shape
        if S > self.max_tokens:
            raise ValueError(f"ClapTextTower: S={S} tokens, but the position table holds {self.max_tokens} "
                             "(max_position_embeddings - pad_token_id - 1)")
        V = self.text_model.embeddings.word_embeddings.num_embeddings
        bad = ((input_ids < 0) | (input_ids >= V)).any()
        live = None
        if attention_mask is not None:
            if not torch.is_tensor(attention_mask) or tuple(attention_mask.shape) != (B, S):
                raise ValueError(f"ClapTextTower: attention_mask must be ({B}, {S}) like input_ids")
            live = attention_mask != 0
            empty = ~live.any(dim=1).all()
            if live.device != bad.device:
                empty = empty.to(bad.device)
            bad = torch.stack([bad, empty])
        bad = bad.reshape(-1).tolist()
        if bad[0]:
            raise ValueError(f"ClapTextTower: input_ids outside the vocabulary [0, {V})")
        if len(bad) > 1 and bad[1]:
            raise ValueError("ClapTextTower: a row of attention_mask is all zero (softmax over no key)")
        dev = self.text_projection.linear2.weight.device
        if dev.type != "cuda":
            raise RuntimeError("diffusynth_amd ClapTextTower runs on MI355X only (ds_text_embed / ds_text_attention / ds_linear); no CPU fallback")
        ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
        return ids, None if live is None else live.to(device=dev, dtype=torch.uint8).contiguous()

    # ------------------------------------------------------------------------------------------------ forward
    def _run(self, input_ids, attention_mask):
        ids, mask = self._inputs(input_ids, attention_mask)
        w = self._weights()
        B, S = ids.shape
        H, V, P = w["word"].shape[1], w["word"].shape[0], w["pos"].shape[0]
        I, D = w["layers"][0]["inter"][0].shape[0] if w["layers"] else 0, w["linear1"][0].shape[0]
        rows, st, dev = B * S, L.current_stream(), ids.device
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)                    # noqa: E731

        def norm(a, r, gb):
            y = new(rows, H)
            L.call("ds_add_layernorm", a.data_ptr(), r.data_ptr(), gb[0].data_ptr(), gb[1].data_ptr(), rows, H, float(self.eps), y.data_ptr(), st)
            return y

        x = new(rows, H)
        L.call("ds_text_embed", ids.data_ptr(), B, S, self.pad_token_id, w["word"].data_ptr(), V, w["pos"].data_ptr(), P, w["type0"].data_ptr(),
               w["emb_norm"][0].data_ptr(), w["emb_norm"][1].data_ptr(), H, float(self.eps), x.data_ptr(), st)
        for l in w["layers"]:
            qkv = _linear(x, l["qkv"], rows, H, 3 * H)
            ctx = new(rows, H)
            L.call("ds_text_attention", qkv.data_ptr(), L.ptr(mask), 1, B, S, self.heads, H // self.heads, ctx.data_ptr(), st)
            x = norm(_linear(ctx, l["attn_out"], rows, H, H), x, l["attn_norm"])
            mid = _linear(x, l["inter"], rows, H, I)
            L.call("ds_activation", mid.data_ptr(), rows * I, L.ACT_GELU, mid.data_ptr(), st)       # once, not per 16 outputs of the next linear
            x = norm(_linear(mid, l["out"], rows, I, H), x, l["out_norm"])
        pooled = _linear(x, w["pooler"], B, H, H, x_stride=S * H)                                    # the first token's row of every sample
        L.call("ds_text_tail", pooled.data_ptr(), B, H, L.TAIL["DS_TAIL_TANH"], 0.0, pooled.data_ptr(), st)
        hidden = _linear(pooled, w["linear1"], B, H, D)
        L.call("ds_text_tail", hidden.data_ptr(), B, D, L.TAIL["DS_TAIL_RELU"], 0.0, hidden.data_ptr(), st)
        return x.view(B, S, H), pooled, _linear(hidden, w["linear2"], B, D, D)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None):
        """(last_hidden_state (B, S, H), pooler_output (B, H), text_embeds (B, P)), fp32 on the device.  ``attention_mask`` None: all ones."""
        return self._run(input_ids, attention_mask)

    @torch.no_grad()
    def get_text_features(self, input_ids, attention_mask=None, **ignored):
        """The (B, P) unit-norm text feature, fp32 on the device: text_embeds / max(||text_embeds||_2, 1e-12) per row - the tensor the
        reference's callers index with [0].  Takes a tokenizer's dict as keywords; token_type_ids and position_ids are ignored (one token type,
        positions by RoBERTa's rule from input_ids).  Inputs may live on either device."""
        embeds = self._run(input_ids, attention_mask)[2]
        L.call("ds_text_tail", embeds.data_ptr(), embeds.shape[0], embeds.shape[1], L.TAIL["DS_TAIL_L2NORM"], 1e-12, embeds.data_ptr(),
               L.current_stream())
        return embeds
