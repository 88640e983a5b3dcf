#!/usr/bin/env python3
"""Generate tests/golden/clap_text.npz and tests/golden/clap_text_keys.json by running the `transformers` library's own
ClapTextModelWithProjection on synthetic weights.  The only file of this repository that imports `transformers`; run where it is installed.

Nothing is fetched: there is no from_pretrained here.  Each model is built from a config alone, ClapTextModelWithProjection(ClapTextConfig(**cfg)),
and loaded by key and shape with synth_state_dict, so no weight is stored; the two index buffers (text_model.embeddings.position_ids and
.token_type_ids) keep their built-in values.  Configs and input ids are the literals of tests/clap_text_ref.py.

  <input>.last_hidden_state / .pooler_output     model.text_model(input_ids, attention_mask), input in clap_text_ref.INPUTS
  <input>.text_embeds                            model.text_projection(pooler_output) (checked equal to the whole model's text_embeds)
  <input>.text_features                          F.normalize(text_embeds, dim=-1)

These are exactly the lines of ClapModel.get_text_features (text_model -> pooler_output -> text_projection -> F.normalize): the
(B, 512) unit-norm tensor that callers written against transformers 4.x index with [0].  transformers 5.x returns it inside a
BaseModelOutputWithPooling instead, where [0] is last_hidden_state.

clap_text_keys.json: the state-dict key and shape list of every case and of the default production config.  The archive is written with
fixed member dates, so a second run reproduces both files byte for byte."""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clap_text_ref as R  # noqa: E402
from diffusynth_amd.synth import synth_state_dict  # noqa: E402


def build(cfg, load=True):
    from transformers import ClapTextConfig, ClapTextModelWithProjection
    model = ClapTextModelWithProjection(ClapTextConfig(**cfg)).eval()
    spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    if load:
        sd = synth_state_dict([(k, s) for k, s in spec if k not in R.BUFFERS])
        res = model.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys and set(res.missing_keys) <= set(R.BUFFERS), res
    return model, spec


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    out, keys, models = {}, {}, {}
    keys["prod"] = build(R.PROD_CONFIG, load=False)[1]
    with torch.no_grad():
        for name in R.INPUTS:
            case, ids, mask = R.inputs(name)
            if case not in models:
                models[case], keys[case] = build(R.CONFIGS[case])
            res = models[case].text_model(input_ids=ids, attention_mask=mask)
            embeds = models[case].text_projection(res.pooler_output)
            assert torch.equal(embeds, models[case](input_ids=ids, attention_mask=mask).text_embeds)
            out[name + ".last_hidden_state"] = res.last_hidden_state.numpy()
            out[name + ".pooler_output"] = res.pooler_output.numpy()
            out[name + ".text_embeds"] = embeds.numpy()
            out[name + ".text_features"] = F.normalize(embeds, dim=-1).numpy()
    keys["wide"] = build(R.WIDE_CONFIG, load=False)[1]
    path = os.path.join(ROOT, "tests", "golden", "clap_text.npz")
    write_npz(path, out)
    with open(os.path.join(ROOT, "tests", "golden", "clap_text_keys.json"), "w") as f:
        json.dump({k: [[n, list(s)] for n, s in v] for k, v in sorted(keys.items())}, f, indent=0)
    for k, v in out.items():
        print(f"{k:40s} {tuple(v.shape)}  max |.| {np.abs(v).max():.3f}")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
