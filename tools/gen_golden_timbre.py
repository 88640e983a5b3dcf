#!/usr/bin/env python3
"""Generate tests/golden/timbre.npz and tests/golden/timbre_keys.json by running the reference's own TimbreEncoder
(model/timbre_encoder_pretrain.py) and multi_modal_model (model/multimodal_model.py) on synthetic weights.

Runs only where the reference tree exists (the path tools/gen_golden.py uses, or --reference); the modules are imported at run time through
gen_golden.import_reference().  Only data is written.  Weights are synth_state_dict(keys) and inputs are synth_input tags (tests/timbre_ref.py
names them), so neither is stored:

  prod.w<W>.<output>    production encoder, x (3, 4, 128, W), W in {20, 64}: feature, instrument, instrument_family, velocity, qualities
  small.t<T>.<output>   TimbreEncoder(32, 16, 48, 7, 5, 6, 4, num_layers=2), x (17, 4, 8, T), T in {1, 2, 9}
  mmm.timbre_emb / mmm.text_emb / mmm.logits
                        multi_modal_model over the production encoder (two projection layers, temperature 0.5) with a parameter-free
                        stand-in text encoder that returns its input_ids: get_timbre_features at W = 64, get_text_features of two
                        512-d vectors, and forward()'s logits line applied to the two
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import timbre_ref as R  # noqa: E402


class PassThroughText(torch.nn.Module):
    """Stands where the CLAP tower would: its "text feature" is whatever was passed as input_ids."""

    def get_text_features(self, input_ids, attention_mask=None):
        return input_ids


def main():
    import gen_golden as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    args = ap.parse_args()
    G.REF = args.reference
    G.import_reference()
    import model.multimodal_model as mm
    import model.timbre_encoder_pretrain as te

    out, keys = {}, {}
    with torch.no_grad():
        for case, cfg, inputs in (("prod", R.PROD_CONFIG, [(f"w{W}", R.prod_input(W)) for W in R.PROD_W]),
                                  ("small", R.SMALL_CONFIG, [(f"t{T}", R.small_input(T)) for T in R.SMALL_T])):
            enc = te.TimbreEncoder(**cfg)
            keys[case] = G.load_synth(enc)
            for tag, x in inputs:
                for name, y in zip(R.OUTPUTS, enc(x)):
                    out[f"{case}.{tag}.{name}"] = y.numpy()
        m = mm.multi_modal_model(te.TimbreEncoder(**R.PROD_CONFIG), PassThroughText(), **R.MMM_CONFIG)
        keys["mmm"] = G.load_synth(m)
        timbre_emb = m.get_timbre_features(R.prod_input(R.MMM_W))
        text_emb = m.get_text_features(input_ids=R.text_input(), attention_mask=None)
        out["mmm.timbre_emb"], out["mmm.text_emb"] = timbre_emb.numpy(), text_emb.numpy()
        out["mmm.logits"] = ((text_emb @ timbre_emb.T) / m.temperature).numpy()                    # multimodal_model.py:100
    path = os.path.join(ROOT, "tests", "golden", "timbre.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(ROOT, "tests", "golden", "timbre_keys.json"), "w") as f:
        json.dump({k: [[n, list(s)] for n, s in v] for k, v in keys.items()}, f, indent=0)
    for k, v in out.items():
        print(f"{k:32s} {tuple(v.shape)}  max |.| {np.abs(v).max():.3f}")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
