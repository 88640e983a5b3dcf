#!/usr/bin/env python3
"""Child process of tests/test_hip_pinned_batch.py: the production U-Net under a pinned launch batch through the bounds-checked library
(DS_LIB=libdiffusynth_hip_bounds.so, selected before the first load — so not in the test session's process, as tools/bounds_sweep.py).

Under a pin the split-K factors, segment counts and blocks per sample come from the pin while every buffer is sized from the actual batch:
slab = ksplit x B x ..., part = B x nseg x ..., partials = B x parts.  The two extremes no unpinned run produces — pin 1 at batch 16
(maximal splitting everywhere) and pin 128 at batch 1 (none; chunks of several samples with one sample to walk) — and a batch above and
an odd batch below a pin of 16.  Prints one line per group and `BOUNDS OK` when no access left its operand."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("DS_LIB", "libdiffusynth_hip_bounds.so")

import torch  # noqa: E402

from diffusynth_amd import _lib as L  # noqa: E402
from diffusynth_amd.synth import synth_input, synth_state_dict  # noqa: E402

CASES = ((1, 16), (128, 1), (16, 17), (16, 3))      # (pin, batch)
SIZES = ((128, 64), (128, 27))


def main():
    lib = L.load()
    assert "bounds" in L.lib_path(), L.lib_path()
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        keys = json.load(f)
    from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet
    net = ConditionedUnet(**PRODUCTION_CONFIG)
    net.load_state_dict(synth_state_dict([(k, tuple(s)) for k, s in keys["unet_production"]]))
    net.to("cuda")
    fail = []
    for tier in ("bf16x3", "bf16"):
        net.set_compute_dtype(tier)
        for pin, B in CASES:
            net.pin_launch_batch(pin)
            for H, W in SIZES:
                x = synth_input("pb_bounds_x", (B, 4, H, W)).cuda()
                t = torch.arange(B).cuda() * 37 % 1000
                c = synth_input("pb_bounds_c", (B, 512)).cuda()
                y = net(x, t, c)
                finite = bool(torch.isfinite(y).all())
                if B % 2 == 0:
                    finite = finite and bool(torch.isfinite(net(torch.cat([x[:B // 2]] * 2), torch.cat([t[:B // 2]] * 2), c, paired_halves=True)).all())
                buf = C.create_string_buffer(4096)
                n = lib.ds_bounds_report(buf, 4096, 1)
                print(f"[bounds] {tier} pin {pin} batch {B} {H}x{W}: {n} violation record(s) {buf.value.decode()}"
                      f"{'' if finite else ' NON-FINITE OUTPUT'}", flush=True)
                if n != 0 or not finite:
                    fail.append((tier, pin, B, H, W, n))
    if fail:
        print("BOUNDS VIOLATIONS", fail)
        sys.exit(1)
    print("BOUNDS OK")


if __name__ == "__main__":
    main()
