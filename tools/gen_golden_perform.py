#!/usr/bin/env python3
"""Generate tests/golden/perform.npz by running the reference's own tools.adsr_envelope (tools.py:267-309).

Runs only where the reference tree exists (the path tools/gen_golden.py uses, or --reference); tools.py is loaded at run time with stub
modules for what it imports at module level and adsr_envelope never touches (matplotlib, librosa, scipy.io.wavfile).  Only data is written:

  names                     the cases
  <case>.params  float64 (8,)  signal length, seed of the signal (numpy default_rng(seed).standard_normal(length), float64), sample_rate,
                            duration, attack_time, decay_time, sustain_level, release_time
  <case>.out     float64    what adsr_envelope returned
  refused        float64 (8,)  parameters with release_time > 1 that the function's assert refused

sample_rate is 2000 so that the file stays small; the envelope's arithmetic does not depend on the rate.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SR = 2000
#        name                       length seed duration attack decay sustain release
CASES = (("ordinary",               3600, 1, 0.7, 0.05, 0.1, 0.6, 0.3),
         ("attack_decay_zero",      3000, 2, 0.4, 0.0, 0.0, 1.0, 0.1),
         ("attack_decay_past_hold", 3000, 3, 0.1, 0.2, 0.15, 0.5, 0.25),
         ("one_sample_segments",    2500, 4, 0.0015, 0.0005, 0.0005, 0.25, 0.0005),
         ("release_zero",           3000, 5, 0.3, 0.02, 0.03, 0.8, 0.0),
         ("longer_than_signal",     1500, 6, 0.6, 0.1, 0.1, 0.7, 0.5),
         ("release_one_second",     3500, 7, 0.25, 0.01, 0.2, 0.4, 1.0),
         ("sustain_zero",           3000, 8, 0.3, 0.05, 0.05, 0.0, 0.2))
REFUSED = (3000, 9, 0.3, 0.05, 0.05, 0.5, 1.0005)


def load_tools(ref):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    mpl = stub("matplotlib")
    mpl.pyplot = stub("matplotlib.pyplot")
    stub("librosa")
    sp = stub("scipy")
    sp.io = stub("scipy.io")
    sp.io.wavfile = stub("scipy.io.wavfile", write=None)
    spec = importlib.util.spec_from_file_location("ref_tools", os.path.join(ref, "tools.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def signal(length, seed):
    return np.random.default_rng(int(seed)).standard_normal(int(length))


def main():
    ap = argparse.ArgumentParser()
    from gen_golden import REF
    ap.add_argument("--reference", default=REF)
    args = ap.parse_args()
    tools = load_tools(args.reference)
    out = {"names": np.array([c[0] for c in CASES])}
    for name, length, seed, dur, at, dt, sus, rt in CASES:
        got = tools.adsr_envelope(signal(length, seed), SR, dur, at, dt, sus, rt)
        assert got.dtype == np.float64
        out[name + ".params"] = np.array([length, seed, SR, dur, at, dt, sus, rt], dtype=np.float64)
        out[name + ".out"] = got
        print(f"{name}: {length} samples in, {len(got)} out")
    try:
        tools.adsr_envelope(signal(*REFUSED[:2]), SR, *REFUSED[2:])
        raise SystemExit("the reference accepted release_time > 1")
    except AssertionError:
        out["refused"] = np.array(REFUSED[:2] + (SR,) + REFUSED[2:], dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "perform.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
