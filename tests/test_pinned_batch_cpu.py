"""The pinned launch batch without a GPU: ConditionedUnet.pin_launch_batch's interface, the batch_hint fields of the header-derived structs,
and the purity of the split-K rules in the batch they are given (what lets a plan hand them a pin instead of its own batch)."""
import itertools
import os

import numpy as np
import pytest
import torch

from diffusynth_amd import conv_policy as policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CONFIG = dict(in_dim=4, down_dims=[96, 96], up_dims=[96, 96], mid_depth=1, attn_type="linear_add",
                    condition_type="natural_language_prompt", label_emb_dim=32)


@pytest.fixture(scope="module")
def model():
    from diffusynth_amd.unet import ConditionedUnet
    return ConditionedUnet(**SMALL_CONFIG)


def test_pin_launch_batch_validates_and_returns_self(model):
    assert model.launch_batch is None                     # the default: every call decides from its own batch
    try:
        for n in (1, 16, 128, np.int64(7)):
            assert model.pin_launch_batch(n) is model
            assert model.launch_batch == int(n) and type(model.launch_batch) is int
        assert model.pin_launch_batch(None) is model and model.launch_batch is None
        model.pin_launch_batch(5)
        for bad in (0, -1, 2.0, 1.5, "4", True, False, [1], (2,)):
            with pytest.raises(ValueError):
                model.pin_launch_batch(bad)
            assert model.launch_batch == 5                # a rejected value leaves the pin as it was
    finally:
        model.pin_launch_batch(None)


def test_pin_survives_tier_changes_state_dict_and_moves(model):
    try:
        model.pin_launch_batch(16)
        for tier in ("bf16x3", "bf16", "fp32"):
            assert model.set_compute_dtype(tier) is model
            assert model.launch_batch == 16 and model._engine is None
        model.load_state_dict(model.state_dict())
        assert model.launch_batch == 16
        assert model.to(torch.float32) is model and model.float() is model
        assert model.launch_batch == 16
        assert "launch_batch" not in "".join(model.state_dict().keys())          # like hip_graph: not part of the state dict
    finally:
        model.pin_launch_batch(None)
        model.set_compute_dtype("fp32")


def test_header_derived_structs_carry_batch_hint():
    """Every parameter struct whose launcher takes a reduction-grouping choice from the batch has the field (0 = B), as an int32."""
    import ctypes as C
    from diffusynth_amd import _lib as L
    for st in (L.DwconvParams, L.ConvParams, L.AttnFusedParams, L.AttnX3Params):
        fields = dict(st._fields_)
        assert fields.get("batch_hint") is C.c_int32, st.__name__
        assert st().batch_hint == 0                       # what every caller that never heard of it passes: use B
        assert st(batch_hint=128).batch_hint == 128
    # the field fills padding the structs already had (their kernels take them by value: no argument grew)
    assert C.sizeof(L.ConvParams) % 8 == 0 and L.ConvParams.batch_hint.offset + 4 == L.ConvParams.slab.offset
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        assert f.read().count("int32_t batch_hint;") == 4


_KSPLIT_CASES = [
    ("halo3_ksplit", lambda B: [policy.halo3_ksplit(B, H, W, cp, ncc, split) for (H, W), cp, ncc, split in itertools.product(
        ((128, 64), (64, 32), (32, 16), (16, 8), (128, 27), (16, 4)), (96, 192, 384), (3, 6, 12, 24), (False, True))]),
    ("quad_ksplit", lambda B: [policy.quad_ksplit(B, H, W, cp, nch, split) for (H, W), cp, nch, split in itertools.product(
        ((64, 32), (32, 16), (16, 8), (64, 14)), (96, 384, 1536), (12, 36, 72, 144), (False, True))]),
    ("x3_1x1_ksplit", lambda B: [policy.x3_1x1_ksplit(B, H, W, cp, nq) for (H, W), cp, nq in itertools.product(
        ((128, 64), (32, 16), (16, 8), (128, 27)), (96, 192, 384), (3, 6, 9, 12, 24))]),
    ("igemm_ksplit", lambda B: [policy.igemm_ksplit(B, tile, H, W, cp, nq, ph) for tile, (H, W), cp, nq, ph in itertools.product(
        (policy.TILE_64x192, policy.TILE_128x192, policy.TILE_256x96, policy.TILE_128x32), ((128, 64), (16, 8), (128, 27)), (192, 384),
        (9, 54, 108, 216), (1, 4))]),
]


@pytest.mark.parametrize("name,rule", _KSPLIT_CASES, ids=[c[0] for c in _KSPLIT_CASES])
def test_split_k_rules_are_pure_in_the_batch_they_are_given(name, rule):
    """A plan under a pin hands these rules the pin instead of its batch: the answer for a batch must be a function of the arguments alone —
    the same whatever was asked before, in whatever order — and must not read a batch from anywhere else (the module keeps no state)."""
    batches = list(range(1, 65)) + [85, 86, 128, 171, 256]
    first = {B: rule(B) for B in batches}
    state = {k: v for k, v in vars(policy).items() if not callable(v) and not k.startswith("__")}
    for B in reversed(batches):                           # another order, after every other batch was asked
        assert rule(B) == first[B], (name, B)
    assert {k: v for k, v in vars(policy).items() if not callable(v) and not k.startswith("__")} == state
    assert all(k >= 1 for v in first.values() for k in v)
    assert len({tuple(v) for v in first.values()}) > 1    # (the cases can see the batch at all: the factors do differ between batches)
