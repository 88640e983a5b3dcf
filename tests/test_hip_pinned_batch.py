"""The pinned launch batch (ConditionedUnet.pin_launch_batch) on the GPU: with every batch-dependent launch decision taken from the pin,
a sample's result is the same bits in whatever batch, at whatever position, it travels — in the bf16x3 and bf16 tiers, where unpinned
plans group fp32 partial sums by the batch (split-K, depthwise family and row ranges, attention segments and blocks per sample).

The contract, for a model pinned at P in any tier:
  (a) model(x, t, c)[i] is torch.equal to model(x[i:i+1], t[i:i+1], c[i:i+1])[0] for every B >= 1 and every position i;
  (b) the paired (CFG) plan equals the plain plan bit for bit;
  (c) pinned at P, a batch of exactly P is torch.equal to the unpinned model at that batch;
  (d) unpinned, nothing changes (the untouched suite).

Latents: 128 x 64 (the reference's own size; the smallest at which the depthwise family and row ranges part by batch, and its deepest
level, 16 x 8, runs the two-samples-per-tile convolution), 128 x 27 (ragged tiles) and 16 x 8 (SMALL of test_hip_batch_ladder.py: the FIRST
level fits the pair tile).  The 16 x 8 latent takes part in the dry tests only: its deepest level is 2 x 1, which the convolution entry
point rejects in either plan (test_hip_batch_ladder.py says the same of its bits test) — the pair tile's bits are covered by the deepest
level of the 128-row latents, where a lone sample, an odd batch and both positions of a pair all occur.  No latent can run a FIRST-level
pair tile: the tile needs W <= 8 there, the deepest level is then one column wide (8 / 2^3), and the 3 x 3 convolutions' border classes
need W >= 2 (32 x 8 ends at 4 x 1 and is rejected like 16 x 8).  The pair launch is the same code at whichever level it is taken.

Bounds are the tiers' existing ones (test_hip_batch_ladder.py: 1e-4 bf16x3, 1.5e-2 bf16, per sample, no margin); the reference is the
fp32 tier; every bit comparison is torch.equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err
from diffusynth_amd.synth import synth_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = {"128x64": (128, 64), "128x27": (128, 27), "16x8": (16, 8)}
RUN_SIZES = ("128x64", "128x27")            # (16 x 8: dry plans only, see the module docstring)
TIERS = ("bf16x3", "bf16")
PINS = (1, 16, 128)
BATCHES = (1, 2, 3, 5, 8, 16)
NMAX = 17                                   # 17 under pin 16: a batch above the pin
TOL = {"bf16x3": 1e-4, "bf16": 1.5e-2}      # test_hip_batch_ladder.py's


def _batches(pin):
    return BATCHES + ((17,) if pin == 16 else ())


@pytest.fixture(scope="module")
def unet(unet_sd):
    from diffusynth_amd.unet import ConditionedUnet, PRODUCTION_CONFIG
    assert torch.cuda.is_available()
    m = ConditionedUnet(**PRODUCTION_CONFIG)
    m.load_state_dict(unet_sd)
    return m.to("cuda")


class _as:
    """with _as(unet, tier, pin): ... — the shared model in that tier under that pin; fp32 and unpinned afterwards."""

    def __init__(self, unet, tier, pin):
        self.unet, self.tier, self.pin = unet, tier, pin

    def __enter__(self):
        return self.unet.set_compute_dtype(self.tier).pin_launch_batch(self.pin)

    def __exit__(self, *exc):
        self.unet.set_compute_dtype("fp32").pin_launch_batch(None)


_INPUTS = {}


def _inputs(size):
    """Sample i is the same in every batch that holds it: batch B is the first B of NMAX samples."""
    if size not in _INPUTS:
        H, W = SIZES[size]
        _INPUTS[size] = (synth_input(f"pin_x_{H}x{W}", (NMAX, 4, H, W)).cuda(), ((torch.arange(NMAX) * 61 + 7) % 1000).cuda(),
                         synth_input("pin_c", (NMAX, 512)).cuda())
    return _INPUTS[size]


# ---------------------------------------------------------------------------------------------------------------- dry plans
_ENGINES = {}


def _engine(unet, tier):
    """An engine of its own for the dry plans (the model's engine keeps its plan cache to itself)."""
    from diffusynth_amd.engine import UnetEngine
    if tier not in _ENGINES or _ENGINES[tier][0] is not unet:
        _ENGINES[tier] = (unet, UnetEngine(unet, tier))
    return _ENGINES[tier][1]


def _signature(eng, pin, B, H, W, paired=False):
    """Dry run under `pin` (records the launches, touches no device memory): (categorical, counts) of launch_signature()."""
    from diffusynth_amd.engine import _PlanBuilder
    eng.launch_batch = pin
    try:
        pb = _PlanBuilder(eng, B, H, W, True, paired)
        pb.build(4096)
        return pb.launch_signature()
    finally:
        eng.launch_batch = None


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("tier", TIERS)
def test_unpinned_plans_of_these_batches_decide_differently(unet, tier, size):
    """The shapes can see the problem: with no pin the chosen batches do not share one (categorical, counts) signature — the fp32 partial
    sums of a sample are grouped by who travels with it.  (Passes without the feature; it is why the other tests mean something.)"""
    H, W = SIZES[size]
    eng = _engine(unet, tier)
    # (a 16 x 8 latent is one tile per level: its launches fill the chip, and stop splitting K, only from about a hundred samples on)
    batches = BATCHES + ((64, 128, 256) if size == "16x8" else ())
    sigs = {B: _signature(eng, None, B, H, W) for B in batches}
    distinct = len(set(sigs.values()))
    print(f"{tier} {size}: unpinned batches {batches} take {distinct} distinct (categorical, counts) signatures")
    assert distinct >= 2


@pytest.mark.parametrize("pin", PINS)
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("tier", TIERS)
def test_pinned_plans_decide_the_same_at_every_batch(unet, tier, size, pin):
    """Dry census under a pin: for every B in 1 .. 64 categorical AND counts are those of B = P — and those of the unpinned plan at P; the
    paired plan of every even B decides op for op what the plain plan decides (the ds_dup_batch ops aside)."""
    H, W = SIZES[size]
    eng = _engine(unet, tier)
    want = _signature(eng, pin, pin, H, W)
    assert want == _signature(eng, None, pin, H, W), f"{tier} {size}: pinned at {pin}, the plan of batch {pin} is not the unpinned plan"
    moved = [B for B in range(1, 65) if _signature(eng, pin, B, H, W) != want]
    assert not moved, f"{tier} {size} pin {pin}: batches {moved} decide differently from batch {pin}"
    strip = lambda cat: tuple(o for o in cat if o[0] != "ds_dup_batch")                     # noqa: E731
    parted = []
    for B in range(2, 65, 2):
        cat, counts = _signature(eng, pin, B, H, W, paired=True)
        if strip(cat) != strip(want[0]) or counts != want[1]:
            parted.append(B)
    assert not parted, f"{tier} {size} pin {pin}: the paired plans of batches {parted} part from the plain plan"


def test_plan_cache_key_holds_the_pin(unet):
    """Changing the pin must not replay a stale plan: one shape under three pins is three cached plans with their own decisions, and going
    round them again builds nothing."""
    x, t, c = _inputs("128x27")
    with _as(unet, "bf16x3", None):
        pins = (1, 128, None)
        for _ in range(2):                                # (twice: a growing arena drops the cached plans once)
            for pin in pins:
                unet.pin_launch_batch(pin)
                unet(x[:2], t[:2], c[:2])
        eng = unet._engine
        n0, out = eng.plan_builds, {}
        for pin in pins + (1,):
            unet.pin_launch_batch(pin)
            out[pin] = unet(x[:2], t[:2], c[:2]).clone()
            assert unet._engine is eng and eng.launch_batch == pin
        assert eng.plan_builds == n0
        mine = [k for k in eng.plans if k[:3] == (2,) + SIZES["128x27"]]
        assert len(mine) == 3 and sorted(k[4:] for k in mine) == [(), ("pin", 1), ("pin", 128)], mine
        sig = {k[4:]: eng.plans[k].launch_signature() for k in mine}
        assert sig[("pin", 1)] != sig[("pin", 128)] and sig[()] == _signature(_engine(unet, "bf16x3"), None, 2, *SIZES["128x27"])
        assert not torch.equal(out[1], out[128])          # (the two pins do group the sums differently: a stale replay would show)


# ---------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("pin", PINS)
@pytest.mark.parametrize("size", RUN_SIZES)
@pytest.mark.parametrize("tier", TIERS)
def test_a_sample_is_the_same_bits_in_every_batch(unet, tier, size, pin):
    """Contract (a): every sample of every batch against the same sample run alone, on the same pinned model."""
    x, t, c = _inputs(size)
    moved = []
    with _as(unet, tier, pin):
        batches = sorted(_batches(pin), reverse=True)                                       # (largest first: the arena is sized once)
        whole = {B: unet(x[:B], t[:B], c[:B]).clone() for B in batches}
        alone = torch.cat([unet(x[i:i + 1], t[i:i + 1], c[i:i + 1]).clone() for i in range(batches[0])])
        assert torch.isfinite(alone).all()
        assert not torch.equal(alone[0], alone[1])
        for B in batches:
            bad = [i for i in range(B) if not torch.equal(whole[B][i], alone[i])]
            if bad:
                d = (whole[B] - alone[:B]).abs().max().item() / alone[:B].abs().max().item()
                moved.append((B, bad[:8], f"{d:.1e}"))
    assert not moved, f"{tier} {size} pin {pin}: (batch, samples that differ from the sample alone, relative difference) {moved}"


@pytest.mark.parametrize("pin", PINS)
@pytest.mark.parametrize("size", RUN_SIZES)
@pytest.mark.parametrize("tier", TIERS)
def test_paired_plan_is_the_plain_plan_under_a_pin(unet, tier, size, pin):
    """Contract (b) at U-Net batches 2, 6 and 16: unet(cat([x, x]), cat([t, t]), c) with and without paired_halves."""
    x, t, c = _inputs(size)
    with _as(unet, tier, pin):
        for B in (16, 6, 2):
            b = B // 2
            xx, tt = torch.cat([x[:b], x[:b]]), torch.cat([t[:b], t[:b]])
            plain = unet(xx, tt, c[:B]).clone()
            paired = unet(xx, tt, c[:B], paired_halves=True)
            assert torch.isfinite(plain).all() and not torch.equal(plain[:b], plain[b:])
            assert torch.equal(plain, paired), (tier, size, pin, B)


@pytest.mark.parametrize("pin", (1, 16))
@pytest.mark.parametrize("size", RUN_SIZES)
@pytest.mark.parametrize("tier", TIERS)
def test_pinned_at_its_own_batch_is_the_unpinned_model(unet, tier, size, pin):
    """Contract (c): every pinned result is tied to a code path the suite already holds to the reference."""
    x, t, c = _inputs(size)
    with _as(unet, tier, None):
        free = unet(x[:pin], t[:pin], c[:pin]).clone()
        unet.pin_launch_batch(pin)
        assert torch.equal(unet(x[:pin], t[:pin], c[:pin]), free)


@pytest.mark.parametrize("size", RUN_SIZES)
def test_fp32_tier_is_unaffected_by_a_pin(unet, size):
    x, t, c = _inputs(size)
    with _as(unet, "fp32", None):
        free = {B: unet(x[:B], t[:B], c[:B]).clone() for B in (5, 1)}
        for pin in (1, 128):
            unet.pin_launch_batch(pin)
            for B in (5, 1):
                assert torch.equal(unet(x[:B], t[:B], c[:B]), free[B]), (pin, B)


# ---------------------------------------------------------------------------------------------------------------- accuracy
def _per_sample_errs(got, want):
    """Per sample: (max |d| / max |want|, ||d|| / ||want||), each sample against its OWN reference scale."""
    d, w = (got - want).double().flatten(1), want.double().flatten(1)
    return d.abs().amax(1) / w.abs().amax(1).clamp_min(1e-30), d.norm(dim=1) / w.norm(dim=1).clamp_min(1e-30)


_REFS = {}


def _reference(unet, size):
    """The fp32 tier on samples [0, 16) in batches of two (the configuration the reference goldens pin), once per size."""
    if size not in _REFS:
        x, t, c = _inputs(size)
        unet.set_compute_dtype("fp32").pin_launch_batch(None)
        _REFS[size] = torch.cat([unet(x[i:i + 2], t[i:i + 2], c[i:i + 2]).clone() for i in range(0, 16, 2)])
    return _REFS[size]


@pytest.mark.parametrize("pin,B", [(1, 16), (128, 1)])
@pytest.mark.parametrize("size", RUN_SIZES)
@pytest.mark.parametrize("tier", TIERS)
def test_extreme_pins_keep_the_tiers_accuracy(unet, tier, size, pin, B):
    """The two combinations no unpinned run produces — pin 1 at batch 16 splits K and segments as far as the rules go with sixteen samples
    in flight, pin 128 at batch 1 splits nothing — against the fp32 tier at the tiers' own bounds, per call and per sample."""
    x, t, c = _inputs(size)
    ref = _reference(unet, size)[:B]
    with _as(unet, tier, pin):
        y = unet(x[:B], t[:B], c[:B]).clone()
    whole = rel_err(y, ref)
    smax, srms = _per_sample_errs(y, ref)
    print(f"{tier} {size} pin {pin} batch {B}: batch rel_err {whole:.2e} | worst sample: max-norm {smax.max().item():.2e} rms {srms.max().item():.2e}")
    assert torch.isfinite(y).all()
    assert whole < TOL[tier]
    assert (torch.maximum(smax, srms) < TOL[tier]).all(), torch.maximum(smax, srms).tolist()


# ---------------------------------------------------------------------------------------------------------------- bounds build
def test_pinned_extremes_stay_inside_their_operands():
    """The same extremes (and a batch above / an odd batch below a pin) through the bounds-checked library, in a child process like
    test_hip_bounds.py: under a pin ksplit and B no longer move together, so slabs and partial buffers are the new risk."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_bounds()                  # no-op when the prebuilt library is up to date
    assert os.path.exists(g.BOUNDS_LIB)
    env = dict(os.environ, DS_LIB="libdiffusynth_hip_bounds.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pinned_batch_bounds_worker.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and "BOUNDS OK" in r.stdout


# ---------------------------------------------------------------------------------------------------------------- serving
def test_batcher_results_are_the_calls_alone_in_the_headline_tier(unet):
    """The mixed workload of test_hip_batching.py (CFG-6 DDPM, DDIM, null condition, guided, inpaint with dynamic masks, interpolate, late
    joiners, widths 27 and 64) in bf16x3 with the model pinned at the batcher's max_rows: every h.result(), each trajectory entry
    included, is the same call alone on the same pinned model, bit for bit — what only the fp32 tier gave before."""
    from test_hip_batching import _mix, _run_alone, _run_batched
    from diffusynth_amd.batching import SamplingBatcher
    mix = _mix("cpu")
    max_rows = SamplingBatcher(unet).max_rows
    with _as(unet, "bf16x3", max_rows):
        b, _, got = _run_batched(unet, mix, max_rows=max_rows)
        _, want = _run_alone(unet, mix)
    assert len(b.unet_batches) > 1                        # (the ticks did run different U-Net batches)
    for i, ((gi, gn), (wi, wn)) in enumerate(zip(got, want)):
        assert torch.equal(gn, wn), i
        assert len(gi) == len(wi), i
        for k, (u, v) in enumerate(zip(gi, wi)):
            assert torch.equal(u, v), (i, k)


def test_shard_is_the_unsharded_run_in_the_headline_tier(unet):
    """The workload of test_sharded_sampling_in_the_headline_tier (bf16x3, the two shards of a CFG batch of 4 against the unsharded run)
    with both sides pinned equally: torch.equal instead of a bound."""
    from diffusynth_amd.sampler import DiffSynthSampler
    cond = synth_input("shard3_c", (4, 512)).cuda()
    unc = synth_input("shard3_u", (512,)).cuda()

    def run(B, shard, c):
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=32, max_batchsize=B, noise_device="cpu", shard=shard)
        s.respace(list(np.linspace(0, 999, 3, dtype=np.int32)))
        s.activate_classifier_free_guidance(3.0, unc)
        return s.sample(unet, (B, 4, 32, 64), return_tensor=True, condition=c, sampler="ddpm", seed=5)[0][-1]

    with _as(unet, "bf16x3", 8):                          # (the unsharded run's U-Net batch: CFG doubles the four samples)
        ref = run(4, None, cond)
        assert torch.isfinite(ref).all()
        for rank in (0, 1):
            assert torch.equal(run(2, (rank, 2), cond[2 * rank:2 * rank + 2]), ref[2 * rank:2 * rank + 2]), rank


def test_graph_replay_is_the_eager_plan_under_a_pin(unet):
    x, t, c = _inputs("128x27")
    with _as(unet, "bf16x3", 16):
        eager = unet(x[:3], t[:3], c[:3]).clone()
        try:
            unet.use_hip_graph(True)
            first = unet(x[:3], t[:3], c[:3]).clone()     # (captures)
            replay = unet(x[:3], t[:3], c[:3]).clone()
        finally:
            unet.use_hip_graph(False)
        assert torch.equal(first, eager) and torch.equal(replay, eager)
