"""Batch-dependent launch decisions at every batch serving can form (SamplingBatcher: any integer U-Net batch, changing from tick to tick).

Which kernel, which template instantiation, how many K slices, how many row ranges a launch gets is decided from the batch.  The census
(test_ladder_covers_every_decision_class) builds the dry plan for every batch 1 .. 256, groups the batches by what their launches DECIDED
(_PlanBuilder.launch_signature()) and checks that LADDER — a committed constant — holds both ends of every class, so a rule that changes
fails here with the batches that went uncovered.  The ladder is then run: every class against the fp32 tier (documented batch-invariant,
pinned to the reference goldens at 2e-6) evaluated in batches of two, every sample compared; and the paired (classifier-free guidance)
plan against the plain plan, bit for bit.

No number here comes from the code under test: the bounds are the tiers' existing ones (test_hip_unet.py), the classes come from the
plans, the reference is the fp32 tier.

What makes a class: the categorical part of launch_signature() — kernel family, tile, K slices, flags, the two-samples-per-block
predicate, the depthwise launch's family and row ranges / chunks per image, the attention generations.  The two COUNTS of an attention
block (segments of the context pass, GroupNorm partials per sample of the output pass) are budgets divided by the batch: they change at
almost every batch (with them every second batch would be a class of its own: 129 - 135 classes in the bf16 tier) and select no other
code path, so they are kept apart; the census prints the values met on the ladder and holds the segment counts to NSEG_ON_LADDER, which
tests/test_hip_kernels.py sweeps against the float64 oracle at 64 x 64.

Measured on an MI355X (profiles/batch_ladder_errors.txt has every batch): bf16x3 at most 1.8e-5 per call and 2.0e-5 for the worst single
sample (bound 1e-4); bf16 at most 1.15e-2 per call and 1.34e-2 for the worst single sample (bound 1.5e-2) — the per-sample form holds the
existing bounds, no margin was added.  The file takes 23 s of a 97 s suite run."""
import collections

import pytest
import torch

from conftest import rel_err
from diffusynth_amd.synth import synth_input

pytestmark = pytest.mark.gpu

BMAX = 256
SIZES = {"256x64": (256, 64), "128x64": (128, 64)}
SMALL = (16, 8)        # a latent whose FIRST level fits the halo kernel's two-samples-per-block tile (at most 16 x 8): the pair predicate could
#                        differ between a paired plan's prefix at B = 1 and the plain plan at B = 2 (dry plans only: see the bits test)
TOL = {"bf16x3": 1e-4,      # test_unet_forward_bf16x3_matches_reference: the tier's level (measured 1e-5)
       "bf16": 1.5e-2}      # BF16_TOL of test_hip_unet.py

# Both ends of every decision class of the batches 1 .. 256: its smallest member and, where it has more than one, its largest member not
# above 128.  Computed by the census from the plans, committed as a constant; the census test fails when a rule moves a boundary.
_X3 = (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 14, 15, 16, 21, 22, 28, 29, 31, 32, 42, 43, 56, 57, 63, 64, 85, 86, 128, 171)
LADDER = {
    ("bf16x3", "256x64"): _X3,
    ("bf16x3", "128x64"): _X3,
    ("bf16", "256x64"): (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 14, 15, 16, 21, 22, 23, 24, 28, 29, 31, 32, 42, 43, 44, 46, 47, 48, 49, 55, 56, 57, 58, 62,
                         63, 64, 65, 69, 81, 84, 85, 86, 87, 89, 93, 94, 95, 96, 97, 99, 115, 123, 125, 127, 128, 171, 172, 173, 175, 215),
    ("bf16", "128x64"): (1, 3, 4, 7, 8, 10, 11, 12, 14, 15, 16, 21, 22, 23, 24, 28, 29, 31, 32, 42, 43, 44, 46, 47, 48, 49, 55, 56, 57, 58, 62, 63, 64,
                         65, 69, 81, 84, 85, 86, 87, 89, 93, 94, 95, 96, 97, 99, 112, 114, 115, 123, 125, 127, 128, 129, 171, 172, 173, 175),
    ("fp32", "256x64"): (1, 128),       # one class (the tier is batch-invariant): its two ends
    ("fp32", "128x64"): (1, 128),
}
# (segments of the context pass, by channel count) met on the ladders: what tests/test_hip_kernels.py sweeps `nseg` over at 64 x 64
NSEG_ON_LADDER = {
    "bf16x3": {96: (8, 11, 12, 16, 17, 18, 23, 24, 32, 33, 35, 36, 46, 48, 64, 68, 73, 93, 102, 128),
               192: (8, 11, 12, 16, 17, 18, 23, 24, 32, 33, 35, 36, 46, 48, 64, 68, 73, 93, 102, 128),
               384: (4, 8, 9, 11, 12, 16, 17, 18, 23, 24, 32)},
    "bf16": {96: (9, 11, 15, 16, 17, 18, 20, 21, 32), 192: (9, 11, 15, 16, 17, 18, 20, 21, 32), 384: (1, 2, 4, 5, 8, 10)},
}


@pytest.fixture(scope="module")
def unet(unet_sd):
    from diffusynth_amd.unet import ConditionedUnet, PRODUCTION_CONFIG
    assert torch.cuda.is_available()
    m = ConditionedUnet(**PRODUCTION_CONFIG)
    m.load_state_dict(unet_sd)
    return m.to("cuda")


_ENGINES = {}


def _engine(unet, tier):
    """An engine of its own for the dry plans (the model's engine keeps its plan cache to itself)."""
    from diffusynth_amd.engine import UnetEngine
    if tier not in _ENGINES or _ENGINES[tier][0] is not unet:
        _ENGINES[tier] = (unet, UnetEngine(unet, tier))
    return _ENGINES[tier][1]


def _signature(eng, B, H, W, paired=False):
    """Dry run (records the launches, touches no device memory): (categorical, counts, channels of the attention blocks)."""
    from diffusynth_amd.engine import _PlanBuilder
    pb = _PlanBuilder(eng, B, H, W, True, paired)
    pb.build(4096)
    cat, counts = pb.launch_signature()
    chans = tuple(op.args[0]._obj.C for op in pb.ops if op.name in ("ds_attn_x3_context", "ds_attn_fused_context"))
    return cat, counts, chans


def _census(eng, H, W):
    """classes: categorical signature -> its batches (ascending); counts: batch -> ((nseg, partials), ...); chans: the blocks' channels."""
    classes, counts, chans = collections.OrderedDict(), {}, ()
    for B in range(1, BMAX + 1):
        cat, counts[B], ch = _signature(eng, B, H, W)
        classes.setdefault(cat, []).append(B)
        chans = ch or chans
    return classes, counts, chans


def _class_ends(classes):
    ends = set()
    for members in classes.values():
        ends.add(members[0])
        upto128 = [b for b in members if b <= 128]
        if len(members) > 1 and upto128:
            ends.add(upto128[-1])
    return ends


def _nseg_by_channels(batches, counts, chans):
    seen = collections.defaultdict(set)
    for B in batches:
        for (nseg, _), ch in zip(counts[B], chans):
            seen[ch].add(nseg)
    return {ch: tuple(sorted(v)) for ch, v in sorted(seen.items())}


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("tier", ["bf16x3", "bf16"])
def test_ladder_covers_every_decision_class(unet, tier, size):
    H, W = SIZES[size]
    classes, counts, chans = _census(_engine(unet, tier), H, W)
    ladder = set(LADDER[(tier, size)])
    print(f"{tier} {size}: {len(classes)} decision classes of the batches 1 .. {BMAX}: " + ", ".join(
        f"{m[0]}" if len(m) == 1 else f"{m[0]}..{m[-1]} ({len(m)})" for m in classes.values()))
    missing = sorted(_class_ends(classes) - ladder)
    assert not missing, f"{tier} {size}: batches {missing} are ends of a decision class and not on LADDER — a launch rule moved; add them"
    seen = _nseg_by_channels(ladder, counts, chans)
    print(f"{tier} {size}: attention segments (nseg) met on the ladder, by channel count: {seen}")
    print(f"{tier} {size}: GroupNorm partials per sample of the attention output pass met on the ladder: "
          f"{sorted({p for B in ladder for _, p in counts[B]})}")
    rec = NSEG_ON_LADDER[tier]
    unrecorded = {ch: sorted(set(v) - set(rec.get(ch, ()))) for ch, v in seen.items() if set(v) - set(rec.get(ch, ()))}
    assert not unrecorded, f"{tier} {size}: segment counts {unrecorded} are met on the ladder and not recorded in NSEG_ON_LADDER"


@pytest.mark.parametrize("size", list(SIZES))
def test_fp32_tier_takes_the_same_decisions_at_every_batch(unet, size):
    """The parity tier is documented as batch-invariant: one signature, segment counts included, for every batch 1 .. 256."""
    H, W = SIZES[size]
    classes, counts, _ = _census(_engine(unet, "fp32"), H, W)
    assert len(classes) == 1, [m[0] for m in classes.values()]
    assert len(set(counts.values())) == 1
    assert set(LADDER[("fp32", size)]) >= _class_ends(classes)


# ---------------------------------------------------------------------------------------------------------------- ladder parity
_INPUTS, _REFS = {}, {}


def _inputs(H, W):
    """Sample i is the same in every batch that holds it: batch B is the first B of BMAX samples, t = (arange(B) * 13) % 1000."""
    if (H, W) not in _INPUTS:
        _INPUTS[(H, W)] = (synth_input(f"ladder_x_{H}x{W}", (BMAX, 4, H, W)).cuda(), ((torch.arange(BMAX) * 13) % 1000).cuda(),
                           synth_input("ladder_c", (BMAX, 512)).cuda())
    return _INPUTS[(H, W)]


def _reference(unet, H, W, n):
    """The fp32 tier on samples [0, n) in batches of two (the configuration the reference goldens pin at 2e-6), computed once per size."""
    x, t, c = _inputs(H, W)
    ref = _REFS.setdefault((H, W), torch.empty(0, 4, H, W, device="cuda"))
    have = ref.shape[0]
    n = min(BMAX, n + n % 2)
    if have < n:
        unet.set_compute_dtype("fp32")
        ref = _REFS[(H, W)] = torch.cat([ref] + [unet(x[i:i + 2], t[i:i + 2], c[i:i + 2]).clone() for i in range(have, n, 2)])
    return ref


def _per_sample_errs(got, want):
    """Per sample: (max |d| / max |want|, ||d|| / ||want||), each sample against its OWN reference scale."""
    d, w = (got - want).double().flatten(1), want.double().flatten(1)
    return d.abs().amax(1) / w.abs().amax(1).clamp_min(1e-30), d.norm(dim=1) / w.norm(dim=1).clamp_min(1e-30)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("tier", ["bf16x3", "bf16"])
def test_ladder_matches_the_fp32_tier(unet, tier, size):
    """One forward per ladder batch in the tier under test against the fp32 tier in batches of two, EVERY sample compared.  The tier's
    existing bound holds for the call as a whole (rel_err: max norm and rms over the batch) and for each sample against its own reference
    scale — one wrong sample in a batch of 128 is diluted by sqrt(128) in the rms norm and hidden from the max norm by a larger sample."""
    H, W = SIZES[size]
    tol = TOL[tier]
    x, t, c = _inputs(H, W)
    ladder = sorted(LADDER[(tier, size)], reverse=True)          # (largest first: the arena is sized once)
    ref = _reference(unet, H, W, ladder[0])
    bad = []
    try:
        unet.set_compute_dtype(tier)
        for B in ladder:
            y = unet(x[:B], t[:B], c[:B]).clone()
            y2 = unet(x[:B], t[:B], c[:B])
            whole = rel_err(y, ref[:B])
            smax, srms = _per_sample_errs(y, ref[:B])
            print(f"{tier} {size} B={B:3d}: batch rel_err {whole:.2e} | worst sample: max-norm {smax.max().item():.2e} (sample {smax.argmax().item()}) "
                  f"rms {srms.max().item():.2e} (sample {srms.argmax().item()})")
            if not torch.isfinite(y).all():
                bad.append((B, "non-finite output"))
            if not torch.equal(y, y2):
                bad.append((B, "second call returned other bits"))
            if not whole < tol:
                bad.append((B, f"batch rel_err {whole:.2e}"))
            worst = torch.maximum(smax, srms)
            if not (worst < tol).all():
                bad.append((B, f"samples {torch.nonzero(~(worst < tol)).flatten().tolist()[:8]} up to {worst.max().item():.2e}"))
    finally:
        unet.set_compute_dtype("fp32")
    assert not bad, f"{tier} {size}, bound {tol}: {bad}"


# ---------------------------------------------------------------------------------------------------------------- paired == plain
def _first_difference(a, b):
    a, b = [o for o in a if o[0] != "ds_dup_batch"], [o for o in b if o[0] != "ds_dup_batch"]
    if len(a) != len(b):
        return f"{len(a)} ops against {len(b)}"
    for k, (u, v) in enumerate(zip(a, b)):
        if u != v:
            return f"op {k}: plain {u}, paired {v}"
    return None


@pytest.mark.parametrize("size", list(SIZES) + ["16x8"])
@pytest.mark.parametrize("tier", ["fp32", "bf16x3", "bf16"])
def test_cfg_paired_plan_takes_the_plain_plans_decisions(unet, tier, size):
    """Dry, every even batch 2 .. 256: the paired plan — its shared prefix at half the batch included — decides op for op what the plain
    plan decides (the ds_dup_batch ops aside).  Names the op and the batches where the two plans part."""
    H, W = SIZES.get(size, SMALL)
    eng = _engine(unet, tier)
    parted = {}
    for B in range(2, BMAX + 1, 2):
        diff = _first_difference(_signature(eng, B, H, W)[0], _signature(eng, B, H, W, paired=True)[0])
        if diff:
            parted[B] = diff
    assert not parted, f"{tier} {size}: the plans part at {len(parted)} batches {sorted(parted)}; first: {next(iter(parted.items()))}"


def _half_batches(tier, size):
    """Half batches b of the ladder (and 64: the doubled batch 128 of the headline configuration) with 2 b <= 128."""
    return sorted(b for b in set(LADDER[(tier, size)]) | {64} if 2 * b <= 128)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("tier", ["fp32", "bf16x3", "bf16"])
def test_cfg_paired_is_the_plain_plan_on_the_ladder(unet, tier, size):
    """unet(cat([x, x]), cat([t, t]), c) and the same call with paired_halves=True: the same bits at every half batch of the ladder —
    equal signatures (the dry test above) do mean equal bits.  (No forward at the 16 x 8 latent of the dry test: its deepest level is
    2 x 1, which the convolution entry point rejects — the library runs no such latent, in either plan.)"""
    H, W = SIZES[size]
    x, t, c = _inputs(H, W)
    moved = []
    try:
        unet.set_compute_dtype(tier)
        for b in sorted(_half_batches(tier, size), reverse=True):
            xx, tt = torch.cat([x[:b], x[:b]]), torch.cat([t[:b], t[:b]])
            plain = unet(xx, tt, c[:2 * b]).clone()
            paired = unet(xx, tt, c[:2 * b], paired_halves=True)
            assert torch.isfinite(plain).all(), (tier, size, b)
            assert not torch.equal(plain[:b], plain[b:])          # (the halves do differ: different conditions)
            if not torch.equal(plain, paired):
                d = (plain - paired).abs().max().item() / plain.abs().max().item()
                moved.append((2 * b, f"{d:.1e}"))
    finally:
        unet.set_compute_dtype("fp32")
    print(f"{tier} {size}: paired against plain at U-Net batches {[2 * b for b in _half_batches(tier, size)]}: "
          f"{'all bit-identical' if not moved else 'bits moved at ' + str(moved)}")
    assert not moved, f"{tier} {size}: paired != plain at U-Net batches (relative difference) {moved}"
