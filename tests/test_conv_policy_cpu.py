"""Host-side convolution policy (diffusynth_amd/conv_policy.py): the split-K factors and tiles the U-Net plan takes at its levels.

The expected values were recorded from the plan builder before these rules moved out of it; a change here changes which partial sums
a launch adds in which order (and the paired-CFG plan's bit identity with the plain plan rests on these rules looking at the batch
they are given and nothing else)."""
import ast
import os

import pytest

from diffusynth_amd import conv_policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 2, 16, 64, 128)
SIZES = ((256, 64), (128, 64))


def levels(H, W):
    """(channels, h, w) of the U-Net levels: 96 @ full, 192 @ 1/2, 384 @ 1/4, 768 @ 1/8 of each side."""
    return [(96, H, W), (192, H // 2, W // 2), (384, H // 4, W // 4), (768, H // 8, W // 8)]


def downs(H, W):
    """(C, input h, input w) of the Downsamples Conv2d(C, C, 4, 2, 1)."""
    return levels(H, W)[:3]


def ups(H, W):
    """(C, input h, input w) of the Upsamples ConvTranspose2d(C, C, 4, 2, 1)."""
    lv = levels(H, W)
    return [(384, lv[3][1], lv[3][2]), (384, lv[2][1], lv[2][2]), (192, lv[1][1], lv[1][2])]


def ones(H, W):
    """(Cin, Cout, h, w) of 1x1 convolutions (res_conv over a skip concat)."""
    lv = levels(H, W)
    return [(192, 96, lv[0][1], lv[0][2]), (384, 192, lv[1][1], lv[1][2]), (768, 384, lv[2][1], lv[2][2]), (768, 384, lv[3][1], lv[3][2])]


def bn_of(Cout):
    return P.ConvLayer(Cout, 32, 32, (1, 1), False, False, False, False, True, False).bn


# one row per batch in BATCHES
HALO3 = {
    ((256, 64), False): [[1, 2, 4, 8], [1, 2, 4, 8], [1, 1, 1, 2], [1, 1, 1, 1], [1, 1, 1, 1]],
    ((256, 64), True): [[3, 6, 6, 8], [3, 6, 6, 8], [1, 1, 1, 2], [1, 1, 1, 1], [1, 1, 1, 1]],
    ((128, 64), False): [[1, 2, 4, 8], [1, 2, 4, 8], [1, 1, 2, 2], [1, 1, 1, 1], [1, 1, 1, 1]],
    ((128, 64), True): [[3, 6, 6, 8], [3, 6, 6, 8], [1, 1, 2, 2], [1, 1, 1, 1], [1, 1, 1, 1]],
}
QUAD = {      # three Downsamples, then three Upsamples
    ((256, 64), False): [[2, 4, 8, 2, 2, 1], [2, 4, 8, 2, 2, 1], [1, 2, 4, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]],
    ((256, 64), True): [[6, 6, 8, 6, 6, 3], [6, 6, 8, 6, 2, 1], [1, 2, 4, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]],
    ((128, 64), False): [[2, 4, 8, 2, 2, 1], [2, 4, 8, 2, 2, 1], [2, 4, 4, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]],
    ((128, 64), True): [[6, 6, 8, 6, 6, 3], [6, 6, 8, 6, 6, 3], [2, 4, 4, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]],
}
IGEMM_TILES = {   # four 1x1, three Downsamples, three Upsamples on the generic kernel
    (256, 64): [1, 0, 3, 3, 1, 3, 3, 3, 3, 0],
    (128, 64): [1, 0, 3, 3, 1, 3, 3, 3, 3, 0],
}
IGEMM = {
    (256, 64): [[1, 2, 4, 4, 8, 8, 8, 8, 4, 4], [1, 2, 4, 4, 8, 8, 8, 8, 2, 2], [1, 1, 1, 4, 2, 2, 4, 1, 1, 1], [1] * 10, [1] * 10],
    (128, 64): [[1, 2, 4, 4, 8, 8, 8, 8, 8, 4], [1, 2, 4, 4, 8, 8, 8, 8, 4, 4], [1, 2, 2, 4, 4, 4, 8, 2, 1, 1],
                [1, 1, 1, 2, 1, 1, 2, 1, 1, 1], [1] * 10],
}
X3_1X1 = {
    (256, 64): [[2, 4, 8, 8], [2, 4, 8, 8], [1, 1, 1, 4], [1, 1, 1, 1], [1, 1, 1, 1]],
    (128, 64): [[2, 4, 8, 8], [2, 4, 8, 8], [1, 1, 2, 4], [1, 1, 1, 1], [1, 1, 1, 1]],
}


def halo3_row(B, H, W, split):
    return [P.halo3_ksplit(B, h, w, c, c // 32, split) for c, h, w in levels(H, W)]


def quad_row(B, H, W, split):
    nch = lambda c: (3 * c // 32) if split else c // 32      # noqa: E731  (K chunks per tap: hi, hi, lo planes in split precision)
    return ([P.quad_ksplit(B, h // 2, w // 2, c, 4 * nch(c), split) for c, h, w in downs(H, W)]
            + [P.quad_ksplit(B, h, w, 4 * c, nch(c), split) for c, h, w in ups(H, W)])


def igemm_shapes(H, W):
    """(Ho, Wo, Cout, nq, phases) of the generic launches."""
    return ([(h, w, co, -(-ci // 32), 1) for ci, co, h, w in ones(H, W)]
            + [(h // 2, w // 2, c, 16 * c // 32, 1) for c, h, w in downs(H, W)]
            + [(h, w, c, 4 * c // 32, 4) for c, h, w in ups(H, W)])


def igemm_row(B, H, W):
    row = []
    for Ho, Wo, Cout, nq, phases in igemm_shapes(H, W):
        tile = P.igemm_tile(bn_of(Cout), Ho * Wo, 0)
        row.append(P.igemm_ksplit(B, tile, Ho, Wo, P.up(Cout, bn_of(Cout)), nq, phases))
    return row


def x3_row(B, H, W):
    return [P.x3_1x1_ksplit(B, h, w, P.up(co, 96), ci // 32) for ci, co, h, w in ones(H, W)]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_halo3_ksplit(size, split):
    assert [halo3_row(B, *size, split) for B in BATCHES] == HALO3[(size, split)]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_quad_ksplit(size, split):
    assert [quad_row(B, *size, split) for B in BATCHES] == QUAD[(size, split)]


@pytest.mark.parametrize("size", SIZES)
def test_igemm_tile_and_ksplit(size):
    assert [P.igemm_tile(bn_of(Cout), Ho * Wo, 0) for Ho, Wo, Cout, _, _ in igemm_shapes(*size)] == IGEMM_TILES[size]
    assert [igemm_row(B, *size) for B in BATCHES] == IGEMM[size]
    # chunk-major (halo) weights pick the halo tile whatever the family; the narrow family has no split-K
    assert P.igemm_tile(192, 64, 1) == P.igemm_tile(96, 1 << 20, 1) == P.TILE_HALO3_256x96
    assert P.igemm_tile(32, 16, 0) == P.TILE_128x32 and P.igemm_ksplit(1, P.TILE_128x32, 4, 4, 32, 600, 1) == 1


@pytest.mark.parametrize("size", SIZES)
def test_x3_1x1_ksplit(size):
    assert [x3_row(B, *size) for B in BATCHES] == X3_1X1[size]


def test_ksplit_rules_look_at_the_given_batch_only():
    """Same arguments, same factor, whatever was asked before (a paired plan's half-batch prefix passes the full batch and must get the
    plain plan's factors); and the batch does move every rule."""
    rows = {
        "halo3": lambda B: halo3_row(B, 256, 64, False) + halo3_row(B, 128, 64, True),
        "quad": lambda B: quad_row(B, 256, 64, False) + quad_row(B, 128, 64, True),
        "igemm": lambda B: igemm_row(B, 256, 64) + igemm_row(B, 128, 64),
        "x3": lambda B: x3_row(B, 256, 64) + x3_row(B, 128, 64),
    }
    for name, row in rows.items():
        first = [row(B) for B in BATCHES]
        again = [row(B) for B in reversed(BATCHES)][::-1]
        assert first == again, name
        assert first[0] != first[-1], name
    assert P.halo3_ksplit(8, 32, 8, 768, 24, False) == P.halo3_ksplit(8, 32, 8, 768, 24, False) == 4


def test_halo_patches_and_conv_meta():
    # tile widths 8 / 16 / 32 by image width, 256 pixels per tile
    assert [P.halo_patches(32, w) for w in (5, 8, 9, 16, 17, 64)] == [1, 1, 2, 2, 4, 8]
    assert P.conv_meta(P.TILE_HALO3_256x96, 2, 16, 8, 192, 3, 3, False, 192, 192, res_cin=96) == (
        P.TILE_HALO3_256x96, 2.0 * 2 * 16 * 8 * 192 * (9 * 192 + 96), "3x3 192->192 @16x8 +1x1 96")
    assert P.conv_meta(P.TILE_64x192, 1, 8, 4, 384, 2, 2, True, 384, 384) == (P.TILE_64x192, 2.0 * 8 * 4 * 384 * 16 * 384, "2x2T 384->384 @8x4")
    assert P.conv_meta(P.TILE_INIT7, 4, 64, 16, 96, 7, 7, False, 4, 4)[1:] == (2.0 * 4 * 64 * 16 * 96 * 49 * 4, "7x7 4->96 @64x16")
    assert P.conv_meta(P.TILE_256x96, 1, 4, 4, 96, 3, 3, False, 16, 4)[1] == 2.0 * 16 * 96 * 9 * 4      # padding channels excluded


def test_packed_forms_by_tier():
    def layer(Cout, Cin, k, tier, cin_pad=None, transposed=False, gain=False, halo=False, small_out=False):
        return P.ConvLayer(Cout, Cin, cin_pad or Cin, k, transposed, gain, halo, small_out, tier == "bf16", tier == "bf16x3")
    conv1 = {t: layer(192, 96, (3, 3), t, gain=True, halo=True) for t in ("fp32", "bf16", "bf16x3")}
    assert [s.k_order for s in conv1.values()] == [0, 1, 0]
    assert [s.split3_fits for s in conv1.values()] == [False, False, True]
    final = {t: layer(4, 96, (3, 3), t, small_out=True) for t in ("fp32", "bf16", "bf16x3")}
    assert [s.f32n4_fits for s in final.values()] == [True, False, True]
    assert [s.n16_fits for s in final.values()] == [False, True, False]
    assert [layer(96, 192, (1, 1), t).x3_1x1_fits for t in ("fp32", "bf16", "bf16x3")] == [False, False, True]
    assert [layer(192, 192, (4, 4), t).quad_fits for t in ("fp32", "bf16", "bf16x3")] == [False, True, True]
    assert layer(384, 384, (4, 4), "bf16", transposed=True).quad_fits and not layer(80, 160, (4, 4), "bf16", transposed=True).quad_fits
    init = {t: layer(96, 4, (7, 7), t, cin_pad=4) for t in ("fp32", "bf16", "bf16x3")}
    assert [(s.init7_fits, s.init7x3_fits) for s in init.values()] == [(False, False), (True, False), (False, True)]


def test_policy_module_is_pure_python():
    with open(os.path.join(ROOT, "diffusynth_amd", "conv_policy.py")) as f:
        tree = ast.parse(f.read())
    imported = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    imported |= {(n.module or "").split(".")[0] or "." for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert imported <= {"collections"}, imported


def test_free_releases_the_statistics_buffer_of_every_form():
    """An activation's GroupNorm statistics come in three forms (engine._Partials / _Finished / _ChanSums); freeing the activation
    returns the buffer of whichever is attached to the arena.  (The finished form once raised a TypeError here and kept its bytes.)"""
    from diffusynth_amd import engine as E
    plan = object.__new__(E._PlanBase)                # free() needs the arena and its base address only: no library, no device
    plan.arena, plan.base = E._Arena(), 4096
    for form in (lambda buf: E._Partials(buf, 3), lambda buf: E._Finished(buf), lambda buf: E._ChanSums(buf, 5)):
        off, n = plan.arena.alloc(1000)
        a = E._Act(plan.base + off, n, 8, 4, 4)
        a.stats = form(plan.raw(64))
        plan.free(a)
        assert a.stats is None and plan.arena.free == [[0, 1 << 62]]
