"""Which packed weight forms a convolution gets, which tile its launch uses and how many K slices it splits into: plain functions of
shapes and tier flags.  The split-K rules look at the batch ``B`` they are given: the plan passes its FULL batch (``_PlanBuilder.Btile``),
also while a paired (CFG) plan's shared prefix runs at half of it, so the prefix adds its partial sums in the plain plan's order."""
from collections import namedtuple

KSPLIT_FILL = 256        # split K until this many blocks exist (256 CUs)
# ds_conv_params.tile (include/diffusynth_hip.h; 4 .. 10: retired halo kernel generations)
TILE_128x192, TILE_256x96, TILE_128x32, TILE_64x192 = 0, 1, 2, 3
TILE_HALO3_256x96, TILE_QUAD_HALO3, TILE_HALO3_N16, TILE_INIT7 = 11, 12, 13, 14
_IGEMM_BM_BN = {TILE_64x192: (64, 192), TILE_128x192: (128, 192), TILE_256x96: (256, 96)}


def up(x, m):
    return (x + m - 1) // m * m


class ConvLayer(namedtuple("ConvLayer", "Cout Cin cin_pad k transposed gain halo small_out bf16 split3")):
    """A convolution as packed: Cin = its input channels (also when transposed), k = the weight's kernel size, gain = a GroupNorm gain
    is folded in, halo = a block's single-source 3x3 the caller runs on a halo kernel where the tier has one, bf16 / split3 = the tier.
    The *_fits properties: which weight forms it is packed in besides the generic kernel's (conv() picks one per launch)."""
    bn = property(lambda s: 32 if s.small_out else 192 if s.Cout % 192 == 0 else 96)
    cout_pad = property(lambda s: up(s.Cout, s.bn))
    dense3x3 = property(lambda s: s.k == (3, 3) and not s.transposed and s.cin_pad == s.Cin and s.Cin % 32 == 0)
    # 1: chunk-major weights of the bf16 LDS-halo kernel (conv3x3_halo3.hip); 0: the generic kernel's order
    k_order = property(lambda s: int(s.halo and s.bf16 and s.k == (3, 3) and not s.transposed and s.cin_pad % 32 == 0 and s.bn in (96, 192)))
    # few-output 3x3 of the fp32 / split-precision tiers (the final 96 -> 4 convolution): vector-ALU kernel
    f32n4_fits = property(lambda s: not s.bf16 and not s.gain and s.dense3x3 and s.Cout <= 4)
    # ... of the bf16 tier: 16-row chunk-major tiles for conv3x3_smalln.hip
    n16_fits = property(lambda s: s.bf16 and not s.gain and s.dense3x3 and s.Cout <= 16)
    # 1x1 of the split-precision tier (to_qkv, to_out, res_conv): pre-split hi / lo weights for ds_conv1x1_x3
    x3_1x1_fits = property(lambda s: s.split3 and s.k == (1, 1) and not s.transposed and s.cin_pad == s.Cin and s.Cin % 32 == 0
                           and s.Cout % 8 == 0)
    # halo 3x3 of the split-precision tier (Cout % 8: its kernels store bf16-style 8-channel groups into a tensor sized for fp32)
    split3_fits = property(lambda s: s.halo and s.split3 and s.dense3x3 and s.cout_pad % 96 == 0 and s.Cout % 8 == 0)
    # the U-Net's 7x7 init convolution on its own kernel (four real channels = 8 bytes per pixel); split precision: the fp32 input split
    # into hi / lo bf16 on its way to LDS
    init7_fits = property(lambda s: s.bf16 and s.k == (7, 7) and s.Cout == 96 and s.Cin <= 4 and s.cin_pad in (4, 8))
    init7x3_fits = property(lambda s: s.split3 and s.k == (7, 7) and s.Cout == 96 and s.Cin <= 4 and s.cin_pad == 4)

    @property
    def quad_fits(s):      # Downsample / Upsample of the U-Net: quad tiles for conv_quad_halo3.hip
        return ((s.bf16 or (s.split3 and s.Cout % 8 == 0)) and not s.gain and s.cin_pad == s.Cin and s.Cin % 32 == 0 and s.k == (4, 4)
                and ((s.transposed and (s.Cin // 32) % 6 == 0 and s.Cout % 96 == 0) or (not s.transposed and (s.Cin // 32) % 3 == 0)))


def igemm_tile(bn, npix, korder):
    """The BN family fixed by packing, BM halved on the small-spatial levels so the grid still fills the chip: never a function of B."""
    if korder == 1:
        return TILE_HALO3_256x96
    if bn == 192:
        return TILE_64x192 if npix <= 1024 else TILE_128x192
    return TILE_256x96 if bn == 96 else TILE_128x32


def halo_patches(H, W):
    """256-pixel tiles of the halo kernels over H x W: the narrowest power-of-two width in 8 .. 32 that covers W."""
    twl = 3
    while (1 << twl) < W and twl < 5:
        twl += 1
    return -(-H // (256 >> twl)) * -(-W // (1 << twl))


def _fill(blocks, factors):
    """The smallest of the allowed factors that fills the chip, else the largest allowed; 1 when the grid fills it unsplit."""
    ks = 1
    if blocks < KSPLIT_FILL:
        for c in factors:
            ks = c
            if blocks * c >= KSPLIT_FILL:
                break
    return ks


def halo3_ksplit(B, H, W, cout_pad, ncc, split):
    """3x3 halo launch, ncc chunks of 32 channels.  bf16: powers of two, >= 2 chunks per slice; split precision: also 3, 6, >= 1 chunk."""
    ok = [c for c in ((2, 3, 4, 6, 8) if split else (2, 4, 8)) if ncc % c == 0 and ncc // c >= (1 if split else 2)]
    return _fill(halo_patches(H, W) * (cout_pad // 96) * B, ok)


def quad_ksplit(B, Ho, Wo, cout_pad, nch, split):
    """Down / Upsample on the halo pipeline (Ho x Wo: its grid), nch K chunks: slices of whole groups of six (the loop period)."""
    ok = [c for c in ((2, 3, 4, 6, 8) if split else (2, 4, 8)) if nch % c == 0 and (nch // c) % 6 == 0]
    return _fill(halo_patches(Ho, Wo) * (cout_pad // 96) * B, ok)


def x3_1x1_ksplit(B, Ho, Wo, cout_pad, nq):
    """ds_conv1x1_x3 over nq chunks of 32 input channels: three chunks per slice at least, never an empty last slice."""
    ok = [c for c in (2, 3, 4, 6, 8) if nq // c >= 3 and (c - 1) * -(-nq // c) < nq]
    return _fill(-(-(Ho * Wo) // 256) * (cout_pad // 96) * B, ok)


def igemm_ksplit(B, tile, Ho, Wo, cout_pad, nq, phases):
    """Generic kernel (phases = 4 when transposed), nq K steps: powers of two while the grid is small and the K loop long, no empty slice."""
    if tile not in _IGEMM_BM_BN:
        return 1
    bm, bn = _IGEMM_BM_BN[tile]
    blocks = -(-(Ho * Wo) // bm) * (cout_pad // bn) * B * phases
    ks = 1
    while ks < 8 and blocks * ks < 384 and nq // (ks * 2) >= 6:
        ks *= 2
    while ks > 1 and (ks - 1) * -(-nq // ks) >= nq:
        ks //= 2
    return ks


def conv_meta(tile, B, Ho, Wo, Cout, kh, kw, transposed, cin, cin_real, res_cin=0):
    """(tile, algorithmic FLOPs, description) of a launch: real taps x real channels (padding excluded), + a fused 1x1 over res_cin."""
    flops = 2.0 * B * Ho * Wo * Cout * (16 if transposed else kh * kw) * min(cin, cin_real)
    if res_cin:
        flops += 2.0 * B * Ho * Wo * Cout * res_cin
    return (tile, flops, f"{kh}x{kw}{'T' if transposed else ''} {cin}->{Cout} @{Ho}x{Wo}" + (f" +1x1 {res_cin}" if res_cin else ""))
