"""The split-precision (tier bf16x3) convolution kernels, bit for bit, on exact data (tests/exact_ref.py explains why no tolerance is
needed: on integer operands hi = bf16(v) and lo = bf16(v - hi) are integers too, every bf16 x bf16 product is exact in fp32, and with
the summed magnitudes below 2^24 units every partial sum is exact in any order).  The expected tensor is the float64 value of the
documented algebra x_hi w_hi + x_lo w_hi + x_hi w_lo (no x_lo w_lo), compared with torch.equal.

Every case is built on the CPU by a `*_case` function below, which asserts the case's preconditions BEFORE anything is launched:
  always   x3_margin < 2^24 units, every operand a kernel receives exactly representable in its type;
  xwide    x = integers of 9 - 10 bits (256 <= |x| <= 1023, narrower where the margin asks for it), w = integers of [-2, 2]: at least 25 % of
           the x elements have lo != 0 (every x_lo w_hi product counts);
  wwide    x in [-4, 4], w = integers of 9 - 10 bits: at least 25 % of the weights a kernel reads have lo != 0, counted after the gain is
           folded (x_hi w_lo);
  wide3    (kernels that split fp32 themselves) x = integers up to 2^18, w in {-1, 0, 1}: at least 5 % of the x elements have x != hi + lo,
           with exact ties among the lo roundings; the reference uses the split parts, so a truncated lo fails;
  stats    small sparse integers that meet check_stats: sum and sum of squares come back exactly whatever the slot grouping;
  a case whose output is OUT_SPLIT: at least 50 % of the expected v have lo != 0, at least 1 % have v != hi + lo, with an exact tie.
Where the issue of this file left a range open it is chosen so that the conditions hold at every shape: the bias of the 3x3 fold cases reaches
2^16 (the planes of the OUT_SPLIT store then drop a third part at short reductions too), the narrow operand of the depthwise cases is
+-128 (dw_case).  The operand range follows the reduction length (_LADDER): the first step whose margin stays below 2^24; nothing a kernel computes
enters the choice.  tests/test_exact_ref_x3_cpu.py builds every case again without a GPU.

GELU is inexact by design: test_gelu_behind_split_epilogues isolates it behind an identity convolution and holds it to gelu_fast's bound."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_ref as E
from diffusynth_amd import _lib as L
from test_hip_exact import Case, _seed, _sparse, gelu_fast_bound, gelu_inputs, _identity3x3

BF, F32 = L.DS_BF16, L.DS_F32
NAN = float("nan")
SPLIT_IN, OUT_SPLIT, OUT_F32, IN_F32 = 1, 2, 4, 8          # DS_CONV_F_* (include/diffusynth_hip.h)


def H():
    import hip_helpers
    return hip_helpers


# ===================================================================================================== case builders (CPU only)
def wide(g, shape, top, low=256):
    """Seeded integers of 9 - 10 bits: magnitude in [256, top], random sign, as float64."""
    return torch.randint(low, top + 1, tuple(shape), generator=g).double() * (2.0 * torch.randint(0, 2, tuple(shape), generator=g) - 1.0)


# (top of the wide operand, range of the narrow one as a share of its full range): 9 - 10 bits throughout
_LADDER = [(1023, 1.0), (511, 1.0), (300, 1.0), (300, 0.5), (300, 0.25)]


def _first_within_margin(draw):
    """draw(top, share) -> (margin, case) at the first step of _LADDER whose margin is below 2^24 (a property of the data alone)."""
    for top, share in _LADDER:
        m, c = draw(top, share)
        if m < E.LIMIT:
            c["margin"], c["top"] = m, top
            return c
    E.check_exact(m)


def _xw(g, kind, xshape, wshape, top, share):
    """The two wide data sets: the wide operand 256 .. top, the narrow one [-4, 4] (x) or [-2, 2] (w), narrowed by `share`."""
    if kind == "xwide":
        n = max(1, int(2 * share))
        return wide(g, xshape, top), E.ints(g, wshape, -n, n)
    assert kind == "wwide"
    n = max(1, int(4 * share))
    return E.ints(g, xshape, -n, n), wide(g, wshape, top)


def _check_wide(kind, x, w_read):
    """The share conditions of the two wide sets; w_read = the weights a kernel reads (gain folded)."""
    if kind == "xwide":
        E.check_lo_share(x, 0.25, "xwide x")
    else:
        E.check_lo_share(w_read, 0.25, "wwide w")


@functools.lru_cache(maxsize=None)
def halo_case(shape, cout, kind):
    """3x3 pad 1 with the nine-class GroupNorm fold and bias, gn_numbers as they are; an integer fp32 residual for the OUT_F32 form."""
    B, Cin, Hh, Ww = shape

    def numbers(g):
        a, mean, gamma, beta = E.gn_numbers(g, B, Cin)
        return a[:, 0], mean[:, 0], gamma, beta

    if kind == "stats":
        g = E.gen(_seed("halo3", shape, cout, kind))
        a, mean, gamma, beta = numbers(g)

        def draw(d):
            x, w, b = E.ints(g, shape, -2, 2), E.ints(g, (cout, Cin, 3, 3), -1, 1, density=d), E.ints(g, (cout,), -2, 2)
            return x, w, b, E.conv_x3_fold_ref(x, w, b, gamma, beta, a, mean)
        x, w, b, v = _sparse(draw, 1 / 16)
        r = None
        margin = E.conv_x3_fold_margin(x, w, b, gamma, beta, a, mean)
        E.check_exact(margin)
        E.check_stats(v)
        c = Case(margin=margin, top=2)
    else:
        def draw(top, share):
            g = E.gen(_seed("halo3", shape, cout, kind))
            a, mean, gamma, beta = numbers(g)
            x, w = _xw(g, kind, shape, (cout, Cin, 3, 3), top, share)
            # (the bias reaches 2^16: with it the planes of the OUT_SPLIT store drop a third part at every reduction length)
            b, r = E.ints(g, (cout,), -(1 << 16), 1 << 16), E.ints(g, (B, cout, Hh, Ww), -1000, 1000)
            return E.conv_x3_fold_margin(x, w, b, gamma, beta, a, mean, r), Case(x=x, w=w, b=b, r=r, gn=(a, mean, gamma, beta))
        c = _first_within_margin(draw)
        x, w, b, r = c.x, c.w, c.b, c.r
        a, mean, gamma, beta = c.gn
        _check_wide(kind, x, w * gamma.view(1, -1, 1, 1))
        v = E.conv_x3_fold_ref(x, w, b, gamma, beta, a, mean)
        E.check_out_split(v)
    assert E.is_f32(v) and E.is_bf16(torch.cat(E.split_hi_lo(x))) and E.is_bf16(torch.cat(E.split_hi_lo(w * gamma.view(1, -1, 1, 1))))
    c.update(x=x, w=w, b=b, gamma=gamma, beta=beta, ab=E.gn_ab_tensor(a, mean).view(B, 2), r=r, v=v)
    return c


HALO_CASES = [((2, 96, 8, 64), 192), ((1, 64, 37, 16), 96), ((2, 32, 33, 8), 96), ((1, 96, 9, 27), 96), ((2, 64, 7, 3), 96),
              ((3, 96, 16, 8), 192), ((5, 32, 16, 5), 96)]            # the last two: the two-samples-per-block tile, an odd batch leaves half a block
HALO_SPLITK = [((2, 192, 16, 16), 96, 2), ((2, 192, 16, 16), 96, 3), ((2, 192, 16, 16), 96, 6), ((2, 768, 32, 8), 384, 8)]
OUT_MODES = ["split", "f32", "f32+res"]
KINDS = ["xwide", "wwide"]

CONV1 = {"qkv_fold": (96, 0, 384), "res_two_source": (96, 192, 96), "to_out_residual": (128, 0, 192)}
CONV1_HW = (9, 31)                              # 279 pixels: one full 256-pixel block and a ragged one
# (wide3 on the two bias cases: at 2^18 the fold's fractions leave no margin)
CONV1_RUNS = [(n, k) for n in CONV1 for k in ["xwide", "wwide", "stats"] + ([] if n == "qkv_fold" else ["wide3"])]
WIDE3_DENSITY = {"qkv_fold": 0.5, "res_two_source": 0.2, "to_out_residual": 0.4}


def wide3_x(g, shape):
    """Integers up to 2^18: those beyond 2^16 with a low bit set have x != hi + lo, every one of them by an exact tie of the lo rounding."""
    x = E.ints(g, shape, -(1 << 18), 1 << 18)
    E.check_wide3(x)
    return x


@functools.lru_cache(maxsize=None)
def conv1_case(name, kind):
    """ds_conv1x1_x3 on fp32 tensors: to_qkv with the one-class fold (no bias), res_conv over pad_and_concat(encoder, decoder) with the
    decoder map at (H - 1, W - 3) and offset (0, 1), to_out with bias and an integer fp32 residual."""
    C0, C1, cout = CONV1[name]
    B, (Hh, Ww) = 2, CONV1_HW
    off = (0, 1)
    fold, has_res = name == "qkv_fold", name == "to_out_residual"

    def build(g, x, x1, w, rr=1000):
        gn = None
        b = None if fold else E.ints(g, (cout,), -8, 8)
        r = E.ints(g, (B, cout, Hh, Ww), -rr, rr) if has_res else None
        if fold:
            a, mean, gamma, beta = E.gn_numbers(g, B, C0)
            gn = (a[:, 0], mean[:, 0], gamma, beta)
            margin = E.conv_x3_fold_margin(x, w, None, gamma, beta, gn[0], gn[1], pad=0)
        else:
            margin = E.x3_margin(x, w, b, r, x1=x1, off=off)
        return margin, Case(x=x, x1=x1, w=w, b=b, r=r, gn=gn)

    def value(c):
        if fold:
            a, mean, gamma, beta = c.gn
            return E.conv_x3_fold_ref(c.x, c.w, None, gamma, beta, a, mean, pad=0)
        return E.conv_x3_ref(c.x, c.w, x1=c.x1, off=off) + c.b.view(1, -1, 1, 1)

    xs, x1s, ws = (B, C0, Hh, Ww), (B, C1, Hh - 1, Ww - 3), (cout, C0 + C1, 1, 1)
    if kind == "stats":
        g = E.gen(_seed("c1", name, kind))

        def draw(d):
            x, x1 = E.ints(g, xs, -2, 2), (E.ints(g, x1s, -2, 2) if C1 else None)
            m, c = build(g, x, x1, E.ints(g, ws, -1, 1, density=d), rr=2)
            c["margin"] = m
            return c, value(c) + (c.r if has_res else 0)          # the statistics count the stored values: the residual is in them
        c, v = _sparse(draw, 1 / 4)
        E.check_stats(v)
    elif kind == "wide3":
        assert not fold
        g = E.gen(_seed("c1", name, kind))
        x, x1 = wide3_x(g, xs), (wide3_x(g, x1s) if C1 else None)
        m, c = build(g, x, x1, E.ints(g, ws, -1, 1, density=WIDE3_DENSITY[name]))
        c["margin"] = m
    else:
        def draw(top, share):
            g = E.gen(_seed("c1", name, kind))
            x, w = _xw(g, kind, xs, ws, top, share)
            x1 = None
            if C1:
                x1 = wide(g, x1s, top) if kind == "xwide" else E.ints(g, x1s, -4, 4)
            return build(g, x, x1, w)
        c = _first_within_margin(draw)
        wr = c.w * c.gn[2].view(1, -1, 1, 1) if fold else c.w
        _check_wide(kind, torch.cat([c.x.flatten(), c.x1.flatten()]) if C1 else c.x, wr)
    E.check_exact(c.margin)
    v = value(c)
    assert E.is_f32(v) and E.is_f32(c.x) and (c.x1 is None or E.is_f32(c.x1))
    c.update(v=v, out=v + c.r if has_res else v, off=off, ab=E.gn_ab_tensor(*c.gn[:2]).view(B, 2) if fold else None)
    return c


QUAD_CASES = [("up", 192, 96, (9, 27)), ("up", 384, 96, (32, 8)), ("down", 96, 192, (18, 54)), ("down", 384, 384, (32, 16))]


@functools.lru_cache(maxsize=None)
def quad_case(mode, cin, cout, hw, kind):
    """Conv2d(4, 2, 1) / ConvTranspose2d(4, 2, 1) with bias on an fp32 tensor that ds_split_planes re-stores as planes."""
    tr = mode == "up"
    B = 2
    xs, ws = (B, cin, *hw), ((cin, cout, 4, 4) if tr else (cout, cin, 4, 4))
    geo = dict(stride=2, pad=1, transposed=tr)
    if kind == "stats":
        g = E.gen(_seed("quad3", mode, cin, cout, hw, kind))

        def draw(d):
            x, w, b = E.ints(g, xs, -2, 2), E.ints(g, ws, -1, 1, density=d), E.ints(g, (cout,), -2, 2)
            return x, w, b, E.conv_x3_ref(x, w, **geo) + b.view(1, -1, 1, 1)
        x, w, b, v = _sparse(draw, 1 / 16)
        E.check_stats(v)
        c = Case(x=x, w=w, b=b, margin=E.x3_margin(x, w, b, **geo))
    else:
        def draw(top, share):
            g = E.gen(_seed("quad3", mode, cin, cout, hw, kind))
            x, w = _xw(g, kind, xs, ws, top, share)
            b = E.ints(g, (cout,), -8, 8)
            return E.x3_margin(x, w, b, **geo), Case(x=x, w=w, b=b)
        c = _first_within_margin(draw)
        _check_wide(kind, c.x, c.w)
        v = E.conv_x3_ref(c.x, c.w, **geo) + c.b.view(1, -1, 1, 1)
    E.check_exact(c.margin)
    assert E.is_f32(v) and E.is_f32(c.x) and E.is_bf16(torch.cat(E.split_hi_lo(c.w)))
    c["v"] = v
    return c


C7_CASES = [((37, 45), 4, 0.4), ((9, 100), 3, 0.5)]


@functools.lru_cache(maxsize=None)
def c7_case(hw, cin, density, kind):
    """7x7 pad 3 over <= 4 real fp32 channels, split inside the kernel; the stored channel beyond cin holds a non-zero integer."""
    B = 2
    g = E.gen(_seed("c7x3", hw, cin, kind))
    if kind == "wide3":
        x, w = wide3_x(g, (B, cin, *hw)), E.ints(g, (96, cin, 7, 7), -1, 1, density=density)
    else:
        x, w = E.ints(g, (B, cin, *hw), -4, 4), wide(g, (96, cin, 7, 7), 1023)
        _check_wide(kind, x, w)
    b = E.ints(g, (96,), -8, 8)
    margin = E.x3_margin(x, w, b, pad=3)
    E.check_exact(margin)
    v = E.conv_x3_ref(x, w, pad=3) + b.view(1, -1, 1, 1)
    xp = torch.cat([x, E.ints(g, (B, 4 - cin, *hw), 1, 9)], 1) if cin < 4 else x
    assert E.is_f32(v) and E.is_f32(xp)
    return Case(x=x, xp=xp, w=w, b=b, v=v, margin=margin)


PLANES_CASES = [(279, 96), (35, 8), (1, 32)]


def planes_case(npix, Cc):
    return wide3_x(E.gen(_seed("planes", npix, Cc)), (npix, Cc))


DW_CASES = [((64, 16), (96, 0)), ((70, 37), (32, 64)), ((33, 20), (96, 96))]


@functools.lru_cache(maxsize=None)
def dw_case(hw, c01, kind):
    """fp32 depthwise 7x7 over pad_and_concat(x0, x1 one row / three columns smaller at (0, 1)), bias, integer time bias per sample.  Plain
    fp32 fma: any integers with sum |x||w| below 2^24 are exact, and the one rounding site is the split store, which needs |v| beyond
    2^16 to drop a third part - out of reach with w in [-2, 2] (49 taps of at most 1023 x 2), so the narrow operand of the two wide sets
    is +-128 here: 49 x 1023 x 128 = 6.4e6 stays below 2^24."""
    (Hh, Ww), (c0, c1) = hw, c01
    B, Cc = 2, c0 + c1
    g = E.gen(_seed("dwx3", hw, c01, kind))
    s0, s1, wsh = (B, c0, Hh, Ww), (B, c1, Hh - 1, Ww - 3), (Cc, 1, 7, 7)
    ref = lambda x0, x1, w, b, tb: F.conv2d(E.pad_concat(x0, x1, (0, 1), Hh, Ww), w, b, padding=3, groups=Cc) + tb[:, 5:5 + Cc, None, None]
    if kind == "stats":
        def draw(d):
            x0, x1 = E.ints(g, s0, -2, 2), (E.ints(g, s1, -2, 2) if c1 else None)
            w, b, tb = E.ints(g, wsh, -1, 1, density=d), E.ints(g, (Cc,), -1, 1), E.ints(g, (B, Cc + 12), -2, 2)
            return x0, x1, w, b, tb, ref(x0, x1, w, b, tb)
        x0, x1, w, b, tb, v = _sparse(draw, 1 / 4)
        E.check_stats(v)
    else:
        if kind == "xwide":
            x0, x1, w = wide(g, s0, 1023), (wide(g, s1, 1023) if c1 else None), E.ints(g, wsh, -128, 128)
        else:
            x0, x1, w = E.ints(g, s0, -128, 128), (E.ints(g, s1, -128, 128) if c1 else None), wide(g, wsh, 1023)
        b, tb = E.ints(g, (Cc,), -8, 8), E.ints(g, (B, Cc + 12), -16, 16)
        _check_wide(kind, torch.cat([x0.flatten(), x1.flatten()]) if c1 else x0, w)
        v = ref(x0, x1, w, b, tb)
        E.check_out_split(v)
    margin = E.exactness_margin(E.pad_concat(x0, x1, (0, 1), Hh, Ww), w, b, tb, pad=3, groups=Cc)
    E.check_exact(margin)
    assert E.is_f32(v) and E.is_f32(x0) and E.is_f32(w)
    return Case(x0=x0, x1=x1, w=w, b=b, tb=tb, v=v, margin=margin)


N4_CASES = [((2, 96, 37, 19), 4), ((1, 32, 16, 16), 3), ((2, 64, 5, 70), 1)]


def n4_case(shape, cout):
    """fp32 3x3 to at most four outputs: fp32 integers, plain fp32 arithmetic."""
    g = E.gen(_seed("n4", shape, cout))
    x, w, b = E.ints(g, shape, -255, 255), E.ints(g, (cout, shape[1], 3, 3), -31, 31), E.ints(g, (cout,), -8, 8)
    E.check_exact(E.exactness_margin(x, w, b, pad=1))
    return Case(x=x, w=w, b=b, v=F.conv2d(x, w, b, padding=1))


GELU_SHAPE = (1, 96, 8, 16)                     # 96 x 128 = 12288 slots for the 4612 inputs


def gelu_case(seed):
    """x_hi over every bf16 value of magnitude 2^-14 .. 16 plus +-0; x_lo = +-m 2^(e - 16), m in [0, 128], e the exponent of x_hi: a bf16
    value with |lo| <= 2^-9 |hi|, and hi + lo is exact in fp32 (17 bits)."""
    B, Cc, Hh, Ww = GELU_SHAPE
    hi = gelu_inputs(Cc * Hh * Ww, seed).view(GELU_SHAPE).double()
    g = E.gen(seed + 1)
    e = torch.floor(torch.log2(hi.abs().clamp_min(2.0 ** -20)))
    lo = E.ints(g, GELU_SHAPE, -128, 128) * torch.exp2(e - 16) * (hi != 0)
    assert E.is_bf16(hi) and E.is_bf16(lo) and E.is_f32(hi + lo) and (lo.abs() <= 2.0 ** -9 * hi.abs()).all()
    return hi, lo


def lone_case():
    """Statistics of values that DROP a third part, exact all the same: every sample has ONE non-zero output (x non-zero at one pixel in
    two channels, w at the centre tap of one output channel; no bias, no fold), so whatever the slot grouping the sums are v itself and
    the fp32 rounding of v^2 - and differ from those of hi + lo, which a kernel that counted after the split would return."""
    B, Cin, Hh, Ww, cout = 3, 64, 16, 8, 96
    x, w = torch.zeros(B, Cin, Hh, Ww, dtype=torch.float64), torch.zeros(cout, Cin, 3, 3, dtype=torch.float64)
    for b, xv in enumerate((1021.0, 1017.0, -1013.0)):
        x[b, 3, b + 1, b], x[b, 40, b + 1, b] = xv, (1.0 if xv > 0 else -1.0)
    w[5, 3, 1, 1], w[5, 40, 1, 1] = 1019.0, 259.0
    E.check_exact(E.x3_margin(x, w, pad=1))
    v = E.conv_x3_ref(x, w, pad=1)
    return Case(x=x, w=w, b=None, v=v, want=lone_stats(v))


def lone_dw_case():
    """The same for the fp32 depthwise kernels (32 channels at (33, 20), where both the tile and the strip kernel run): v = 1021 x 1279."""
    B, Cc, Hh, Ww = 2, 32, 33, 20
    x0, w = torch.zeros(B, Cc, Hh, Ww, dtype=torch.float64), torch.zeros(Cc, 1, 7, 7, dtype=torch.float64)
    x0[0, 7, 10, 5], x0[1, 7, 31, 19], w[7, 0, 3, 3] = 1021.0, -1021.0, 1279.0
    v = F.conv2d(x0, w, None, padding=3, groups=Cc)
    return Case(x0=x0, x1=None, w=w, b=torch.zeros(Cc, dtype=torch.float64), tb=torch.zeros(B, Cc + 12, dtype=torch.float64), v=v, want=lone_stats(v))


def lone_stats(v):
    """(v, fp32(v^2)) of the one non-zero output of every sample; asserts that it is one, and that its planes drop a third part."""
    nz = v.flatten(1)
    assert ((nz != 0).sum(1) == 1).all()
    one = nz.sum(1)
    hi, lo = E.split_hi_lo(one)
    assert (one != hi + lo).all() and E.is_f32(one)
    want = torch.stack([one, (one * one).float().double()], 1)
    assert not torch.equal(want, torch.stack([hi + lo, ((hi + lo) ** 2).float().double()], 1))
    return want


def all_cpu_cases():
    """Every case of this file, built on the CPU (preconditions asserted inside the builders): tests/test_exact_ref_x3_cpu.py runs this."""
    n = 0
    for shape, cout in HALO_CASES + sorted(set(s[:2] for s in HALO_SPLITK)):
        for kind in KINDS + ["stats"]:
            halo_case(shape, cout, kind)
            n += 1
    for name, kind in CONV1_RUNS:
        conv1_case(name, kind)
        n += 1
    for q in QUAD_CASES:
        for kind in KINDS + ["stats"]:
            quad_case(*q, kind)
            n += 1
    for c in C7_CASES:
        for kind in ("wide3", "wwide"):
            c7_case(*c, kind)
            n += 1
    for p in PLANES_CASES:
        planes_case(*p)
        n += 1
    for d in DW_CASES:
        for kind in KINDS + ["stats"]:
            dw_case(*d, kind)
            n += 1
    for c in N4_CASES:
        n4_case(*c)
        n += 1
    gelu_case(1)
    lone_case()
    lone_dw_case()
    return n + 3


# ===================================================================================================== device plumbing
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    L.load()


def f32dev(t):
    assert E.is_f32(t)
    return t.float().contiguous().cuda()


def nhwc_f32(x):
    """Exact NCHW float64 (cpu) -> NHWC fp32 device tensor."""
    assert E.is_f32(x)
    return x.float().permute(0, 2, 3, 1).contiguous().cuda()


def planes_dev(hi, lo):
    """NCHW float64 parts -> the SPLIT_IN tensor: NHWC bf16 [..., hi plane | lo plane]; the conversion must not round."""
    assert E.is_bf16(hi) and E.is_bf16(lo)
    return torch.cat([hi, lo], 1).float().permute(0, 2, 3, 1).contiguous().cuda().bfloat16()


def nchw(y):
    return y.float().permute(0, 3, 1, 2).contiguous().cpu()


def stat_sums(st):
    return st.double().sum(1).cpu()


def assert_planes_equal(out, v, cout, what):
    """out: NHWC bf16 [..., 2 cout]; v: the exact values (NCHW float64): both planes of the OUT_SPLIT store, bit for bit."""
    got = nchw(out)
    hi, lo = E.store_split(v)
    E.assert_bits_equal(got[:, :cout], hi.float(), what + ", hi plane")
    E.assert_bits_equal(got[:, cout:], lo.float(), what + ", lo plane")


def conv_params(xd, cin_planes, wpk, cout, cout_pad, out, out_C, **kw):
    B, Hh, Ww, _ = xd.shape
    f = dict(src0=xd.data_ptr(), src1=None, C0=cin_planes, C1=0, H=Hh, W=Ww, H1=0, W1=0, off_h1=0, off_w1=0, wpk=wpk.data_ptr(), Cout=cout,
             cout_pad=cout_pad, KH=3, KW=3, stride=1, pad_h=1, pad_w=1, Ho=Hh, Wo=Ww, transposed=0, out=out.data_ptr(), out_C=out_C,
             out_c0=0, out_nchw_f32=0, bias=None, gn_ab=None, fold_t1=None, fold_t2=None, ncls=1, act=L.ACT_NONE, res=None, stats_part=None,
             B=B, dtype=BF, tile=L.TILE_HALO3_256x96, wk_order=1)
    f.update(kw)
    return L.ConvParams(**f)


def launch(p, B, entry="ds_conv_igemm", parts_fn="ds_conv_stats_parts"):
    """entry (+ ds_conv_splitk_reduce when p.ksplit > 1) with zeroed statistics partials; returns the partials."""
    st = torch.zeros(B, getattr(L.load(), parts_fn)(C.byref(p)), 2, device="cuda")
    p.stats_part = st.data_ptr()
    L.call(entry, C.byref(p), L.current_stream())
    if p.ksplit > 1:
        L.call("ds_conv_splitk_reduce", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    return st


class Halo3:
    """One packed split-precision 3x3 layer: [W_hi | W_lo | W_hi] per chunk (split3_weight, gain folded before the split) and the
    nine-class fold tables from the unsplit fp32 w, gamma, beta."""

    def __init__(self, c, fold=True):
        from diffusynth_amd.engine import split3_weight
        h = H()
        cout, cin = c.w.shape[:2]
        assert E.is_f32(c.w)
        self.pc = h.PackedConv(split3_weight(c.w.float(), c.gamma.float() if fold else None), c.b, BF, L.TILE_HALO3_256x96)
        self.cout, self.cin, self.fold = cout, cin, fold
        if fold:
            self.t1, self.t2 = torch.empty(9 * cout, device="cuda"), torch.empty(9 * cout, device="cuda")
            self.keep = f32dev(c.w), f32dev(c.gamma), f32dev(c.beta)
            L.call("ds_conv_fold_tables", self.keep[0].data_ptr(), L.ptr(self.pc.bias), self.keep[1].data_ptr(), self.keep[2].data_ptr(), cout, cin, 3, 3,
                   self.t1.data_ptr(), self.t2.data_ptr(), L.current_stream())
            self.ab = c.ab.cuda()
        self.xd = planes_dev(*E.split_hi_lo(c.x))

    def run(self, out_mode, res=None, ks=1, act=L.ACT_NONE):
        """Returns (out NHWC, statistics partials, slab or None); out and slab are NaN-filled before the launch."""
        B, Hh, Ww, _ = self.xd.shape
        cout = self.cout
        if out_mode == "split":
            out, out_C, flags = torch.full((B, Hh, Ww, 2 * cout), NAN, device="cuda").bfloat16(), 2 * cout, SPLIT_IN | OUT_SPLIT
        else:
            out, out_C, flags = torch.full((B, Hh, Ww, cout), NAN, device="cuda"), cout, SPLIT_IN | OUT_F32
        kw = dict(bias=L.ptr(self.pc.bias), act=act, res=L.ptr(res), flags=flags)
        if self.fold:
            kw.update(gn_ab=self.ab.data_ptr(), fold_t1=self.t1.data_ptr(), fold_t2=self.t2.data_ptr(), ncls=9)
        p = conv_params(self.xd, 2 * self.cin, self.pc.w, cout, self.pc.cout_pad, out, out_C, **kw)
        slab = None
        if ks > 1:
            slab = torch.full((ks, B, Hh * Ww, (cout + 7) // 8 * 8), NAN, device="cuda")
            p.ksplit, p.slab = ks, slab.data_ptr()
        return out, launch(p, B), slab


def check_halo_modes(layer, c, what, ks=1):
    """The three output forms of a wide case: OUT_SPLIT, OUT_F32, OUT_F32 with the integer fp32 residual (added after the fold, exact)."""
    cout = layer.cout
    for mode in OUT_MODES:
        rd = nhwc_f32(c.r) if mode == "f32+res" else None
        out, _, slab = layer.run(mode, rd, ks)
        assert slab is None or torch.isfinite(slab).all(), "%s: a slab element was not written" % what
        if mode == "split":
            assert_planes_equal(out, c.v, cout, "%s, OUT_SPLIT" % what)
        else:
            E.assert_bits_equal(nchw(out), E.store(c.v + c.r if rd is not None else c.v, False), "%s, %s" % (what, mode))


def check_halo_stats(layer, s, what, ks=1):
    for mode in ("split", "f32"):
        out, st, _ = layer.run(mode, None, ks)
        if mode == "split":
            assert_planes_equal(out, s.v, layer.cout, "%s statistics case, OUT_SPLIT" % what)
        else:
            E.assert_bits_equal(nchw(out), E.store(s.v, False), "%s statistics case, OUT_F32" % what)
        E.assert_stats_exact(stat_sums(st), s.v, "%s, %s" % (what, mode))


# ===================================================================================================== ds_split_planes
@pytest.mark.parametrize("npix,Cc", PLANES_CASES)
def test_split_planes(npix, Cc):
    x = planes_case(npix, Cc)
    xd = f32dev(x)
    out = torch.full((npix, 2 * Cc), NAN, device="cuda").bfloat16()
    L.call("ds_split_planes", xd.data_ptr(), out.data_ptr(), npix, Cc, L.current_stream())
    torch.cuda.synchronize()
    hi, lo = E.store_split(x)
    got = out.float().cpu()
    E.assert_bits_equal(got[:, :Cc], hi.float(), "split_planes (%d, %d), hi plane" % (npix, Cc))
    E.assert_bits_equal(got[:, Cc:], lo.float(), "split_planes (%d, %d), lo plane" % (npix, Cc))


# ===================================================================================================== DS_CONV_TILE_HALO3_256x96, SPLIT_IN
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,cout", HALO_CASES)
def test_halo3_x3(shape, cout, kind):
    """32- / 16- / 8-wide tiles, ragged H and W, Cout below and at two N-blocks, the two-samples-per-block tile with an odd batch;
    nine-class fold, ACT_NONE, the three output forms."""
    c = halo_case(shape, cout, kind)
    check_halo_modes(Halo3(c), c, "halo3 x3 %s -> %d (%s, +-%d)" % (shape, cout, kind, c.top))


@pytest.mark.parametrize("shape,cout", HALO_CASES)
def test_halo3_x3_statistics(shape, cout):
    s = halo_case(shape, cout, "stats")
    check_halo_stats(Halo3(s), s, "halo3 x3 %s -> %d" % (shape, cout))


@pytest.mark.parametrize("shape,cout,ks", HALO_SPLITK)
def test_halo3_x3_split_k(shape, cout, ks):
    """K slices of whole source chunks (hi chunk twice, lo chunk once) -> fp32 slab -> ds_conv_splitk_reduce in its three out_modes of this
    tier (planes, fp32, fp32 + residual); (2, 768, 32, 8) at 8: slices of three chunks, the loop's odd-count peel."""
    for kind in KINDS:
        c = halo_case(shape, cout, kind)
        check_halo_modes(Halo3(c), c, "halo3 x3 split-K %d %s -> %d (%s, +-%d)" % (ks, shape, cout, kind, c.top), ks)
    s = halo_case(shape, cout, "stats")
    check_halo_stats(Halo3(s), s, "halo3 x3 split-K %d %s -> %d" % (ks, shape, cout), ks)


# ===================================================================================================== ds_conv1x1_x3
def _run_conv1(c, name, ks=1):
    from diffusynth_amd.engine import pack_x3_1x1
    C0, C1, cout = CONV1[name]
    B, (Hh, Ww) = 2, CONV1_HW
    fold = c.gn is not None
    assert E.is_f32(c.w)
    wpk, cout_pad = pack_x3_1x1(c.w.float().cuda(), c.gn[2].float().cuda() if fold else None)
    xd0, xd1 = nhwc_f32(c.x), (nhwc_f32(c.x1) if C1 else None)
    out = torch.full((B, Hh, Ww, cout), NAN, device="cuda")
    keep = []
    kw = dict(src1=L.ptr(xd1), C1=C1, H1=Hh - 1 if C1 else 0, W1=Ww - 3 if C1 else 0, off_h1=c.off[0] if C1 else 0, off_w1=c.off[1] if C1 else 0,
              KH=1, KW=1, pad_h=0, pad_w=0, tile=0, flags=IN_F32 | OUT_F32)
    if fold:
        wd, gd, bd = f32dev(c.w), f32dev(c.gn[2]), f32dev(c.gn[3])
        t1, t2, ab = torch.empty(cout, device="cuda"), torch.empty(cout, device="cuda"), c.ab.cuda()
        L.call("ds_conv_fold_tables", wd.data_ptr(), None, gd.data_ptr(), bd.data_ptr(), cout, C0, 1, 1, t1.data_ptr(), t2.data_ptr(), L.current_stream())
        keep += [wd, gd, bd, t1, t2, ab]
        kw.update(gn_ab=ab.data_ptr(), fold_t1=t1.data_ptr(), fold_t2=t2.data_ptr())
    else:
        keep.append(f32dev(c.b))
        kw.update(bias=keep[-1].data_ptr())
    if c.r is not None:
        keep.append(nhwc_f32(c.r))
        kw.update(res=keep[-1].data_ptr())
    p = conv_params(xd0, C0, wpk, cout, cout_pad, out, cout, **kw)
    slab = None
    if ks > 1:
        slab = torch.full((ks, B, Hh, Ww, cout), NAN, device="cuda")
        p.ksplit, p.slab = ks, slab.data_ptr()
    st = launch(p, B, "ds_conv1x1_x3", "ds_conv1x1_x3_stats_parts")
    assert slab is None or torch.isfinite(slab).all(), "a slab element was not written"
    return nchw(out), stat_sums(st)


@pytest.mark.parametrize("name,kind", CONV1_RUNS)
def test_conv1x1_x3(name, kind):
    """fp32 tensors split inside the kernel; whole-K and every admissible split-K factor (no empty slice, the existing test's rule); the
    zeros of the second source's pad region count as lo = 0; wide3 (the two bias cases): a truncated lo plane would differ on an eighth of the inputs."""
    c = conv1_case(name, kind)
    want = E.store(c.out, False)
    nq = (CONV1[name][0] + CONV1[name][1]) // 32
    for ks in (1, 2, 3, 4, 6, 8):
        if ks > 1 and (ks - 1) * (-(-nq // ks)) >= nq:
            continue
        got, sums = _run_conv1(c, name, ks)
        what = "conv1x1_x3 %s (%s), ksplit %d" % (name, kind, ks)
        E.assert_bits_equal(got, want, what)
        if kind == "stats":
            E.assert_stats_exact(sums, c.out, what)


# ===================================================================================================== DS_CONV_TILE_QUAD_HALO3, SPLIT_IN | OUT_F32
@pytest.mark.parametrize("kind", KINDS + ["stats"])
@pytest.mark.parametrize("mode,cin,cout,hw", QUAD_CASES)
def test_quad_halo3_x3(mode, cin, cout, hw, kind):
    """Input planes written by ds_split_planes, weights [W_hi | W_hi | W_lo] as quad tiles, fp32 output; whole-K and every admissible
    split-K factor; the statistics case also checks the partials."""
    from diffusynth_amd.engine import pack_quad_weights
    tr = mode == "up"
    B, (Hh, Ww) = 2, hw
    c = quad_case(mode, cin, cout, hw, kind)
    wh, wl = E.split_hi_lo(c.w)
    wpk, cout_pad = pack_quad_weights(torch.cat([wh, wh, wl], 0 if tr else 1).float().cuda(), tr)
    xd, bd = nhwc_f32(c.x), f32dev(c.b)
    xs = torch.full((B, Hh, Ww, 2 * cin), NAN, device="cuda").bfloat16()
    L.call("ds_split_planes", xd.data_ptr(), xs.data_ptr(), B * Hh * Ww, cin, L.current_stream())
    oh, ow = (2 * Hh, 2 * Ww) if tr else (Hh // 2, Ww // 2)
    gh, gw = (Hh, Ww) if tr else (oh, ow)
    nch = (1 if tr else 4) * 3 * cin // 32
    want = E.store(c.v, False)
    for ks in (1, 2, 3, 4, 6, 8):
        if ks > 1 and (nch % ks or (nch // ks) % 6):
            continue
        out = torch.full((B, oh, ow, cout), NAN, device="cuda")
        p = conv_params(xs, 2 * cin, wpk, cout, cout_pad, out, cout, KH=2 if tr else 4, KW=2 if tr else 4, stride=1 if tr else 2, pad_h=0 if tr else 1,
                        pad_w=0 if tr else 1, Ho=gh, Wo=gw, transposed=int(tr), bias=bd.data_ptr(), tile=L.TILE_QUAD_HALO3, wk_order=2,
                        flags=SPLIT_IN | OUT_F32)
        slab = None
        if ks > 1:
            slab = torch.full((ks, B, oh, ow, (cout + 7) // 8 * 8), NAN, device="cuda")
            p.ksplit, p.slab = ks, slab.data_ptr()
        st = launch(p, B)
        what = "quad x3 %s %d -> %d %s, ksplit %d (%s)" % (mode, cin, cout, hw, ks, kind)
        assert slab is None or torch.isfinite(slab).all(), what
        E.assert_bits_equal(nchw(out), want, what)
        if kind == "stats":
            E.assert_stats_exact(stat_sums(st), c.v, what)


# ===================================================================================================== ds_conv7x7_c4_x3
@pytest.mark.parametrize("kind", ["wide3", "wwide"])
@pytest.mark.parametrize("hw,cin,density", C7_CASES)
def test_conv7x7_c4_x3(hw, cin, density, kind):
    c = c7_case(hw, cin, density, kind)
    B, (Hh, Ww) = 2, hw
    xd, wd, bd = nhwc_f32(c.xp), f32dev(c.w), f32dev(c.b)
    wp = torch.empty(2 * L.load().ds_conv7x7_c4_weight_elems(), dtype=torch.bfloat16, device="cuda")
    st = L.current_stream()
    L.call("ds_pack_conv7x7_c4_x3", wd.data_ptr(), 96, cin, wp.data_ptr(), st)
    out = torch.full((B, Hh, Ww, 96), NAN, device="cuda")
    L.call("ds_conv7x7_c4_x3", xd.data_ptr(), B, Hh, Ww, wp.data_ptr(), bd.data_ptr(), out.data_ptr(), st)
    torch.cuda.synchronize()
    E.assert_bits_equal(nchw(out), E.store(c.v, False), "conv7x7_c4_x3 %s cin %d (%s)" % (hw, cin, kind))


# ===================================================================================================== ds_dwconv7, fp32
def _run_dw(c, hw, c01, strip, split):
    (Hh, Ww), (c0, c1) = hw, c01
    B, Cc = 2, c0 + c1
    x0, x1 = nhwc_f32(c.x0), (nhwc_f32(c.x1) if c1 else None)
    wd, bd, tbd = f32dev(c.w), f32dev(c.b), f32dev(c.tb)
    wt = torch.empty(49 * Cc, device="cuda")
    L.call("ds_pack_dw_weight", wd.data_ptr(), Cc, wt.data_ptr(), L.current_stream())
    out = torch.full((B, Hh, Ww, Cc), NAN, device="cuda")
    p = L.DwconvParams(src0=x0.data_ptr(), src1=L.ptr(x1), C0=c0, C1=c1, H=Hh, W=Ww, H1=Hh - 1 if c1 else 0, W1=Ww - 3 if c1 else 0, off_h1=0,
                       off_w1=1 if c1 else 0, wt=wt.data_ptr(), bias=bd.data_ptr(), tbias=tbd.data_ptr() + 4 * 5, tb_stride=Cc + 12, out=out.data_ptr(),
                       stats_part=None, B=B, dtype=F32, out_split=split, strip=strip)
    parts = L.load().ds_dwconv_stats_parts(C.byref(p))
    st = torch.zeros(B, parts, 2, device="cuda")
    p.stats_part = st.data_ptr()
    L.call("ds_dwconv7", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    return (out.view(torch.bfloat16).view(B, Hh, Ww, 2 * Cc) if split else out), stat_sums(st), parts


@pytest.mark.parametrize("kind", KINDS + ["stats"])
@pytest.mark.parametrize("hw,c01", DW_CASES)
def test_dwconv7_f32(hw, c01, kind):
    """Tile kernel (strip = 2) and strip kernel (strip = 1), plane and fp32 output, two sources with the pad offsets, integer time bias per
    sample; the two kernels agree bit for bit and both with the reference; the statistics case checks the partials of both."""
    c = dw_case(hw, c01, kind)
    Cc = c01[0] + c01[1]
    for split in (1, 0):
        outs, parts = [], []
        for strip in (2, 1):
            out, sums, np_ = _run_dw(c, hw, c01, strip, split)
            what = "dwconv7 fp32 %s %s (%s), strip %d, out_split %d" % (hw, c01, kind, strip, split)
            if split:
                assert_planes_equal(out, c.v, Cc, what)
            else:
                E.assert_bits_equal(nchw(out), E.store(c.v, False), what)
            if kind == "stats":
                E.assert_stats_exact(sums, c.v, what)
            outs.append(out)
            parts.append(np_)
        assert torch.equal(outs[0].view(torch.int16 if split else torch.int32), outs[1].view(torch.int16 if split else torch.int32))
        assert parts[0] != parts[1], "a different number of partials shows that the strip kernel did run"


# ===================================================================================================== statistics before the split
def test_statistics_are_counted_before_the_split():
    """The statistics sets hold bf16 numbers (check_stats), for which v and hi + lo coincide.  Here every sample has one non-zero output
    that drops a third part: the partials must sum to (v, fp32(v^2)) exactly - halo3_epilogue_hp with planes and with fp32 output (the
    two-samples-per-block tile, an odd batch), ds_conv_splitk_reduce in both forms, the fp32 depthwise tile and strip kernels with planes."""
    c = lone_case()
    layer = Halo3(c, fold=False)
    for ks in (1, 2):
        for mode in ("split", "f32"):
            out, st, _ = layer.run(mode, None, ks)
            what = "lone outputs, %s, ksplit %d" % (mode, ks)
            if mode == "split":
                assert_planes_equal(out, c.v, layer.cout, what)
            else:
                E.assert_bits_equal(nchw(out), E.store(c.v, False), what)
            assert torch.equal(stat_sums(st), c.want), "%s: statistics %s, expected %s" % (what, stat_sums(st).tolist(), c.want.tolist())
    d = lone_dw_case()
    for strip in (2, 1):
        out, sums, _ = _run_dw(d, (33, 20), (32, 0), strip, 1)
        assert_planes_equal(out, d.v, 32, "lone outputs, dwconv7 strip %d" % strip)
        assert torch.equal(sums, d.want), "dwconv7 strip %d: statistics %s, expected %s" % (strip, sums.tolist(), d.want.tolist())


# ===================================================================================================== ds_conv3x3_f32_n4
@pytest.mark.parametrize("shape,cout", N4_CASES)
def test_conv3x3_f32_n4(shape, cout):
    B, Cc, Hh, Ww = shape
    c = n4_case(shape, cout)
    xd, wd, bd = nhwc_f32(c.x), f32dev(c.w), f32dev(c.b)
    wpk = torch.empty(L.load().ds_conv3x3_f32_n4_weight_floats(Cc), device="cuda")
    out = torch.full((B, Hh, Ww, 4), NAN, device="cuda")
    L.call("ds_pack_conv3x3_f32_n4", wd.data_ptr(), bd.data_ptr(), cout, Cc, wpk.data_ptr(), L.current_stream())
    L.call("ds_conv3x3_f32_n4", xd.data_ptr(), B, Hh, Ww, Cc, wpk.data_ptr(), out.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    got = nchw(out)
    E.assert_bits_equal(got[:, :cout], E.store(c.v, False), "conv3x3_f32_n4 %s -> %d" % (shape, cout))
    assert (got[:, cout:] == 0).all(), "pad outputs must be exact zeros"


# ===================================================================================================== GELU behind the split epilogues
GELU_ROUTES = [("halo3_epilogue_hp OUT_SPLIT", 1), ("splitk_reduce planes", 3)]


@pytest.mark.parametrize("name,ks", GELU_ROUTES, ids=[r[0].replace(" ", "_") for r in GELU_ROUTES])
def test_gelu_behind_split_epilogues(name, ks):
    """GELU(v) stored as planes, behind a SPLIT_IN 3x3 whose weight is the identity at the centre tap (w_hi = 1, w_lo = 0; no bias, no
    fold): the accumulator is x_hi + x_lo exactly.  x_hi runs over every bf16 value of magnitude 2^-14 .. 16 plus +-0, x_lo is seeded
    with |lo| <= 2^-9 |hi|.  Both routes evaluate gelu_fast (halo3_epilogue_hp: act_const; ds_conv_splitk_reduce), so per element
        |hi + lo - gelu64(x)| <= E_fast(x) + 2^-17 (|gelu64(x)| + E_fast(x)),
    E_fast = gelu_fast_bound of tests/test_hip_exact.py.  The second term is the plane store of g = gelu_fast(x), from its two roundings:
    hi = rne(g) leaves |g - hi| <= half an ulp of g = 2^(e - 8) (e the exponent of g, bf16 has 8 significant bits); r = g - hi is either
    2^(e - 8) itself (a bf16 number: lo = r) or has an exponent of at most e - 9, so lo = rne(r) leaves |r - lo| <= 2^(e - 9 - 8) =
    2^(e - 17) <= 2^-17 |g|.  (2^-18 does not hold: g = 1 + 2^-9 + 2^-17 gives hi = 1, r = 2^-9 (1 + 2^-8), a tie that rounds to 2^-9 and
    leaves 2^-17, that is 2^-17 / 1.002 of g; the header states the same 2^-17 for the input split.)  Measured on an MI355X: beyond the
    store's term the error reaches 87 % (epilogue) and 85 % (reduce) of E_fast, near x = -3; the whole error 92 % and 88 % of the tolerance,
    and 177 % and 169 % of one that allowed the store 2^-18 only.  The fp32 output form takes no activation (the launcher refuses it:
    test_gelu_has_no_fp32_output_form), so there is no third route."""
    hi, lo = gelu_case(_seed("gelu3", name))
    x = hi + lo
    c = Case(x=x, w=_identity3x3(96, 96), b=None)
    layer = Halo3(c, fold=False)
    layer.xd = planes_dev(hi, lo)                      # the seeded lo, not the split of hi + lo
    assert torch.equal(E.conv_x3_ref(hi, c.w, pad=1, split=lambda t: (hi, lo)), x)   # one non-zero product per part: the accumulator is hi + lo
    out, _, slab = layer.run("split", None, ks, act=L.ACT_GELU)
    assert slab is None or torch.isfinite(slab).all()
    pl = nchw(out).double()
    got = pl[:, :96] + pl[:, 96:]
    ref = E.gelu64(x)
    bound = gelu_fast_bound(x)
    err = (got - ref).abs()
    store_err = 2.0 ** -17 * ref.abs()
    own = (err - store_err).clamp_min(0.0)           # what the store's two roundings cannot explain: a lower bound of the implementation's error
    share = own / bound.clamp_min(1e-30)
    k = share.argmax()
    rel = lambda sh: 100 * (err / (bound + 2.0 ** sh * (ref.abs() + bound)).clamp_min(1e-30)).max().item()
    print("GELU %s: max |got - gelu64(x)| beyond the plane store's 2^-17 |gelu| = %.3e at x = %r, where E = %.3e (%.0f %% of it); whole error at most %.0f %% "
          "of its tolerance (with 2^-18 for the store it would be %.0f %%)"
          % (name, own.flatten()[k].item(), x.flatten()[k].item(), bound.flatten()[k].item(), 100 * share.flatten()[k].item(), rel(-17), rel(-18)))
    tol = bound + 2.0 ** -17 * (ref.abs() + bound)
    worst = (err - tol).argmax()
    assert torch.isfinite(got).all() and (err <= tol).all(), (name, x.flatten()[worst].item(), err.flatten()[worst].item(), tol.flatten()[worst].item())


def test_gelu_has_no_fp32_output_form():
    """The third route the plane tests could have had: the launcher refuses an activation with DS_CONV_F_OUT_F32, whole-K and split-K alike."""
    hi, lo = gelu_case(_seed("gelu3", "fp32"))
    layer = Halo3(Case(x=hi + lo, w=_identity3x3(96, 96), b=None), fold=False)
    for ks in (1, 3):
        with pytest.raises(L.DsError, match="no activation variant"):
            layer.run("f32", None, ks, act=L.ACT_GELU)
