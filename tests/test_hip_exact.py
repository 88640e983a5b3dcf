"""The bf16 convolution family, bit for bit, on exact integer data (tests/exact_ref.py explains why no tolerance is needed).

Every case is built on the CPU by a `*_case` function below, which also asserts the case's preconditions BEFORE anything is
launched: the exactness margin (sum |x||w| + |bias| + |res| below 2^24 units), for a 'rounding' data set that at least 0.5 % of the
expected outputs need a bf16 rounding with exact ties among them, for a 'statistics' data set that |v| <= 256 units and the
per-sample sum v^2 < 2^24 units.  tests/test_exact_ref_cpu.py builds every case again without a GPU.

GELU is the one epilogue part that is inexact by design: test_gelu_per_implementation isolates it behind an identity convolution
and holds each implementation to its documented bound on every bf16 input of magnitude 2^-14 .. 16."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import exact_ref as E
from diffusynth_amd import _lib as L

BF, F32 = L.DS_BF16, L.DS_F32
NAN = float("nan")


def H():
    import hip_helpers
    return hip_helpers


class Case(dict):
    __getattr__ = dict.__getitem__


def _seed(*key):
    return sum((i + 1) * 7919 * (ord(ch) if isinstance(ch, str) else int(ch)) for i, ch in enumerate(str(key))) % (1 << 31)


def _x_range(K):
    """Operand range of a 'rounding' data set by reduction length: +-4 reaches |v| > 256 from K of about a thousand on; shorter sums
    take wider operands (the issue's example: (2, 64, 7, 3) with +-4 reaches 252 and rounds nothing)."""
    return 4 if K >= 800 else (32 if K >= 100 else 64)


# ===================================================================================================== case builders (CPU only)
def _sparse(draw, d0):
    """A 'statistics' data set: draw(density) -> (tensors, v), at the first density of d0, d0 / 2, d0 / 4, ... whose v meets
    check_stats (the bound on sum v^2 is a property of the data alone; nothing the kernels compute enters the choice)."""
    for k in range(8):
        out = draw(d0 / 2 ** k)
        try:
            E.check_stats(out[-1])
            return out
        except AssertionError as e:
            err = e
    raise err


def halo_case(shape, cout, kind):
    """3x3 pad 1 with the nine-class GroupNorm fold and bias; 'rounding': v (no residual) and v + r; 'stats': v alone."""
    B, Cin, Hh, Ww = shape
    g = E.gen(_seed("halo", shape, cout, kind))
    a, mean, gamma, beta = E.gn_numbers(g, B, Cin)
    a, mean = a[:, 0], mean[:, 0]
    if kind == "rounding":
        xr = _x_range(9 * Cin)
        x, w, b = E.ints(g, shape, -xr, xr), E.ints(g, (cout, Cin, 3, 3), -2, 2), E.ints(g, (cout,), -8, 8)
        r = E.ints(g, (B, cout, Hh, Ww), -16, 16)
        v = E.conv_fold_ref(x, w, b, gamma, beta, a, mean)
    else:
        def draw(d):
            x, w, b = E.ints(g, shape, -2, 2), E.ints(g, (cout, Cin, 3, 3), -1, 1, density=d), E.ints(g, (cout,), -2, 2)
            return x, w, b, E.conv_fold_ref(x, w, b, gamma, beta, a, mean)
        (x, w, b, v), r = _sparse(draw, 1 / 16), None
    E.check_exact(E.conv_fold_margin(x, w, b, gamma, beta, a, mean, r))
    if kind == "rounding":
        E.check_rounding(v)
        E.check_rounding(v + r)
    else:
        E.check_stats(v)
    return Case(x=x, w=w, b=b, gamma=gamma, beta=beta, ab=E.gn_ab_tensor(a, mean).view(B, 2), r=r, v=v)


HALO_SHAPES = [(2, 96, 8, 64), (1, 160, 37, 16), (3, 32, 33, 8), (1, 96, 9, 27), (2, 64, 7, 3)]
HALO_COUTS = [96, 64, 192]
HALO_SPLITK = [(64, 2), (192, 3), (96, 4), (96, 6)]           # (Cout, ksplit) at (2, 384, 20, 8): 12 chunks


def res_conv_case(shape, cx, kind):
    """ConvNeXt conv2 with the block's 1x1 res_conv fused: a * (acc_res / a + acc_3x3) + shift = res_conv(x) + res_bias + conv3x3(GN(g))."""
    B, Cin, Hh, Ww = shape
    cout, (c0, c1) = 96, cx
    g = E.gen(_seed("rf", shape, cx, kind))
    a, mean, gamma, beta = E.gn_numbers(g, B, Cin)
    a, mean = a[:, 0], mean[:, 0]
    h1, w1, off = Hh - 2, Ww - 1, (1, 0)
    if kind == "rounding":
        xr = _x_range(9 * Cin)
        gin, w, b = E.ints(g, shape, -xr, xr), E.ints(g, (cout, Cin, 3, 3), -2, 2), E.ints(g, (cout,), -8, 8)
        x0, x1 = E.ints(g, (B, c0, Hh, Ww), -4, 4), (E.ints(g, (B, c1, h1, w1), -4, 4) if c1 else None)
        wr, br = E.ints(g, (cout, c0 + c1, 1, 1), -2, 2), E.ints(g, (cout,), -8, 8)
        xcat = E.pad_concat(x0, x1, off, Hh, Ww)
    else:
        def draw(d):
            gin, w, b = E.ints(g, shape, -2, 2), E.ints(g, (cout, Cin, 3, 3), -1, 1, density=d), E.ints(g, (cout,), -2, 2)
            x0, x1 = E.ints(g, (B, c0, Hh, Ww), -2, 2), (E.ints(g, (B, c1, h1, w1), -2, 2) if c1 else None)
            wr, br = E.ints(g, (cout, c0 + c1, 1, 1), -1, 1, density=min(1.0, 9 * d)), E.ints(g, (cout,), -2, 2)
            xcat = E.pad_concat(x0, x1, off, Hh, Ww)
            return gin, w, b, x0, x1, wr, br, xcat, E.conv_fold_ref(gin, w, b, gamma, beta, a, mean) + F.conv2d(xcat, wr, br)
        gin, w, b, x0, x1, wr, br, xcat, _ = _sparse(draw, 1 / 16)
    # the accumulator holds acc_res / a + acc_3x3 (a >= 0.5: at most twice the res_conv sum)
    E.check_exact(E.conv_fold_margin(gin, w, b, gamma, beta, a, mean) + 2 * E.exactness_margin(xcat, wr, br, unit=0.25))
    v = E.conv_fold_ref(gin, w, b, gamma, beta, a, mean) + F.conv2d(xcat, wr, br)
    E.check_rounding(v) if kind == "rounding" else E.check_stats(v)
    return Case(gin=gin, w=w, b=b, gamma=gamma, beta=beta, ab=E.gn_ab_tensor(a, mean).view(B, 2), x0=x0, x1=x1, wr=wr, br=br, v=v, off=off,
                h1=h1, w1=w1, c0=c0, c1=c1, cout=cout)


RES_CONV_CASES = [((2, 192, 16, 32), (96, 0)), ((1, 64, 37, 16), (64, 32)), ((2, 96, 9, 27), (96, 96)), ((1, 32, 33, 8), (32, 64))]


def plain_case(tag, xshape, wshape, kind, stride=1, pad=0, transposed=False, x1shape=None, off=(0, 0), wr=2, bias=True):
    """Bias-only convolution (any geometry F.conv2d / F.conv_transpose2d takes), optionally over pad_and_concat(x, x1)."""
    g = E.gen(_seed(tag, xshape, wshape, kind, stride, transposed))
    cout = wshape[1] if transposed else wshape[0]
    K = (wshape[0] if transposed else wshape[1]) * wshape[2] * wshape[3] // (4 if transposed else 1)
    if kind == "rounding":
        xr = _x_range(K)
        x, w, b = E.ints(g, xshape, -xr, xr), E.ints(g, wshape, -wr, wr), E.ints(g, (cout,), -8, 8)
        x1 = E.ints(g, x1shape, -xr, xr) if x1shape else None
    else:
        def draw(d):
            x, w, b = E.ints(g, xshape, -2, 2), E.ints(g, wshape, -1, 1, density=d), E.ints(g, (cout,), -2, 2)
            x1 = E.ints(g, x1shape, -2, 2) if x1shape else None
            xin = E.pad_concat(x, x1, off, xshape[2], xshape[3])
            return x, w, b, x1, (F.conv_transpose2d(xin, w, b, stride=2, padding=1) if transposed else F.conv2d(xin, w, b, stride=stride, padding=pad))
        x, w, b, x1, _ = _sparse(draw, 1 / 16)
    if not bias:
        b = None
    xin = E.pad_concat(x, x1, off, xshape[2], xshape[3])
    if transposed:
        E.check_exact(E.exactness_margin(xin, w, b, stride=2, pad=1, transposed=True))
        v = F.conv_transpose2d(xin, w, b, stride=2, padding=1)
    else:
        E.check_exact(E.exactness_margin(xin, w, b, stride=stride, pad=pad))
        v = F.conv2d(xin, w, b, stride=stride, padding=pad)
    E.check_rounding(v) if kind == "rounding" else E.check_stats(v)
    return Case(x=x, x1=x1, w=w, b=b, v=v)


def fold1x1_case(kind="rounding"):
    """1x1 with the one-class GroupNorm fold, bias and residual at (2, 192, 10, 14) -> 96 (the generic kernel's split-K form)."""
    B, Cin, Hh, Ww, cout = 2, 192, 10, 14, 96
    g = E.gen(_seed("f1", kind))
    a, mean, gamma, beta = E.gn_numbers(g, B, Cin)
    a, mean = a[:, 0], mean[:, 0]
    x, w, b = E.ints(g, (B, Cin, Hh, Ww), -32, 32), E.ints(g, (cout, Cin, 1, 1), -2, 2), E.ints(g, (cout,), -8, 8)
    r = E.ints(g, (B, cout, Hh, Ww), -16, 16)
    E.check_exact(E.conv_fold_margin(x, w, b, gamma, beta, a, mean, r, pad=0))
    v = E.conv_fold_ref(x, w, b, gamma, beta, a, mean, pad=0) + r
    E.check_rounding(v)
    return Case(x=x, w=w, b=b, gamma=gamma, beta=beta, ab=E.gn_ab_tensor(a, mean).view(B, 2), r=r, v=v)


PLAIN3_PAIRS = [("TILE_128x192", 192), ("TILE_256x96", 96), ("TILE_64x192", 384), ("TILE_128x32", 4)]
QUAD_CASES = [("up", 192, 96, (8, 32)), ("up", 192, 192, (9, 27)), ("up", 384, 96, (32, 8)), ("up", 192, 96, (5, 100)),
              ("down", 96, 96, (16, 64)), ("down", 96, 192, (18, 54)), ("down", 192, 96, (64, 16)), ("down", 96, 96, (10, 200))]
SMALLN_CASES = [((2, 96, 8, 64), 4), ((1, 64, 37, 16), 16), ((2, 128, 33, 8), 3), ((1, 96, 9, 27), 4), ((1, 32, 5, 100), 8)]
C7_CASES = [((9, 5), 3, 4), ((37, 70), 4, 8), ((16, 32), 4, 8)]


def quad_case(mode, cin, cout, hw, kind):
    tr = mode == "up"
    return plain_case("quad" + mode, (2, cin, *hw), (cin, cout, 4, 4) if tr else (cout, cin, 4, 4), kind, stride=2, pad=1, transposed=tr)


def c7_case(hw, cin, cx, kind="rounding"):
    """7x7 pad 3 over <= 4 real channels; the stored channels beyond them hold non-zero integers that must be ignored."""
    c = plain_case("c7", (3, cin, *hw), (96, cin, 7, 7), kind, pad=3)
    g = E.gen(_seed("c7pad", hw))
    c["xp"] = torch.cat([c.x, E.ints(g, (3, cx - cin, *hw), 1, 9)], 1)
    return c


def dw_case(hw, B, kind, tag="dw"):
    """Depthwise 7x7 over pad_and_concat(enc 96, dec 192 one row / three columns smaller), bias, integer time bias per sample."""
    Hh, Ww = hw
    g = E.gen(_seed(tag, hw, B, kind))
    if kind == "rounding":
        enc, dec = E.ints(g, (B, 96, Hh, Ww), -64, 64), E.ints(g, (B, 192, Hh - 1, Ww - 3), -64, 64)
        w, b, tb = E.ints(g, (288, 1, 7, 7), -2, 2), E.ints(g, (288,), -8, 8), E.ints(g, (B, 300), -16, 16)
    else:
        def draw(d):
            enc, dec = E.ints(g, (B, 96, Hh, Ww), -2, 2), E.ints(g, (B, 192, Hh - 1, Ww - 3), -2, 2)
            w, b, tb = E.ints(g, (288, 1, 7, 7), -1, 1, density=d), E.ints(g, (288,), -1, 1), E.ints(g, (B, 300), -2, 2)
            return enc, dec, w, b, tb, F.conv2d(E.pad_concat(enc, dec, (0, 1), Hh, Ww), w, b, padding=3, groups=288) + tb[:, 5:293, None, None]
        enc, dec, w, b, tb, _ = _sparse(draw, 1 / 4)
    cat = E.pad_concat(enc, dec, (0, 1), Hh, Ww)
    E.check_exact(E.exactness_margin(cat, w, b, tb, pad=3, groups=288))
    v = F.conv2d(cat, w, b, padding=3, groups=288) + tb[:, 5:293, None, None]
    E.check_rounding(v) if kind == "rounding" else E.check_stats(v)
    return Case(enc=enc, dec=dec, w=w, b=b, tb=tb, v=v)


DW_MFMA_HW = [(10, 9), (37, 70), (40, 16), (33, 13)]
C80_HW = [(4, 32), (19, 45)]


def c80_case(hw, kind, gn, act, add_x):
    """80-channel 3x3: out = [x +] conv3x3(act(GroupNorm(16, 80)(x))) + bias; the normalised x must be exact in bf16 (asserted)."""
    B, (Hh, Ww), G = 3, hw, 16
    g = E.gen(_seed("c80", hw, kind, gn, act, add_x))
    a, mean, gamma, beta = E.gn_numbers(g, B, 80, G)
    if kind == "rounding":
        xr = 4 if gn else 16                   # (normalised on load, +-4 becomes up to +-26 in quarters: the widest that stays exact in bf16)
        x, w, b = E.ints(g, (B, 80, Hh, Ww), -xr, xr), E.ints(g, (80, 80, 3, 3), -2, 2), E.ints(g, (80,), -8, 8)
    else:
        def draw(d):
            x, w, b = E.ints(g, (B, 80, Hh, Ww), -2, 2), E.ints(g, (80, 80, 3, 3), -1, 1, density=d), E.ints(g, (80,), -2, 2)
            xn = E.gn_on_load(x, a, mean, gamma, beta, act, G) if gn else x
            return x, w, b, F.conv2d(xn, w, b, padding=1) + (x if add_x else 0)
        x, w, b, _ = _sparse(draw, 1 / 16)
    xn = E.gn_on_load(x, a, mean, gamma, beta, act, G) if gn else x
    assert E.is_bf16(xn)
    E.check_exact(E.exactness_margin(xn, w, b, x, pad=1, unit=0.25))
    v = F.conv2d(xn, w, b, padding=1) + (x if add_x else 0)
    E.check_rounding(v) if kind == "rounding" else E.check_stats(v)
    return Case(x=x, w=w, b=b, gamma=gamma, beta=beta, ab=E.gn_ab_tensor(a, mean), xn=xn, v=v)


def convt80_case(hw, cin, kind, gn):
    """ConvTranspose2d(cin, 80, 4, 2, 1) reading relu(GroupNorm(16, cin)(x)) or x."""
    B, (Hh, Ww), G = 3, hw, 16
    g = E.gen(_seed("t80", hw, cin, kind, gn))
    a, mean, gamma, beta = E.gn_numbers(g, B, cin, G)
    if kind == "rounding":
        x, w, b = E.ints(g, (B, cin, Hh, Ww), -8, 8), E.ints(g, (cin, 80, 4, 4), -2, 2), E.ints(g, (80,), -8, 8)
    else:
        def draw(d):
            x, w, b = E.ints(g, (B, cin, Hh, Ww), -2, 2), E.ints(g, (cin, 80, 4, 4), -1, 1, density=d), E.ints(g, (80,), -2, 2)
            xn = E.gn_on_load(x, a, mean, gamma, beta, "relu", G) if gn else x
            return x, w, b, F.conv_transpose2d(xn, w, b, stride=2, padding=1)
        x, w, b, _ = _sparse(draw, 1 / 16)
    xn = E.gn_on_load(x, a, mean, gamma, beta, "relu", G) if gn else x
    assert E.is_bf16(xn)
    E.check_exact(E.exactness_margin(xn, w, b, stride=2, pad=1, transposed=True, unit=0.25))
    v = F.conv_transpose2d(xn, w, b, stride=2, padding=1)
    E.check_rounding(v) if kind == "rounding" else E.check_stats(v)
    return Case(x=x, w=w, b=b, gamma=gamma, beta=beta, ab=E.gn_ab_tensor(a, mean), v=v)


IN_NCHW_CASES = [(4, 160, (9, 7), 3), (8, 80, (4, 32), 2), (4, 8, (1, 5), 1)]


def in_nchw_case(cin, cout, hw, B):
    """fp32 NCHW latent -> 1x1 -> bf16 NHWC: fp32 operands, so any integers below 2^24 are exact."""
    g = E.gen(_seed("in", cin, cout, hw))
    x, w, b = E.ints(g, (B, cin, *hw), -64, 64), E.ints(g, (cout, cin, 1, 1), -16, 16), E.ints(g, (cout,), -8, 8)
    E.check_exact(E.exactness_margin(x, w, b))
    v0, v1 = F.conv2d(x, w, None), F.conv2d(x, w, b)
    E.check_rounding(v0)
    E.check_rounding(v1)
    return Case(x=x, w=w, b=b, v0=v0, v1=v1)


def gelu_inputs(n_slots, seed):
    """Every bf16 value of magnitude 2^-14 .. 16, both signs, plus +-0, in shuffled positions of n_slots slots (the rest repeats them)."""
    vals = E.all_bf16_values(2.0 ** -14, 16.0)
    assert n_slots >= vals.numel()
    g = E.gen(seed)
    fill = vals[torch.randint(0, vals.numel(), (n_slots - vals.numel(),), generator=g)]
    allv = torch.cat([vals, fill])
    return allv[torch.randperm(n_slots, generator=g)]


def gelu_fast_bound(x):
    """E of gelu_fast (csrc/common.hpp), per element, for the input x (float64): see test_gelu_per_implementation."""
    t_tail = 0.5 * x.abs() * torch.special.erfc(x.abs() * math.sqrt(0.5))
    return 0.5 * x.abs() * 1.5e-7 + t_tail * (16.0 + x * x) * 2.0 ** -24 + E.gelu64(x).abs() * 2.0 ** -24


def all_cpu_cases():
    """Every case of this file, built on the CPU (preconditions asserted inside the builders): tests/test_exact_ref_cpu.py runs this."""
    n = 0
    for shape in HALO_SHAPES:
        for cout in HALO_COUTS:
            halo_case(shape, cout, "rounding")
            n += 1
        halo_case(shape, 64, "stats")
        n += 1
    for cout, ks in HALO_SPLITK:
        halo_case((2, 384, 20, 8), cout, "rounding")
        n += 1
    halo_case((2, 384, 20, 8), 64, "stats")
    for shape, cx in RES_CONV_CASES:
        res_conv_case(shape, cx, "rounding")
        res_conv_case(shape, cx, "stats")
        n += 2
    for _, cout in PLAIN3_PAIRS:
        plain_case("p3", (2, 64, 12, 20), (cout, 64, 3, 3), "rounding", pad=1)
        n += 1
    plain_case("p3", (2, 64, 12, 20), (96, 64, 3, 3), "stats", pad=1)
    plain_case("cc", (2, 96, 9, 7), (96, 288, 1, 1), "rounding", x1shape=(2, 192, 8, 4), off=(0, 1))
    for hw in ((16, 10), (9, 7)):
        plain_case("du", (2, 96, *hw), (96, 96, 4, 4), "rounding", stride=2, pad=1)
        plain_case("du", (2, 96, *hw), (96, 96, 4, 4), "rounding", transposed=True)
    plain_case("i7", (2, 4, 16, 12), (96, 4, 7, 7), "rounding", pad=3)
    plain_case("gs", (2, 192, 10, 14), (192, 192, 4, 4), "rounding", stride=2, pad=1)
    plain_case("gs", (2, 192, 10, 14), (192, 192, 4, 4), "stats", stride=2, pad=1)
    plain_case("gs", (2, 192, 10, 14), (192, 192, 4, 4), "rounding", transposed=True)
    fold1x1_case()
    n += 10
    for q in QUAD_CASES:
        quad_case(*q, "rounding")
        quad_case(*q, "stats")
        n += 2
    for shape, cout in SMALLN_CASES:
        plain_case("sn", shape, (cout, shape[1], 3, 3), "rounding", pad=1)
        n += 1
    for hw, cin, cx in C7_CASES:
        c7_case(hw, cin, cx)
        n += 1
    dw_case((10, 9), 2, "rounding")
    dw_case((10, 9), 2, "stats")
    dw_case((10, 9), 6, "stats", tag="dwchunk")
    for hw in DW_MFMA_HW:
        dw_case(hw, 2, "rounding")
        dw_case(hw, 2, "stats")
        n += 2
    n += 3
    for hw in C80_HW:
        for gn, act, add_x in C80_CONFIGS:
            c80_case(hw, "rounding", gn, act, add_x)
            c80_case(hw, "stats", gn, act, add_x)
            n += 2
        for cin in (80, 160):
            for gn in (False, True):
                convt80_case(hw, cin, "rounding", gn)
                convt80_case(hw, cin, "stats", gn)
                n += 2
    for c in IN_NCHW_CASES:
        in_nchw_case(*c)
        n += 1
    return n


C80_CONFIGS = [(False, None, 0), (True, None, 0), (True, None, 1), (True, "relu", 0), (True, "relu", 1)]


# ===================================================================================================== device plumbing
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    L.load()


def dev(x, dt=BF, c_pad=None):
    """Exact NCHW float64 (cpu) -> NHWC device tensor of the kernel type; the conversion must not round."""
    assert E.is_bf16(x) if dt == BF else E.is_f32(x)
    return H().to_nhwc(x, dt, c_pad)


def f32dev(t):
    assert E.is_f32(t)
    return t.float().contiguous().cuda()


def nchw(y):
    return H().from_nhwc(y)


def want_of(v, dt=BF):
    return E.store(v, dt == BF).float()


def stat_sums(st):
    return st.double().sum(1).cpu()


def conv_params(xd, wpk, cout, cout_pad, out, **kw):
    B, Hh, Ww, C0 = xd.shape
    f = dict(src0=xd.data_ptr(), src1=None, C0=C0, C1=0, H=Hh, W=Ww, H1=0, W1=0, off_h1=0, off_w1=0, wpk=wpk.data_ptr(), Cout=cout,
             cout_pad=cout_pad, KH=3, KW=3, stride=1, pad_h=1, pad_w=1, Ho=Hh, Wo=Ww, transposed=0, out=out.data_ptr(), out_C=out.shape[3],
             out_c0=0, out_nchw_f32=0, bias=None, gn_ab=None, fold_t1=None, fold_t2=None, ncls=1, act=L.ACT_NONE, res=None, stats_part=None,
             B=B, dtype=BF, tile=L.TILE_HALO3_256x96, wk_order=1)
    f.update(kw)
    return L.ConvParams(**f)


def launch_conv(p, B, splitk=False):
    """ds_conv_igemm (+ ds_conv_splitk_reduce) with zeroed statistics partials; returns the partials."""
    st = torch.zeros(B, L.load().ds_conv_stats_parts(C.byref(p)), 2, device="cuda")
    p.stats_part = st.data_ptr()
    L.call("ds_conv_igemm", C.byref(p), L.current_stream())
    if splitk:
        L.call("ds_conv_splitk_reduce", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    return st


# ===================================================================================================== DS_CONV_TILE_HALO3_256x96
@pytest.mark.parametrize("cout", HALO_COUTS)
@pytest.mark.parametrize("shape", HALO_SHAPES)
def test_halo3_fold_bias_residual(shape, cout):
    """32- / 16- / 8-wide tiles, several column tiles, ragged H and W, Cout below an N-block; nine-class fold, ACT_NONE, without a residual
    (register / bf16-staged epilogue) and with one (line-sized fp32-staged epilogue: 'the same fp32 sum, rounded once')."""
    h = H()
    c = halo_case(shape, cout, "rounding")
    pc = h.PackedConv(c.w, c.b, BF, L.TILE_HALO3_256x96, gamma=c.gamma, beta=c.beta)
    xd, rd, ab = dev(c.x), dev(c.r), c.ab.cuda()
    y, _ = h.run_conv(pc, xd, pad=1, gn_ab=ab)
    E.assert_bits_equal(nchw(y), want_of(c.v), "halo3 %s -> %d, no residual" % (shape, cout))
    y, _ = h.run_conv(pc, xd, pad=1, gn_ab=ab, res=rd)
    E.assert_bits_equal(nchw(y), want_of(c.v + c.r), "halo3 %s -> %d, residual" % (shape, cout))


@pytest.mark.parametrize("shape", HALO_SHAPES)
def test_halo3_statistics(shape):
    h = H()
    c = halo_case(shape, 64, "stats")
    pc = h.PackedConv(c.w, c.b, BF, L.TILE_HALO3_256x96, gamma=c.gamma, beta=c.beta)
    y, st = h.run_conv(pc, dev(c.x), pad=1, gn_ab=c.ab.cuda(), want_stats=True)
    E.assert_bits_equal(nchw(y), want_of(c.v), "halo3 statistics case %s" % (shape,))
    E.assert_stats_exact(stat_sums(st), c.v, "halo3 %s" % (shape,))


@pytest.mark.parametrize("cout,ks", HALO_SPLITK)
def test_halo3_split_k(cout, ks):
    """K slices -> fp32 slab -> ds_conv_splitk_reduce (fold, residual, bf16 store): integer partial sums are exact in any split."""
    h = H()
    shape = (2, 384, 20, 8)
    c = halo_case(shape, cout, "rounding")
    pc = h.PackedConv(c.w, c.b, BF, L.TILE_HALO3_256x96, gamma=c.gamma, beta=c.beta)
    y, _ = h.run_conv(pc, dev(c.x), pad=1, gn_ab=c.ab.cuda(), res=dev(c.r), ksplit=ks)
    E.assert_bits_equal(nchw(y), want_of(c.v + c.r), "halo3 split-K %d -> %d" % (ks, cout))
    if cout == 64:
        s = halo_case(shape, 64, "stats")
        ps = h.PackedConv(s.w, s.b, BF, L.TILE_HALO3_256x96, gamma=s.gamma, beta=s.beta)
        y, st = h.run_conv(ps, dev(s.x), pad=1, gn_ab=s.ab.cuda(), want_stats=True, ksplit=ks)
        E.assert_bits_equal(nchw(y), want_of(s.v), "halo3 split-K statistics case")
        E.assert_stats_exact(stat_sums(st), s.v, "halo3 split-K %d" % ks)


@pytest.mark.parametrize("shape,cx", RES_CONV_CASES)
def test_halo3_fused_res_conv(shape, cx):
    h = H()
    lib = L.load()
    for kind in ("rounding", "stats"):
        c = res_conv_case(shape, cx, kind)
        B, Cin, Hh, Ww = shape
        pc = h.PackedConv(c.w, c.b, BF, L.TILE_HALO3_256x96, gamma=c.gamma, beta=c.beta)
        rpk = torch.empty(lib.ds_pack_conv_elems(c.c0 + c.c1, 1, 1, pc.cout_pad, 0), dtype=torch.bfloat16, device="cuda")
        wrd = f32dev(c.wr)
        pp = L.PackConvParams(w=wrd.data_ptr(), gamma=None, dst=rpk.data_ptr(), dtype=BF, Cout=c.cout, Cin=c.c0 + c.c1, cin_pad=c.c0 + c.c1, KH=1, KW=1,
                              cout_pad=pc.cout_pad, transposed=0, k_order=1)
        L.call("ds_pack_conv_weight", C.byref(pp), L.current_stream())
        wall = torch.cat([rpk, pc.w])
        gd, x0d, x1d = dev(c.gin), dev(c.x0), (dev(c.x1) if c.c1 else None)
        brd, ab = f32dev(c.br), c.ab.cuda()
        out = torch.full((B, Hh, Ww, c.cout), NAN, device="cuda").bfloat16()
        p = conv_params(gd, wall, c.cout, pc.cout_pad, out, bias=pc.bias.data_ptr(), gn_ab=ab.data_ptr(), fold_t1=pc.t1.data_ptr(),
                        fold_t2=pc.t2.data_ptr(), ncls=9, res_src0=x0d.data_ptr(), res_src1=L.ptr(x1d), res_C0=c.c0, res_C1=c.c1,
                        res_H1=c.h1 if c.c1 else 0, res_W1=c.w1 if c.c1 else 0, res_off_h1=c.off[0] if c.c1 else 0,
                        res_off_w1=c.off[1] if c.c1 else 0, res_steps=(c.c0 + c.c1) // 32, res_bias=brd.data_ptr())
        st = launch_conv(p, B)
        E.assert_bits_equal(nchw(out), want_of(c.v), "fused res_conv %s %s (%s)" % (shape, cx, kind))
        if kind == "stats":
            E.assert_stats_exact(stat_sums(st), c.v, "fused res_conv %s" % (shape,))


# ===================================================================================================== generic tiles
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("tile,cout", PLAIN3_PAIRS)
def test_generic_conv3x3(dt, tile, cout):
    """fp32 MFMA on integers is exact too: the fp32 kernels must return the integers themselves."""
    h = H()
    c = plain_case("p3", (2, 64, 12, 20), (cout, 64, 3, 3), "rounding", pad=1)
    pc = h.PackedConv(c.w, c.b, dt, getattr(L, tile))
    y, _ = h.run_conv(pc, dev(c.x, dt), pad=1)
    E.assert_bits_equal(nchw(y), want_of(c.v, dt), "generic 3x3 %s -> %d" % (tile, cout))
    if cout == 96:
        s = plain_case("p3", (2, 64, 12, 20), (96, 64, 3, 3), "stats", pad=1)
        ps = h.PackedConv(s.w, s.b, dt, getattr(L, tile))
        y, st = h.run_conv(ps, dev(s.x, dt), pad=1, want_stats=True)
        E.assert_bits_equal(nchw(y), want_of(s.v, dt), "generic 3x3 statistics case")
        E.assert_stats_exact(stat_sums(st), s.v, "generic 3x3")


@pytest.mark.parametrize("dt", [BF, F32])
def test_generic_conv1x1_two_source_concat(dt):
    h = H()
    c = plain_case("cc", (2, 96, 9, 7), (96, 288, 1, 1), "rounding", x1shape=(2, 192, 8, 4), off=(0, 1))
    pc = h.PackedConv(c.w, c.b, dt, L.TILE_256x96)
    y, _ = h.run_conv(pc, dev(c.x, dt), dev(c.x1, dt), off1=(0, 1))
    E.assert_bits_equal(nchw(y), want_of(c.v, dt), "two-source 1x1")


@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("hw", [(16, 10), (9, 7)])
def test_generic_down_and_upsample(dt, hw):
    h = H()
    c = plain_case("du", (2, 96, *hw), (96, 96, 4, 4), "rounding", stride=2, pad=1)
    y, _ = h.run_conv(h.PackedConv(c.w, c.b, dt, L.TILE_256x96), dev(c.x, dt), stride=2, pad=1)
    E.assert_bits_equal(nchw(y), want_of(c.v, dt), "conv 4x4 stride 2 %s" % (hw,))
    c = plain_case("du", (2, 96, *hw), (96, 96, 4, 4), "rounding", transposed=True)
    y, _ = h.run_conv(h.PackedConv(c.w, c.b, dt, L.TILE_256x96, transposed=True), dev(c.x, dt))
    E.assert_bits_equal(nchw(y), want_of(c.v, dt), "transposed 4x4 %s" % (hw,))


@pytest.mark.parametrize("dt", [BF, F32])
def test_generic_init_conv7x7(dt):
    h = H()
    c = plain_case("i7", (2, 4, 16, 12), (96, 4, 7, 7), "rounding", pad=3)
    cp = 8 if dt == BF else 4
    y, _ = h.run_conv(h.PackedConv(c.w, c.b, dt, L.TILE_256x96, cin_pad=cp), dev(c.x, dt, cp), pad=3)
    E.assert_bits_equal(nchw(y), want_of(c.v, dt), "7x7 init convolution")


@pytest.mark.parametrize("ks", [2, 3, 4])
def test_generic_split_k(ks):
    h = H()
    xs, ws = (2, 192, 10, 14), (192, 192, 4, 4)
    c = plain_case("gs", xs, ws, "rounding", stride=2, pad=1)
    y, _ = h.run_conv(h.PackedConv(c.w, c.b, BF, L.TILE_64x192), dev(c.x), stride=2, pad=1, ksplit=ks)
    E.assert_bits_equal(nchw(y), want_of(c.v), "generic split-K %d, 4x4 stride 2" % ks)
    s = plain_case("gs", xs, ws, "stats", stride=2, pad=1)
    y, st = h.run_conv(h.PackedConv(s.w, s.b, BF, L.TILE_64x192), dev(s.x), stride=2, pad=1, want_stats=True, ksplit=ks)
    E.assert_bits_equal(nchw(y), want_of(s.v), "generic split-K %d statistics case" % ks)
    E.assert_stats_exact(stat_sums(st), s.v, "generic split-K %d" % ks)
    c = plain_case("gs", xs, ws, "rounding", transposed=True)
    y, _ = h.run_conv(h.PackedConv(c.w, c.b, BF, L.TILE_128x192, transposed=True), dev(c.x), ksplit=ks)
    E.assert_bits_equal(nchw(y), want_of(c.v), "generic split-K %d, transposed" % ks)
    if ks == 2:
        c = fold1x1_case()
        pc = h.PackedConv(c.w, c.b, BF, L.TILE_256x96, gamma=c.gamma, beta=c.beta)
        y, _ = h.run_conv(pc, dev(c.x), gn_ab=c.ab.cuda(), res=dev(c.r), ksplit=2)
        E.assert_bits_equal(nchw(y), want_of(c.v), "generic split-K 2, folded 1x1 + residual")


# ===================================================================================================== DS_CONV_TILE_QUAD_HALO3
@pytest.mark.parametrize("mode,cin,cout,hw", QUAD_CASES)
def test_quad_halo3(mode, cin, cout, hw):
    """All four phases / parity planes, every tile width, ragged grids; whole-K and every split-K factor the shape admits."""
    from diffusynth_amd.engine import pack_quad_weights
    tr = mode == "up"
    B, (Hh, Ww) = 2, hw
    oh, ow = (2 * Hh, 2 * Ww) if tr else (Hh // 2, Ww // 2)
    gh, gw = (Hh, Ww) if tr else (oh, ow)
    nch = (1 if tr else 4) * cin // 32
    for kind in ("rounding", "stats"):
        c = quad_case(mode, cin, cout, hw, kind)
        assert E.is_bf16(c.w)
        wpk, cout_pad = pack_quad_weights(c.w.float().cuda(), tr)
        xd, bd = dev(c.x), f32dev(c.b)
        for ks in (1, 2, 3, 4, 6, 8):
            if ks > 1 and (nch % ks or (nch // ks) % 6):
                continue
            out = torch.full((B, oh, ow, cout), NAN, device="cuda").bfloat16()
            p = conv_params(xd, wpk, cout, cout_pad, out, KH=2 if tr else 4, KW=2 if tr else 4, stride=1 if tr else 2, pad_h=0 if tr else 1,
                            pad_w=0 if tr else 1, Ho=gh, Wo=gw, transposed=int(tr), bias=bd.data_ptr(), tile=L.TILE_QUAD_HALO3, wk_order=2)
            slab = None
            if ks > 1:
                slab = torch.full((ks, B, oh, ow, (cout + 7) // 8 * 8), NAN, device="cuda")
                p.ksplit, p.slab = ks, slab.data_ptr()
            st = launch_conv(p, B, splitk=ks > 1)
            what = "quad %s %d -> %d %s, ksplit %d (%s)" % (mode, cin, cout, hw, ks, kind)
            E.assert_bits_equal(nchw(out), want_of(c.v), what)
            if kind == "stats":
                E.assert_stats_exact(stat_sums(st), c.v, what)


# ===================================================================================================== DS_CONV_TILE_HALO3_N16
@pytest.mark.parametrize("shape,cout", SMALLN_CASES)
def test_smalln(shape, cout):
    B, Cin, Hh, Ww = shape
    c = plain_case("sn", shape, (cout, Cin, 3, 3), "rounding", pad=1)
    wpk = torch.empty(L.load().ds_pack_conv_elems(Cin, 3, 3, 16, 0), dtype=torch.bfloat16, device="cuda")
    wd, bd = f32dev(c.w), f32dev(c.b)
    pp = L.PackConvParams(w=wd.data_ptr(), gamma=None, dst=wpk.data_ptr(), dtype=BF, Cout=cout, Cin=Cin, cin_pad=Cin, KH=3, KW=3, cout_pad=16,
                          transposed=0, k_order=1)
    L.call("ds_pack_conv_weight", C.byref(pp), L.current_stream())
    out = torch.full((B, Hh, Ww, (cout + 7) // 8 * 8), NAN, device="cuda").bfloat16()
    p = conv_params(dev(c.x), wpk, cout, 16, out, bias=bd.data_ptr(), tile=L.TILE_HALO3_N16)
    L.call("ds_conv_igemm", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    got = nchw(out)
    E.assert_bits_equal(got[:, :cout], want_of(c.v), "N16 %s -> %d" % (shape, cout))
    assert (got[:, cout:] == 0).all(), "pad channels must be exact zeros"


# ===================================================================================================== ds_conv7x7_c4
@pytest.mark.parametrize("hw,cin,cx", C7_CASES)
def test_conv7x7_c4(hw, cin, cx):
    c = c7_case(hw, cin, cx)
    B, (Hh, Ww) = 3, hw
    xd, wd, bd = dev(c.xp), f32dev(c.w), f32dev(c.b)
    wp = torch.empty(L.load().ds_conv7x7_c4_weight_elems(), dtype=torch.bfloat16, device="cuda")
    st = L.current_stream()
    L.call("ds_pack_conv7x7_c4", wd.data_ptr(), 96, cin, wp.data_ptr(), st)
    out = torch.full((B, Hh, Ww, 96), NAN, device="cuda").bfloat16()
    L.call("ds_conv7x7_c4", xd.data_ptr(), B, Hh, Ww, cx, wp.data_ptr(), bd.data_ptr(), out.data_ptr(), st)
    torch.cuda.synchronize()
    E.assert_bits_equal(nchw(out), want_of(c.v), "conv7x7_c4 %s cin %d" % (hw, cin))


# ===================================================================================================== ds_dwconv7 (bf16)
def _run_dw(c, hw, B, wexp, batch_hint=0):
    Hh, Ww = hw
    x0, x1 = dev(c.enc), dev(c.dec)
    wd = f32dev(c.w)
    assert E.is_bf16(c.w)
    wt = torch.empty(49 * 288, device="cuda")
    L.call("ds_pack_dw_weight", wd.data_ptr(), 288, wt.data_ptr(), L.current_stream())
    we = None
    if wexp:
        we = torch.empty(288 * 6 * 64 * 8, dtype=torch.bfloat16, device="cuda")
        L.call("ds_pack_dw_weight_mfma", wd.data_ptr(), 288, we.data_ptr(), L.current_stream())
    bd, tbd = f32dev(c.b), f32dev(c.tb)
    out = torch.full((B, Hh, Ww, 288), NAN, device="cuda").bfloat16()
    p = L.DwconvParams(src0=x0.data_ptr(), src1=x1.data_ptr(), C0=96, C1=192, H=Hh, W=Ww, H1=Hh - 1, W1=Ww - 3, off_h1=0, off_w1=1,
                       wt=wt.data_ptr(), bias=bd.data_ptr(), tbias=tbd.data_ptr() + 4 * 5, tb_stride=300, out=out.data_ptr(), stats_part=None,
                       B=B, dtype=BF, wexp=L.ptr(we), batch_hint=batch_hint)
    fam, rng, spc = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    L.call("ds_dwconv_launch_choice", C.byref(p), C.byref(fam), C.byref(rng), C.byref(spc))
    st = torch.zeros(B, L.load().ds_dwconv_stats_parts(C.byref(p)), 2, device="cuda")
    p.stats_part = st.data_ptr()
    L.call("ds_dwconv7", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    return nchw(out), stat_sums(st), L.DW_FAMILY[fam.value], spc.value


@pytest.mark.parametrize("hw,wexp", [((10, 9), False)] + [(hw, True) for hw in DW_MFMA_HW])
def test_dwconv7(hw, wexp):
    """Two sources with pad offsets, integer time bias per sample, statistics; without wexp (vector kernel) and with the Toeplitz weights."""
    for kind in ("rounding", "stats"):
        c = dw_case(hw, 2, kind)
        got, sums, fam, _ = _run_dw(c, hw, 2, wexp)
        assert (fam == "mfma") == wexp, fam
        E.assert_bits_equal(got, want_of(c.v), "dwconv7 %s %s (%s)" % (hw, fam, kind))
        if kind == "stats":
            E.assert_stats_exact(sums, c.v, "dwconv7 %s %s" % (hw, fam))


def test_dwconv7_chunk_of_whole_samples_with_a_short_last_chunk():
    """Matrix-core form, image of one tile, decision batch 256: a chunk holds four whole samples, so the six samples run as 4 + 2."""
    c = dw_case((10, 9), 6, "stats", tag="dwchunk")
    got, sums, fam, spc = _run_dw(c, (10, 9), 6, True, batch_hint=256)
    assert fam == "mfma" and spc > 1 and 6 % spc != 0, (fam, spc)
    E.assert_bits_equal(got, want_of(c.v), "dwconv7 chunks of %d samples" % spc)
    E.assert_stats_exact(sums, c.v, "dwconv7 chunks of %d samples" % spc)


# ===================================================================================================== VQGAN tail
def _chan_stats_exact(ws, v, what):
    """ws [B][slots][80][2] with every slot written; summed over the slots in float64 = per-channel integer sums of v [B][80][H][W]."""
    assert torch.isfinite(ws).all(), "%s: a statistics slot was not written" % what
    s = ws.double().sum(1).cpu()
    want = torch.stack([v.flatten(2).sum(2), (v * v).flatten(2).sum(2)], -1)
    assert torch.equal(s, want), "%s: per-channel statistics differ at %s" % (what, (s != want).nonzero()[:6].tolist())


@pytest.mark.parametrize("hw", C80_HW)
def test_conv3x3_c80(hw):
    lib = L.load()
    st = L.current_stream()
    B, (Hh, Ww), G = 3, hw, 16
    for gn, act, add_x in C80_CONFIGS:
        for kind in ("rounding", "stats"):
            c = c80_case(hw, kind, gn, act, add_x)
            xd, wd, bd, gd, bed, ab = dev(c.x), f32dev(c.w), f32dev(c.b), f32dev(c.gamma), f32dev(c.beta), c.ab.cuda()
            wp = torch.empty(lib.ds_conv3x3_c80_weight_elems(), dtype=torch.bfloat16, device="cuda")
            L.call("ds_pack_conv3x3_c80", wd.data_ptr(), 80, 80, wp.data_ptr(), st)
            out = torch.full((B, Hh, Ww, 80), NAN, device="cuda").bfloat16()
            ws = torch.full((B, lib.ds_conv3x3_c80_stats_slots(B, Hh, Ww), 80, 2), NAN, device="cuda")
            L.call("ds_conv3x3_c80", xd.data_ptr(), B, Hh, Ww, wp.data_ptr(), bd.data_ptr(), out.data_ptr(), ab.data_ptr() if gn else None, G if gn else 0,
                   gd.data_ptr() if gn else None, bed.data_ptr() if gn else None, L.ACT_RELU if act == "relu" else L.ACT_NONE, add_x, ws.data_ptr(), st)
            torch.cuda.synchronize()
            what = "conv3x3_c80 %s gn %s act %s add_x %d (%s)" % (hw, gn, act, add_x, kind)
            E.assert_bits_equal(nchw(out), want_of(c.v), what)
            if kind == "stats":
                _chan_stats_exact(ws, c.v, what)
            if gn and add_x:
                # ds_conv3x3_c80_res: the same block as two launches, h = act(GroupNorm(x)) handed over as a bf16 tensor (exact here)
                out2 = torch.full((B, Hh, Ww, 80), NAN, device="cuda").bfloat16()
                ws2 = torch.full_like(ws, NAN)
                L.call("ds_conv3x3_c80_res", dev(c.xn).data_ptr(), xd.data_ptr(), B, Hh, Ww, wp.data_ptr(), bd.data_ptr(), out2.data_ptr(), ws2.data_ptr(), st)
                torch.cuda.synchronize()
                E.assert_bits_equal(nchw(out2), want_of(c.v), what + ", _res form")
                if kind == "stats":
                    _chan_stats_exact(ws2, c.v, what + ", _res form")


@pytest.mark.parametrize("cin", [80, 160])
@pytest.mark.parametrize("hw", C80_HW)
def test_convt4x4_c80(hw, cin):
    lib = L.load()
    st = L.current_stream()
    B, (Hh, Ww), G = 3, hw, 16
    for gn in (False, True):
        for kind in ("rounding", "stats"):
            c = convt80_case(hw, cin, kind, gn)
            xd, wd, bd, gd, bed, ab = dev(c.x), f32dev(c.w), f32dev(c.b), f32dev(c.gamma), f32dev(c.beta), c.ab.cuda()
            wp = torch.empty(lib.ds_convt4x4_c80_weight_elems(cin), dtype=torch.bfloat16, device="cuda")
            L.call("ds_pack_convt4x4_c80", wd.data_ptr(), cin, 80, wp.data_ptr(), st)
            out = torch.full((B, 2 * Hh, 2 * Ww, 80), NAN, device="cuda").bfloat16()
            ws = torch.full((B, lib.ds_convt4x4_c80_stats_slots(B, Hh, Ww, cin), 80, 2), NAN, device="cuda")
            L.call("ds_convt4x4_c80", xd.data_ptr(), B, Hh, Ww, cin, wp.data_ptr(), bd.data_ptr(), out.data_ptr(), ab.data_ptr() if gn else None,
                   G if gn else 0, gd.data_ptr() if gn else None, bed.data_ptr() if gn else None, ws.data_ptr(), st)
            torch.cuda.synchronize()
            what = "convt4x4_c80 %s cin %d gn %s (%s)" % (hw, cin, gn, kind)
            E.assert_bits_equal(nchw(out), want_of(c.v), what)
            if kind == "stats":
                _chan_stats_exact(ws, c.v, what)


@pytest.mark.parametrize("cin,cout,hw,B", IN_NCHW_CASES)
def test_conv1x1_in_nchw(cin, cout, hw, B):
    c = in_nchw_case(cin, cout, hw, B)
    xd, wd, bd = f32dev(c.x), f32dev(c.w.view(cout, cin)), f32dev(c.b)
    for bias, v in ((None, c.v0), (bd, c.v1)):
        out = torch.full((B, *hw, cout), NAN, device="cuda").bfloat16()
        L.call("ds_conv1x1_in_nchw", xd.data_ptr(), B, cin, hw[0] * hw[1], wd.data_ptr(), L.ptr(bias), cout, out.data_ptr(), L.current_stream())
        torch.cuda.synchronize()
        E.assert_bits_equal(nchw(out), want_of(v), "conv1x1_in_nchw %d -> %d %s bias %s" % (cin, cout, hw, bias is not None))


# ===================================================================================================== GELU, per implementation
def _identity3x3(cin, cout):
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    for o in range(cout):
        w[o, o, 1, 1] = 1.0
    return w


GELU_ROUTES = [  # (name, implementation, input shape, Cout, tile, dtype, ksplit)
    ("halo3 16-wide tile", "tab", (1, 96, 8, 16), 96, "TILE_HALO3_256x96", BF, 1),
    ("halo3 8-wide tile", "poly", (1, 96, 16, 8), 96, "TILE_HALO3_256x96", BF, 1),
    ("generic tile bf16", "fast", (1, 96, 8, 16), 96, "TILE_256x96", BF, 1),
    ("generic tile fp32", "fast", (1, 96, 8, 16), 96, "TILE_256x96", F32, 1),
    ("splitk_reduce", "fast", (1, 96, 8, 16), 96, "TILE_HALO3_256x96", BF, 3),
    ("N16 tile", "fast", (1, 32, 16, 32), 16, "TILE_HALO3_N16", BF, 1),
]


@pytest.mark.parametrize("route", GELU_ROUTES, ids=[r[0].replace(" ", "_") for r in GELU_ROUTES])
def test_gelu_per_implementation(route):
    """GELU behind a 3x3 convolution whose weight is the identity at the centre tap (no bias, fold or residual): the accumulator is x
    exactly, and x runs over every bf16 value of magnitude 2^-14 .. 16, both signs, plus +-0 (18 binades x 128 x 2 + 4 = 4612 values).
    Per element |got - gelu64(x)| <= E + 2^-8 (|gelu64(x)| + E): E the implementation's documented bound, the second term the half-ulp
    of the bf16 store (absent for the fp32 output).

    Which implementation runs where (read from the sources): gelu_tab8 in conv3x3_halo3's 32- / 16-wide tiles (HG<TWL>::LUT), gelu_poly8
    in its 8-wide tile, gelu_fast in the generic tiles (conv_epilogue.hpp), in ds_conv_splitk_reduce (conv_splitk.hip) and in the N16
    tile (conv3x3_smalln.hip).  E: table 6.63e-4 and polynomial 2.0e-5 (conv_halo3_common.hpp; tests/test_exact_ref_cpu.py recomputes
    both), gelu_fast from its comment (common.hpp): gelu = relu(v) - 0.5 |v| q with q = erfc(|v| / sqrt 2) from Abramowitz & Stegun
    7.1.26, |error of q| <= 1.5e-7, so 0.5 |v| 1.5e-7; plus the fp32 chain that forms q = poly(t) t e: v_rcp_f32 (1 ulp) and v_exp_f32
    (1 ulp), five fma and two products (half an ulp each, the alternating-sign Horner sum amplifying them a few times): 16 ulp of q
    allowed, and e = exp2(-v^2 c) inherits the two roundings of its argument, a relative ln 2 x (v^2 log2(e) / 2) x 2^-23 = v^2 2^-24;
    both relative to 0.5 |v| q = T(|v|); plus the half-ulp of the final fma, 2^-24 |gelu|:
        E_fast(v) = 0.5 |v| 1.5e-7 + T(|v|) (16 + v^2) 2^-24 + |gelu64(v)| 2^-24."""
    h = H()
    name, impl, shape, cout, tile, dt, ks = route
    B, Cin, Hh, Ww = shape
    xs = gelu_inputs(cout * Hh * Ww, _seed("gelu", name)).view(1, cout, Hh, Ww).double()
    x = torch.zeros(shape, dtype=torch.float64)
    x[:, :cout] = xs
    w = _identity3x3(Cin, cout)
    assert E.is_bf16(x) and (F.conv2d(x, w, padding=1)[:, :cout] == xs).all()   # one non-zero product per output: the accumulator is x
    if tile == "TILE_HALO3_N16":
        wpk = torch.empty(L.load().ds_pack_conv_elems(Cin, 3, 3, 16, 0), dtype=torch.bfloat16, device="cuda")
        wd = f32dev(w)
        pp = L.PackConvParams(w=wd.data_ptr(), gamma=None, dst=wpk.data_ptr(), dtype=BF, Cout=cout, Cin=Cin, cin_pad=Cin, KH=3, KW=3, cout_pad=16,
                              transposed=0, k_order=1)
        L.call("ds_pack_conv_weight", C.byref(pp), L.current_stream())
        out = torch.full((B, Hh, Ww, cout), NAN, device="cuda").bfloat16()
        p = conv_params(dev(x), wpk, cout, 16, out, act=L.ACT_GELU, tile=L.TILE_HALO3_N16)
        L.call("ds_conv_igemm", C.byref(p), L.current_stream())
        torch.cuda.synchronize()
        y = out
    else:
        pc = h.PackedConv(w, None, dt, getattr(L, tile))
        y, _ = h.run_conv(pc, dev(x, dt), pad=1, act=L.ACT_GELU, ksplit=ks)
    got = nchw(y).double()
    ref = E.gelu64(xs)
    bound = {"tab": torch.full_like(ref, E.E_GELU_TAB), "poly": torch.full_like(ref, E.E_GELU_POLY), "fast": gelu_fast_bound(xs)}[impl]
    err = (got - ref).abs()
    half_ulp = 2.0 ** -8 * ref.abs() if dt == BF else torch.zeros_like(ref)
    own = (err - half_ulp).clamp_min(0.0)                   # what the store's rounding cannot explain: a lower bound of the implementation's error
    k = (own / bound.clamp_min(1e-30)).argmax()
    print("GELU %s (%s): max |got - gelu64(x)| beyond the store's half-ulp = %.3e at x = %r, where E = %.3e (%.0f %% of it); over all inputs max %.3e"
          % (name, impl, own.flatten()[k].item(), xs.flatten()[k].item(), bound.flatten()[k].item(),
             100 * (own / bound.clamp_min(1e-30)).flatten()[k].item(), own.max().item()))
    worst = (err - bound).argmax()
    tol = bound + (2.0 ** -8 * (ref.abs() + bound) if dt == BF else 0.0)
    assert torch.isfinite(got).all() and (err <= tol).all(), (name, xs.flatten()[worst].item(), err.flatten()[worst].item(), tol.flatten()[worst].item())
