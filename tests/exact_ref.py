"""Plain CPU helpers for the bit-exact tests (tests/test_hip_exact.py, tests/test_exact_ref_cpu.py; the split-precision tier:
tests/test_hip_exact_x3.py, tests/test_exact_ref_x3_cpu.py).

The idea: when x, w, bias, residual and the GroupNorm numbers are small integers (or integers times a power of two) and
sum |x| |w| stays below 2^24 units, every bf16 x bf16 product is exact in fp32 and every partial sum is exact IN ANY ORDER (MFMA
k-order, split-K slices, chunk order).  The stored value is then ONE round-to-nearest-even of a number this file computes in
float64, and the expected tensor is known bit for bit: torch.equal replaces a tolerance.

Everything here is float64 on the CPU, built from F.conv2d / F.conv_transpose2d, in the algebra include/diffusynth_hip.h documents:
bias, GroupNorm fold a * acc + (t1[cls] - a*mean * t2[cls]) over the nine border classes, activation before the residual, one
rounding at the store, pad channels exact zeros, fused res_conv a * (acc_res / a + acc_3x3), GroupNorm applied on load for the
80-channel kernels."""
import math

import torch
import torch.nn.functional as F

LIMIT = float(1 << 24)


# ------------------------------------------------------------------------------------------------- generators
def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo, hi, density=1.0, scale=1.0):
    """Seeded integers of [lo, hi] as float64, a share `density` of them kept (the others zero), times `scale` (a power of two)."""
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).double()
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < density)
    return t * scale


def choice(g, shape, values):
    """Seeded draws from `values` as float64."""
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


def gn_numbers(g, B, C, groups=1):
    """GroupNorm numbers that keep the fold exact: a in {0.5, 1, 2} by (b + group) % 3, an integer mean different for every sample
    (groups = 1: 1, -1, 2, -2, ...; several groups: (b + group) % 5 - 2, different between the samples of a group for B <= 5 and small
    enough that the normalised values stay exact in bf16), gamma in {0.5, 1, 2}, integer beta.
    Returns a [B][groups], mean [B][groups], gamma [C], beta [C] (float64)."""
    b = torch.arange(B).view(B, 1)
    k = torch.arange(groups).view(1, groups)
    a = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[(b + k) % 3]
    if groups == 1:
        n = b + 1
        mean = (((n + 1) // 2) * torch.where(n % 2 == 0, -1, 1)).double()
    else:
        assert B <= 5
        mean = ((b + k) % 5 - 2).double()
    return a, mean, choice(g, (C,), [0.5, 1.0, 2.0]), ints(g, (C,), -2, 2)


def gn_ab_tensor(a, mean):
    """The device array the kernels read: (rstd, rstd * mean) pairs, fp32 [B][groups][2] (exact: a is a power of two, mean an integer)."""
    return torch.stack([a, a * mean], -1).float().contiguous()


# ------------------------------------------------------------------------------------------------- roundings
def is_f32(v):
    return torch.equal(v.double().float().double(), v.double())


def is_bf16(v):
    return torch.equal(v.double().float().bfloat16().double(), v.double())


def rne_bf16(v):
    """ONE rounding (to nearest, ties to even) of an exactly known float64 value: float64 -> float32 is exact (asserted), -> bfloat16 rounds."""
    assert is_f32(v), "the exact value must be representable in fp32"
    return v.double().float().bfloat16()


def store(v, bf16):
    """What a kernel of this output type stores for the exact value v."""
    assert is_f32(v)
    return rne_bf16(v) if bf16 else v.double().float()


def trunc_bf16(v):
    """A defective store: truncation toward zero instead of rounding."""
    return (v.double().float().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def rounding_profile(v):
    """(share of values that bf16 cannot hold, number of exact ties among them) of a float64 tensor of fp32-exact values."""
    low = v.double().float().view(torch.int32) & 0xFFFF
    return (low != 0).double().mean().item(), int((low == 0x8000).sum())


# ------------------------------------------------------------------------------------------------- preconditions
def exactness_margin(x, w, *adds, stride=1, pad=0, transposed=False, groups=1, scale=1.0, unit=1.0):
    """max over outputs of scale * sum |x| |w| plus the largest |.| of every added term (bias, residual, shift tables, ...), in
    multiples of `unit` (the power of two every operand is a multiple of).  Below 2^24 every partial sum in any order is exact in fp32."""
    if transposed:
        m = F.conv_transpose2d(x.abs().double(), w.abs().double(), None, stride=stride, padding=pad)
    else:
        m = F.conv2d(x.abs().double(), w.abs().double(), None, stride=stride, padding=pad, groups=groups)
    tot = scale * m.max().item()
    for t in adds:
        if t is not None:
            tot += float(torch.as_tensor(t).abs().max())
    return tot / unit


def check_exact(margin):
    assert margin < LIMIT, "sum |x||w| + |bias| + |res| = %.3g units: not below 2^24, partial sums need not be exact" % margin


def check_rounding(v):
    """A 'rounding' case: at least 0.5 % of the expected outputs need a bf16 rounding, with exact ties among them."""
    share, ties = rounding_profile(v)
    assert share >= 0.005 and ties > 0, "only %.4f of the outputs round (%d ties): widen the operand range" % (share, ties)


def unit_of(v):
    """The largest power of two u <= 1 of which every element of v is a multiple."""
    u = 1.0
    while not torch.equal(v / u, (v / u).round()):
        u /= 2
        assert u >= 2.0 ** -10
    return u


def check_stats(v):
    """A 'statistics' case, per sample, with n = v / u the outputs as integers (u = unit_of(sample); 1 where no GroupNorm number is a
    fraction): |n| <= 256 (values counted before and after the bf16 store coincide) and sum n^2 < 2^24 (every fp32 running sum of a
    slot, of v and of v^2, is an integer number of units below 2^24 whatever the kernel's grouping)."""
    assert is_bf16(v)
    for b in range(v.shape[0]):
        n = v[b].double() / unit_of(v[b].double())
        assert n.abs().max().item() <= 256, "sample %d: |v| reaches %g units, beyond 256" % (b, n.abs().max().item())
        assert (n * n).sum().item() < LIMIT, "sample %d: sum v^2 = %.3g units: not below 2^24" % (b, (n * n).sum().item())


# ------------------------------------------------------------------------------------------------- references
def border_maps(w, vec, H, W, pad=1):
    """sum over the taps that fall inside the image of w[o][c][tap] * vec[c], per output pixel: [Cout][H][W].  For 3x3 pad 1 these are
    the nine border classes of the fold tables (t1 without the bias for vec = beta, t2 for vec = gamma); for 1x1 one class."""
    img = vec.view(1, -1, 1, 1).double().expand(1, vec.numel(), H, W)
    return F.conv2d(img, w.double(), None, padding=pad)[0]


def conv_fold_ref(x, w, bias, gamma, beta, a, mean, pad=1):
    """conv(GroupNorm(1, C)(x)) in the kernel's algebra: a * acc + (t1[cls] - a*mean * t2[cls]) with acc = conv(x, w * gamma) (the
    packed weights carry the gain), t1 = bias + sum_{taps in cls} w beta, t2 = sum_{taps in cls} w gamma.  a, mean: [B]."""
    B, _, H, W = x.shape
    acc = F.conv2d(x.double(), w.double() * gamma.view(1, -1, 1, 1), None, padding=pad)
    t1 = border_maps(w, beta, H, W, pad)
    if bias is not None:
        t1 = t1 + bias.view(-1, 1, 1)
    t2 = border_maps(w, gamma, H, W, pad)
    a4, m4 = a.view(B, 1, 1, 1), mean.view(B, 1, 1, 1)
    return a4 * acc + (t1[None] - a4 * m4 * t2[None])


def conv_fold_margin(x, w, bias, gamma, beta, a, mean, res=None, pad=1, unit=0.25):
    """exactness_margin of conv_fold_ref: a * sum |x| |w gamma| + |t1| + |a mean t2| (+ |res|), in units of `unit`."""
    _, _, H, W = x.shape
    t1 = border_maps(w.abs(), beta.abs(), H, W, pad).max() + (bias.abs().max() if bias is not None else 0.0)
    t2 = border_maps(w.abs(), gamma.abs(), H, W, pad).max() * (a * mean).abs().max()
    return exactness_margin(x, w.abs() * gamma.view(1, -1, 1, 1), t1, t2, res, pad=pad, scale=a.max().item(), unit=unit)


def pad_concat(x0, x1, off, H, W):
    """pad_and_concat of the two-source kernels: x1 placed at (off_h, off_w) inside an H x W image of zeros, behind x0's channels."""
    if x1 is None:
        return x0
    p = torch.zeros(x1.shape[0], x1.shape[1], H, W, dtype=x1.dtype)
    p[:, :, off[0]:off[0] + x1.shape[2], off[1]:off[1] + x1.shape[3]] = x1
    return torch.cat([x0, p], 1)


def gn_on_load(x, a, mean, gamma, beta, act, groups):
    """act(GroupNorm(G, C)(x)) as the 80-channel kernels apply it while they stage x: (a * x - a*mean) * gamma + beta per (sample,
    group), rounded to bf16 for the matrix cores (the caller asserts that this rounding is exact).  a, mean: [B][G]."""
    B, C = x.shape[:2]
    rep = C // groups
    a4 = a.repeat_interleave(rep, 1).view(B, C, 1, 1)
    m4 = mean.repeat_interleave(rep, 1).view(B, C, 1, 1)
    y = (a4 * x.double() - a4 * m4) * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)
    if act == "relu":
        y = y.clamp_min(0.0)
    else:
        assert act is None
    return y


def gelu64(x):
    return 0.5 * x.double() * (1.0 + torch.special.erf(x.double() * math.sqrt(0.5)))


# ------------------------------------------------------------------------------------------------- split precision (tier bf16x3)
# The split kernels compute x w as x_hi w_hi + x_lo w_hi + x_hi w_lo with hi = bf16(v), lo = bf16(v - hi) (include/diffusynth_hip.h).  On
# integer operands (or integers times a power of two) hi and lo are such numbers too, each of the three bf16 x bf16 products is exact in
# fp32, and with the sum of their magnitudes below 2^24 units every partial sum is exact in any order: the expected tensor is the float64
# value of that documented algebra, WITHOUT the x_lo w_lo term, bit for bit.
def split_hi_lo(v):
    """(hi, lo) of an fp32-exact float64 tensor, both float64: hi = rne_bf16(v), lo = rne_bf16(v - hi) (v - hi is exact in fp32)."""
    assert is_f32(v), "the value to split must be representable in fp32"
    hi = rne_bf16(v).double()
    return hi, rne_bf16(v.double() - hi).double()


def trunc_split(v):
    """A defective split: the lo plane truncated toward zero instead of rounded."""
    hi = rne_bf16(v).double()
    return hi, trunc_bf16(v.double() - hi).double()


def store_split(v):
    """The OUT_SPLIT store of the exact value v: the two bf16 planes (hi, lo)."""
    hi, lo = split_hi_lo(v)
    return hi.float().bfloat16(), lo.float().bfloat16()


def split_profile(v):
    """(share of elements with lo != 0, share with v != hi + lo: a third part is dropped, the lo plane really rounds, number of exact ties in
    the rounding of hi, number of exact ties in the rounding of lo) of a float64 tensor of fp32-exact values."""
    hi, lo = split_hi_lo(v)
    tie = lambda t: int(((t.double().float().view(torch.int32) & 0xFFFF) == 0x8000).sum())
    return (lo != 0).double().mean().item(), (v.double() != hi + lo).double().mean().item(), tie(v), tie(v.double() - hi)


def check_lo_share(v, least, what):
    share = split_profile(v)[0]
    assert share >= least, "%s: only %.3f of the elements have lo != 0 (at least %.2f asked)" % (what, share, least)


def check_out_split(v):
    """An OUT_SPLIT case: at least 50 % of the expected v have lo != 0, at least 1 % drop a third part, with an exact tie in the lo rounding."""
    s_lo, s_drop, _, ties = split_profile(v)
    assert s_lo >= 0.5 and s_drop >= 0.01 and ties > 0, "split store: lo != 0 on %.3f, v != hi + lo on %.4f, %d ties: widen the operands" % (s_lo, s_drop, ties)


def check_wide3(x):
    """A 'wide3' operand: at least 5 % of the elements drop a third part, with exact ties among the lo roundings."""
    _, s_drop, _, ties = split_profile(x)
    assert s_drop >= 0.05 and ties > 0, "wide3: x != hi + lo on %.4f of the elements, %d ties" % (s_drop, ties)


def _conv(x, w, stride, pad, transposed):
    if transposed:
        return F.conv_transpose2d(x.double(), w.double(), None, stride=stride, padding=pad)
    return F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad)


def _fold_gain(w, gamma, transposed):
    if gamma is None:
        return w.double()
    return w.double() * (gamma.view(-1, 1, 1, 1) if transposed else gamma.view(1, -1, 1, 1))


def conv_x3_ref(x, w, stride=1, pad=0, transposed=False, x1=None, off=(0, 0), gamma=None, split=split_hi_lo):
    """The three convolutions of the split parts, x_hi w_hi + x_lo w_hi + x_hi w_lo, over pad_and_concat(x, x1) (the zeros of the pad region
    split into hi = lo = 0), the GroupNorm gain folded into w BEFORE the split (split3_weight, pack_x3_1x1, the header).  No bias."""
    xin = pad_concat(x, x1, off, x.shape[2], x.shape[3])
    xh, xl = split(xin)
    wh, wl = split_hi_lo(_fold_gain(w, gamma, transposed))
    return _conv(xh, wh, stride, pad, transposed) + _conv(xl, wh, stride, pad, transposed) + _conv(xh, wl, stride, pad, transposed)


def x3_margin(x, w, *adds, stride=1, pad=0, transposed=False, x1=None, off=(0, 0), gamma=None, scale=1.0, scale_min=1.0, unit=1.0):
    """exactness_margin over the three magnitude convolutions, sum |x_hi||w_hi| + |x_lo||w_hi| + |x_hi||w_lo|, times `scale`, plus the largest
    |.| of every added term, in multiples of `unit`: the power of two of which every product of two operand parts, times the smallest factor
    `scale_min` the sum is multiplied by, is a multiple (asserted), as every added term must be."""
    xin = pad_concat(x, x1, off, x.shape[2], x.shape[3])
    xh, xl = split_hi_lo(xin)
    wh, wl = split_hi_lo(_fold_gain(w, gamma, transposed))
    for a in (xh, xl):
        for b in (wh, wl):
            p = a.abs().max().item() and b.abs().max().item() and unit_of(a) * unit_of(b)
            assert not p or p * scale_min >= unit, "a product of operand parts is a multiple of %g only, not of the unit %g" % (p * scale_min, unit)
    m = _conv(xh.abs() + xl.abs(), wh.abs(), stride, pad, transposed) + _conv(xh.abs(), wl.abs(), stride, pad, transposed)
    tot = scale * m.max().item()
    for t in adds:
        if t is not None:
            tot += float(torch.as_tensor(t).abs().max())
    return tot / unit


def conv_x3_fold_ref(x, w, bias, gamma, beta, a, mean, pad=1, split=split_hi_lo):
    """conv(GroupNorm(1, C)(x)) in the split kernels' algebra: a * acc + (t1[cls] - a*mean * t2[cls]) with acc = conv_x3_ref(x, w * gamma) and
    the tables of conv_fold_ref, built from the UNSPLIT fp32 w, gamma and beta (ds_conv_fold_tables gets the same inputs).  a, mean: [B]."""
    B, _, H, W = x.shape
    acc = conv_x3_ref(x, w, pad=pad, gamma=gamma, split=split)
    t1 = border_maps(w, beta, H, W, pad)
    if bias is not None:
        t1 = t1 + bias.view(-1, 1, 1)
    t2 = border_maps(w, gamma, H, W, pad)
    a4, m4 = a.view(B, 1, 1, 1), mean.view(B, 1, 1, 1)
    return a4 * acc + (t1[None] - a4 * m4 * t2[None])


def conv_x3_fold_margin(x, w, bias, gamma, beta, a, mean, res=None, pad=1, unit=0.25):
    """The largest of the three sums that must stay below 2^24 for conv_x3_fold_ref to be exact in fp32, each in its own unit:
      the epilogue  a * (three magnitude convolutions) + |t1| + |a mean t2| (+ |res|) in units of `unit`: x3_margin with the largest
                    entries of the tables as added terms (the accumulator's partial sums are a part of it);
      the tables    ds_conv_fold_tables sums w beta (+ bias) and w gamma in fp32, in an order of its own: sum |w||beta| + |bias| in units
                    of 1 and sum |w||gamma| in units of 1/2 (gamma in {0.5, 1, 2})."""
    _, _, H, W = x.shape
    t1 = border_maps(w, beta, H, W, pad) + (bias.view(-1, 1, 1) if bias is not None else 0.0)
    t2 = border_maps(w, gamma, H, W, pad) * (a * mean).abs().max()
    epi = x3_margin(x, w, t1, t2, res, pad=pad, gamma=gamma, scale=a.max().item(), scale_min=a.min().item(), unit=unit)
    assert unit_of(torch.cat([w.flatten(), beta, bias if bias is not None else beta[:0]])) == 1.0 and unit_of(gamma) >= 0.5
    tab1 = border_maps(w.abs(), beta.abs(), H, W, pad).max().item() + (bias.abs().max().item() if bias is not None else 0.0)
    tab2 = border_maps(w.abs(), gamma.abs(), H, W, pad).max().item() / 0.5
    return max(epi, tab1, tab2)


# ------------------------------------------------------------------------------------------------- the checker
def assert_bits_equal(got, want, what):
    """got, want: tensors of one dtype in NCHW (or any) layout.  Equal bit for bit up to the sign of zero (torch.equal semantics, NaN never
    equal); on failure the number of differing elements and the first few as (b, c, y, x, got, want)."""
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    idx = bad.nonzero()[:8]
    rows = ", ".join("(%s, got %r, want %r)" % (", ".join(str(int(i)) for i in ix), float(got[tuple(ix)]), float(want[tuple(ix)])) for ix in idx)
    raise AssertionError("%s: %d of %d elements differ; first (b, c, y, x, got, want): %s" % (what, int(bad.sum()), bad.numel(), rows))


def assert_stats_exact(sums, v, what):
    """sums [B][2] = float64 sums over the slots of a kernel's (sum, sum of squares) partials; v = the exact integer outputs [B][...]."""
    want = torch.stack([v.double().flatten(1).sum(1), (v.double() ** 2).flatten(1).sum(1)], 1)
    assert torch.equal(sums.double(), want), "%s: statistics (sum, sumsq) per sample %s, expected %s" % (what, sums.tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------- GELU implementations on the CPU
GELU_TAB_LO, GELU_TAB_HI = 0x39800000, 0x40FF0000            # conv_halo3_common.hpp: 2^-12 and 7.96875
GELU_TAB_BASE = GELU_TAB_LO >> 16
GELU_TAB_N = (GELU_TAB_HI >> 16) - GELU_TAB_BASE + 1           # 1920
GELU_POLY_C = [2.748536319e-02, -1.331737041e-01, 2.467794865e-01, -1.447154731e-01, -2.043376267e-01, 4.207932651e-01,
               -2.013681531e-01, -1.442166418e-01, 1.726166159e-01, -1.050815172e-02, -4.117569700e-02, 1.182068978e-02]
E_GELU_TAB = 6.63e-4          # documented bounds (conv_halo3_common.hpp)
E_GELU_POLY = 2.0e-5


def _pattern_f32(p16):
    return (p16.to(torch.int64) << 16).to(torch.int32).view(torch.float32)


def gelu_table():
    """The table as conv3x3_halo3.hip builds it: T(a) = a Phi(-a) at the midpoint of every bf16 bucket [lo, hi) of [2^-12, 8), in float64,
    rounded to fp32.  1920 entries."""
    p = torch.arange(GELU_TAB_N) + GELU_TAB_BASE
    mid = 0.5 * (_pattern_f32(p).double() + _pattern_f32(p + 1).double())
    return (mid * 0.5 * torch.special.erfc(mid * 0.70710678118654752440)).float()


def gelu_tab_f32(x, tab=None):
    """gelu_tab8 on fp32 inputs: relu(x) - table[upper 16 bits of clamp(|x|, 2^-12, 7.96875)], in fp32."""
    tab = gelu_table() if tab is None else tab
    lo, hi = _pattern_f32(torch.tensor(GELU_TAB_LO >> 16)).item(), _pattern_f32(torch.tensor(GELU_TAB_HI >> 16)).item()
    a = x.float().abs().clamp(lo, hi)
    idx = (a.view(torch.int32).to(torch.int64) >> 16) - GELU_TAB_BASE
    return x.float().clamp_min(0.0) - tab[idx]


def all_bf16_values(lo_mag=None, hi_mag=None):
    """Every finite bf16 value (both signs, +-0 included) as fp32, optionally those with lo_mag <= |x| <= hi_mag plus +-0."""
    v = _pattern_f32(torch.arange(65536))
    v = v[torch.isfinite(v)]
    if lo_mag is not None:
        v = v[((v.abs() >= lo_mag) & (v.abs() <= hi_mag)) | (v == 0)]
    return v


def gelu_poly_f32(x):
    """gelu_poly8 on fp32 inputs, every fma with ONE fp32 rounding (the products are formed in float64: 24 x 24 bits are exact there)."""
    f32 = lambda t: t.float().double()
    fma = lambda p, q, r: f32(p * q + r)
    c = [f32(torch.tensor(v, dtype=torch.float64)) for v in GELU_POLY_C]
    xd = x.float().double()
    k = f32(f32(torch.tensor(2.0, dtype=torch.float64)) / 4.5)
    t = fma(xd.abs().clamp_max(4.5), k, -1.0)
    u = fma(c[11], t, c[10])
    for i in range(9, -1, -1):
        u = fma(u, t, c[i])
    return f32(xd.clamp_min(0.0) - u).float()
