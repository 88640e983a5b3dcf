"""The split-precision halo kernels walk a source chunk's three products on as few staged halos and fragment reads as they need:
conv3x3_halo3 interleaves (hi, W_hi) and (hi, W_lo) tap by tap on one set of pixel fragments, conv_quad_halo3 stages each hi halo once
(its 32- and 16-wide tiles; the 8-wide one keeps the packed order).  A tap or a weight set paired with the wrong fragment, halo or weight tile must fail by BITS: the exact tests use operands whose split
is exact and whose three products sum without rounding in fp32, in any order — the fp32 output must equal the float64 sum.  The
tolerance tests run the same shapes on random fp32 data against torch in float64 with the bound of the split-precision tests of
tests/test_hip_kernels.py (3e-5)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from diffusynth_amd import _lib as L
from diffusynth_amd.synth import synth_input

pytestmark = pytest.mark.gpu

TOL = 3e-5

# (B, Cin, H, W), Cout, K slices (the ABI takes 2, 3, 4, 6, 8).  32-wide tile with three source chunks; 16-wide, ragged height; 8-wide,
# a single chunk; five chunks; the deepest level's production slices (six of one source chunk); two samples per block with an odd batch (the 8-wide pair form)
SHAPES_3X3 = [((2, 96, 8, 64), 192, (1, 3)), ((1, 64, 37, 16), 96, (1, 2)), ((2, 32, 33, 8), 96, (1,)), ((2, 160, 8, 32), 96, (1,)),
              ((2, 192, 16, 16), 96, (1, 2, 3, 6)), ((3, 64, 16, 8), 96, (1,))]
# mode, Cin, Cout, (H, W) of the input, K slices (every count the ABI takes that leaves slices of a multiple of six chunks)
SHAPES_QUAD = [("up", 192, 96, (9, 27), (1, 3)), ("down", 96, 192, (18, 54), (1, 2, 3, 6)), ("down", 384, 384, (32, 16), (1, 2, 3, 4, 6, 8))]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    L.load()


def _ints(name, shape, lo, hi, nonzero=False):
    """Deterministic integers in [lo, hi] (from the project's seeded generator), optionally without zero."""
    u = synth_input(name, shape)
    v = torch.floor((u - u.min()) / (u.max() - u.min() + 1e-6) * (hi - lo + 1)).clamp(0, hi - lo) + lo
    if nonzero:
        v = torch.where(v == 0, torch.full_like(v, float(hi)), v)
    return v


def _exact_operands(tag, xshape, wshape):
    """x = xh + xl, w = wh + wl: xh in {-1, 0, 1}, wh in {+-1, +-2}, xl in {-3 .. 3} * 2^-10, wl in {-1, 0, 1} * 2^-10.  bf16(w) == wh
    (|wl| is below half a bf16 step of every wh), every product is a multiple of 2^-10, and with at most 6144 of them per output the
    sum of their magnitudes stays below 2^14: 24 bits — exact in fp32 in any order (checked by the caller on the CPU)."""
    xh = _ints(tag + "xh", xshape, -1, 1)
    xl = _ints(tag + "xl", xshape, -3, 3) * 2.0 ** -10
    wh = _ints(tag + "wh", wshape, -2, 2, nonzero=True)
    wl = _ints(tag + "wl", wshape, -1, 1) * 2.0 ** -10
    return xh, xl, wh, wl


def _planes(xh, xl):
    """NCHW hi / lo -> the DS_CONV_F_SPLIT_IN input: NHWC bf16 [.., 2C] = hi plane, lo plane."""
    xs = torch.cat([xh, xl], 1).permute(0, 2, 3, 1).contiguous().bfloat16()
    assert torch.equal(xs.float().permute(0, 3, 1, 2), torch.cat([xh, xl], 1))
    return xs.cuda()


def _check_exact(want, mag):
    """The float64 sum is an fp32 number and no partial sum can round: multiples of 2^-10 whose magnitudes sum below 2^14."""
    assert mag.max().item() < 2.0 ** 14
    assert torch.equal(want * 1024, torch.round(want * 1024)) and torch.equal(want.float().double(), want)


def _run_3x3(xs, pc, cout, out_mode, ks, act, fold=None, res=None):
    """One split-precision 3x3 launch (+ reduce for K slices) -> NCHW fp32 on the CPU.  fold = (gn_ab, t1, t2) or None."""
    B, Hh, Ww, C2 = xs.shape
    split = out_mode == "split"
    out = torch.full((B, Hh, Ww, 2 * cout if split else cout), float("nan"), device="cuda")
    if split:
        out = out.bfloat16()
    p = L.ConvParams(src0=xs.data_ptr(), src1=None, C0=C2, C1=0, H=Hh, W=Ww, H1=0, W1=0, off_h1=0, off_w1=0, wpk=pc.w.data_ptr(), Cout=cout,
                     cout_pad=pc.cout_pad, KH=3, KW=3, stride=1, pad_h=1, pad_w=1, Ho=Hh, Wo=Ww, transposed=0, out=out.data_ptr(),
                     out_C=out.shape[-1], out_c0=0, out_nchw_f32=0, bias=pc.bias.data_ptr(), gn_ab=fold[0].data_ptr() if fold else None,
                     fold_t1=fold[1].data_ptr() if fold else None, fold_t2=fold[2].data_ptr() if fold else None, ncls=9 if fold else 1,
                     act=act, res=L.ptr(res), stats_part=None, B=B, dtype=L.DS_BF16, tile=L.TILE_HALO3_256x96, wk_order=1,
                     flags=1 | (2 if split else 4))
    slab = None
    if ks > 1:
        slab = torch.full((ks * B * Hh * Ww * ((cout + 7) // 8 * 8),), float("nan"), device="cuda")
        p.ksplit, p.slab = ks, slab.data_ptr()
    L.call("ds_conv_igemm", C.byref(p), L.current_stream())
    if ks > 1:
        L.call("ds_conv_splitk_reduce", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    got = out.float()
    if split:
        got = got[..., :cout] + got[..., cout:]
    return got.permute(0, 3, 1, 2).cpu()


def _run_quad(xs, w, bias, tr, ks):
    """One split-precision Down / Upsample launch (weights [W_hi | W_hi | W_lo] as quad tiles, fp32 output) -> NCHW fp32 on the CPU."""
    from diffusynth_amd.engine import pack_quad_weights
    B, Hh, Ww, C2 = xs.shape
    cin = C2 // 2
    cout = w.shape[1] if tr else w.shape[0]
    hi = w.bfloat16().float()
    wpk, cout_pad = pack_quad_weights(torch.cat([hi, hi, w - hi], 0 if tr else 1).cuda(), tr)
    oh, ow = (2 * Hh, 2 * Ww) if tr else (Hh // 2, Ww // 2)
    gh, gw = (Hh, Ww) if tr else (oh, ow)
    out = torch.full((B, oh, ow, cout), float("nan"), device="cuda")
    bd = bias.cuda()
    p = L.ConvParams(src0=xs.data_ptr(), src1=None, C0=2 * cin, C1=0, H=Hh, W=Ww, H1=0, W1=0, off_h1=0, off_w1=0, wpk=wpk.data_ptr(), Cout=cout,
                     cout_pad=cout_pad, KH=2 if tr else 4, KW=2 if tr else 4, stride=1 if tr else 2, pad_h=0 if tr else 1, pad_w=0 if tr else 1,
                     Ho=gh, Wo=gw, transposed=1 if tr else 0, out=out.data_ptr(), out_C=cout, out_c0=0, out_nchw_f32=0, bias=bd.data_ptr(),
                     gn_ab=None, fold_t1=None, fold_t2=None, ncls=1, act=L.ACT_NONE, res=None, stats_part=None, B=B, dtype=L.DS_BF16,
                     tile=L.TILE_QUAD_HALO3, wk_order=2, flags=1 | 4)
    slab = None
    if ks > 1:
        slab = torch.full((ks, B, oh, ow, (cout + 7) // 8 * 8), float("nan"), device="cuda")
        p.ksplit, p.slab = ks, slab.data_ptr()
    L.call("ds_conv_igemm", C.byref(p), L.current_stream())
    if ks > 1:
        L.call("ds_conv_splitk_reduce", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("shape,cout,slices", SHAPES_3X3)
def test_conv3x3_halo3_pairs_every_tap_and_weight_set_exactly(shape, cout, slices):
    import hip_helpers as h
    from diffusynth_amd.engine import split3_weight
    B, Cin, Hh, Ww = shape
    xh, xl, wh, wl = _exact_operands("hr3_%s_%d" % (shape, cout), shape, (cout, Cin, 3, 3))
    w = wh + wl
    assert torch.equal(w.bfloat16().float(), wh) and torch.equal(w - wh, wl)          # the packer's split is (wh, wl)
    bias = _ints("hr3_b%d" % cout, (cout,), -4, 4)
    want = F.conv2d((xh + xl).double(), wh.double(), bias.double(), padding=1) + F.conv2d(xh.double(), wl.double(), padding=1)
    _check_exact(want, F.conv2d((xh + xl).abs().double(), wh.abs().double(), bias.abs().double(), padding=1) + F.conv2d(xh.abs().double(), wl.abs().double(), padding=1))
    pc = h.PackedConv(split3_weight(w, None), bias, L.DS_BF16, L.TILE_HALO3_256x96)
    xs = _planes(xh, xl)
    for ks in slices:
        assert (Cin // 32) % ks == 0
        got = _run_3x3(xs, pc, cout, "f32", ks, L.ACT_NONE)
        assert torch.equal(got, want.float()), (ks, (got.double() - want).abs().max().item())


@pytest.mark.parametrize("mode,cin,cout,hw,slices", SHAPES_QUAD)
def test_conv_quad_halo3_pairs_every_halo_and_weight_group_exactly(mode, cin, cout, hw, slices):
    tr = mode == "up"
    B = 2
    xh, xl, wh, wl = _exact_operands("hrq_%s%d_%d" % (mode, cin, cout), (B, cin, *hw), (cin, cout, 4, 4) if tr else (cout, cin, 4, 4))
    w = wh + wl
    assert torch.equal(w.bfloat16().float(), wh) and torch.equal(w - wh, wl)
    bias = _ints("hrq_b%d" % cout, (cout,), -4, 4)
    conv = (lambda a, b, c=None: F.conv_transpose2d(a, b, c, stride=2, padding=1)) if tr else (lambda a, b, c=None: F.conv2d(a, b, c, stride=2, padding=1))
    want = conv((xh + xl).double(), wh.double(), bias.double()) + conv(xh.double(), wl.double())
    _check_exact(want, conv((xh + xl).abs().double(), wh.abs().double(), bias.abs().double()) + conv(xh.abs().double(), wl.abs().double()))
    xs = _planes(xh, xl)
    nch = (1 if tr else 4) * 3 * cin // 32
    for ks in slices:
        assert nch % ks == 0 and (nch // ks) % 6 == 0
        got = _run_quad(xs, w, bias, tr, ks)
        assert torch.equal(got, want.float()), (ks, (got.double() - want).abs().max().item())


@pytest.mark.parametrize("out_mode", ["split", "f32", "f32+res"])
@pytest.mark.parametrize("shape,cout,slices", SHAPES_3X3)
def test_conv3x3_halo3_split_precision_within_tolerance(shape, cout, slices, out_mode):
    """Random fp32 data, GroupNorm fold, the three output modes (hi / lo planes with GELU, fp32, fp32 + fp32 residual)."""
    import hip_helpers as h
    from diffusynth_amd.engine import split3_weight, to_split_planes
    B, Cin, Hh, Ww = shape
    x = synth_input("hr3t_x%s" % (shape,), shape) * 1.5 + 0.4
    w = synth_input("hr3t_w%d_%d" % (cout, Cin), (cout, Cin, 3, 3), 0.05)
    bb = synth_input("hr3t_b%d" % cout, (cout,))
    gam = 1 + 0.2 * synth_input("hr3t_g%d" % Cin, (Cin,))
    bet = 0.3 * synth_input("hr3t_be%d" % Cin, (Cin,))
    r = synth_input("hr3t_r%s%d" % (shape, cout), (B, cout, Hh, Ww))
    xs = to_split_planes(x.permute(0, 2, 3, 1).contiguous()).cuda()
    xq = (xs[..., :Cin].float() + xs[..., Cin:].float()).permute(0, 3, 1, 2).cpu()          # what the kernel sees
    want = F.conv2d(F.group_norm(xq.double(), 1, gam.double(), bet.double(), 1e-5), w.double(), bb.double(), padding=1)
    if out_mode == "split":
        want = F.gelu(want)
    if out_mode == "f32+res":
        want = want + r.double()
    pc = h.PackedConv(split3_weight(w, gam), bb, L.DS_BF16, L.TILE_HALO3_256x96)
    t1, t2 = torch.empty(9 * cout, device="cuda"), torch.empty(9 * cout, device="cuda")
    wd, gd, bd = w.cuda().contiguous(), gam.cuda(), bet.cuda()
    L.call("ds_conv_fold_tables", wd.data_ptr(), pc.bias.data_ptr(), gd.data_ptr(), bd.data_ptr(), cout, Cin, 3, 3, t1.data_ptr(), t2.data_ptr(),
           L.current_stream())
    fold = (h.gn_ab_of(xq), t1, t2)
    rd = r.permute(0, 2, 3, 1).contiguous().cuda() if out_mode == "f32+res" else None
    for ks in slices:
        got = _run_3x3(xs, pc, cout, "split" if out_mode == "split" else "f32", ks, L.ACT_GELU if out_mode == "split" else L.ACT_NONE, fold, rd)
        e = rel_err(got, want.float())
        print("3x3 %s %s ks=%d: %.2e" % (shape, out_mode, ks, e))
        assert e < TOL, (ks, e)


@pytest.mark.parametrize("mode,cin,cout,hw,slices", SHAPES_QUAD)
def test_conv_quad_halo3_split_precision_within_tolerance(mode, cin, cout, hw, slices):
    from diffusynth_amd.engine import to_split_planes
    tr = mode == "up"
    B = 2
    x = synth_input("hrqt_x%s%d" % (mode, cin), (B, cin, *hw)) * 1.5 + 0.3
    w = synth_input("hrqt_w%s%d_%d" % (mode, cin, cout), (cin, cout, 4, 4) if tr else (cout, cin, 4, 4), 0.05)
    bb = synth_input("hrqt_b%d" % cout, (cout,))
    want = (F.conv_transpose2d(x.double(), w.double(), bb.double(), stride=2, padding=1) if tr
            else F.conv2d(x.double(), w.double(), bb.double(), stride=2, padding=1))
    xs = to_split_planes(x.permute(0, 2, 3, 1).contiguous()).cuda()
    for ks in slices:
        got = _run_quad(xs, w, bb, tr, ks)
        e = rel_err(got, want.float())
        print("quad %s %d->%d ks=%d: %.2e" % (mode, cin, cout, ks, e))
        assert got.shape == want.shape and e < TOL, (ks, e)
