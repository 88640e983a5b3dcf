"""GroupNorm from raw partials, in every kernel that reduces them (GPU).

The engines hand a producer's per-block (sum, sumsq) partials straight to the consumer (ds_*_params.gn_part / gn_parts / gn_count /
gn_eps): no ds_gn_finalize launch in between.  Part A feeds SYNTHETIC partials (tests/gn_partials_ref.py: distinct samples, quarter-sized
end chunks, NaN guards, an 8-byte-aligned base) into every consumer and holds each launch (1) to the float64 reference at the tolerance
of that kernel's gn_ab test in tests/test_hip_kernels.py and (2) bit for bit to the same kernel's gn_ab form fed by ds_gn_finalize of the
same buffer.  tests/test_gn_partials_cpu.py shows that a wrong sample, a lost tail or an off-by-one partial moves each of these results
by at least ten tolerances.  Part B runs the real producers — every depthwise family and instantiation — and the producer -> consumer
chains the engines run, against the float64 composite of the producer's stored output."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_partials_ref as R
from conftest import rel_err
from diffusynth_amd import _lib as L

pytestmark = pytest.mark.gpu

DT = {"f32": L.DS_F32, "bf16": L.DS_BF16}
ACT = {"none": L.ACT_NONE, "gelu": L.ACT_GELU, "silu": L.ACT_SILU, "relu": L.ACT_RELU}
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    L.load()


def H():
    import hip_helpers
    return hip_helpers


def note(line):
    """Figures worth keeping (profiles/gn_partials_parity.txt): printed, and appended to $DS_GN_PARITY_LOG when that is set."""
    print(line)
    path = os.environ.get("DS_GN_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def device_partials(case, parts):
    """(guarded device buffer, float64 statistics of the contract) for a case's input cut into ``parts`` partials."""
    part = R.case_partials(case, parts)
    assert R.order_independent(part, case.count)          # any float64 summation order gives the same fp32 pair: bit-identity is expected
    return R.guarded(part), R.ab_from_partials(part, case.count)


def finalize(gpart, count, eps=R.EPS):
    B, parts, _ = gpart.shape
    ab = torch.empty(B, 2, device="cuda")
    L.call("ds_gn_finalize", gpart.data_ptr(), B, parts, float(count), eps, ab.data_ptr(), L.current_stream())
    return ab


def set_part(p, gpart, count, eps=R.EPS):
    p.gn_ab, p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = None, gpart.data_ptr(), gpart.shape[1], float(count), eps


def check(got_nchw, ref, tol, what):
    assert torch.isfinite(got_nchw).all(), what
    err = rel_err(got_nchw, ref)
    assert err < tol, (what, err, tol)
    return err


# ================================================================================================ part A: ds_gn_apply
def launch_gn_apply(case, xd, rd, cbd, gd, bd, gpart=None, gn_ab=None, G=1):
    out = torch.full_like(xd, NAN)
    p = L.GnApplyParams(x=xd.data_ptr(), res=L.ptr(rd), out=out.data_ptr(), gn_ab=L.ptr(gn_ab), gamma=gd.data_ptr(), beta=bd.data_ptr(),
                        cbias=L.ptr(cbd), cb_stride=case.C, B=case.B, HW=case.HW, C=case.C, G=G, act=ACT[case.act], dtype=DT[case.dt])
    if gpart is not None:
        p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = gpart.data_ptr(), gpart.shape[1], float(case.count), R.EPS
    L.call("ds_gn_apply", C.byref(p), L.current_stream())
    H().sync()
    return out


def gn_apply_operands(case):
    h = H()
    dt = DT[case.dt]
    xd = h.to_nhwc(case.x, dt)
    rd = h.to_nhwc(case.r, dt) if case.r is not None else None
    cbd = case.cb.cuda().contiguous() if case.cb is not None else None
    return xd, rd, cbd, case.g.cuda(), case.be.cuda()


@pytest.mark.parametrize("args", R.GN_APPLY_FAST + [R.GN_APPLY_CAP], ids=lambda a: "C%d_HW%d_B%d_res%d" % (a[1], a[2], a[3], a[4]))
def test_gn_apply_fast_from_partials(args):
    """gn_apply_lazy_fast_kernel<res> (bf16, no activation, no channel bias; 16 launches per forward): every channel count of its thread
    map, fewer pixels than rows, a ragged last pass, several blocks, and the grid cap (B = 64: 65 blocks wanted, 64 allowed).  Its gn_ab
    form is ANOTHER kernel (gn_apply_table_kernel) that forms the same scale a * gamma and shift fma(-a mean, gamma, beta) and the same
    fma per element: bit-identical outputs are expected and asserted."""
    case = R.gn_apply_case(*args)
    h = H()
    ops = gn_apply_operands(case)
    for parts in case.parts:
        gpart, ab = device_partials(case, parts)
        out = launch_gn_apply(case, *ops, gpart=gpart)
        check(h.from_nhwc(out), case.ref(ab), case.tol, (case.id, parts))
        out_ab = launch_gn_apply(case, *ops, gn_ab=finalize(gpart, case.count))
        assert torch.equal(bits(out), bits(out_ab)), (case.id, parts)


# generic lazy kernel against the float64 reference: 4 x the error measured on the MI355X (profiles/gn_partials_parity.txt: 1.02e-7,
# 2.33e-3 and 2.93e-3, the bf16 figures being the rounding of the stored result; the forms differ from each other by 7.9e-8, 2.9e-4, 2.9e-6)
LAZY_BOUND = {"gp_ga_f32_96_70_3_res_none": 4.1e-7, "gp_ga_bf16_160_70_3_cb_none": 9.3e-3, "gp_ga_bf16_96_70_3_silu": 1.2e-2}


@pytest.mark.parametrize("args", R.GN_APPLY_LAZY, ids=lambda a: "%s_C%d_%s" % (a[0], a[1], a[6]))
def test_gn_apply_lazy_from_partials(args):
    """gn_apply_lazy_kernel<T> (every gn_part launch the fast form does not take: fp32, a channel bias, an activation, a channel count
    whose vectors do not divide 192).  It evaluates ((x * a - a mean) * gamma + beta) per element, its gn_ab counterpart
    (gn_apply_table_kernel) fma(x, a * gamma, beta - a mean * gamma): two roundings placed differently, so the two forms legitimately
    differ in the last bit of some elements.  Instead of bit-identity the gn_part form is held to 4 x the error measured against the
    float64 reference (LAZY_BOUND), next to the tolerance of test_gn_stats_and_apply, and the two forms to each other at that same bound."""
    case = R.gn_apply_case(*args)
    h = H()
    ops = gn_apply_operands(case)
    for parts in case.parts:
        gpart, ab = device_partials(case, parts)
        out = launch_gn_apply(case, *ops, gpart=gpart)
        ref = case.ref(ab)
        err = check(h.from_nhwc(out), ref, case.tol, (case.id, parts))
        out_ab = launch_gn_apply(case, *ops, gn_ab=finalize(gpart, case.count))
        err_ab = rel_err(h.from_nhwc(out_ab), ref)
        between = rel_err(out.float(), out_ab.float())
        note("gn_apply lazy %-32s parts %3d: gn_part form vs float64 %.3e, gn_ab (table kernel) form %.3e, between the forms %.3e"
             % (case.id, parts, err, err_ab, between))
        bound = LAZY_BOUND[case.id]
        assert err < bound and between < bound, (case.id, parts, err, between, bound)


def test_gn_apply_partials_rejections():
    """ds_gn_apply refuses partials with G > 1, together with gn_ab, and with gn_parts = 0 (or no count)."""
    case = R.gn_apply_case(*R.GN_APPLY_LAZY[2])
    xd, rd, cbd, gd, bd = gn_apply_operands(case)
    gpart, _ = device_partials(case, 65)
    ab = finalize(gpart, case.count)
    out = torch.empty_like(xd)

    def params(**kw):
        p = L.GnApplyParams(x=xd.data_ptr(), res=None, out=out.data_ptr(), gn_ab=None, gamma=gd.data_ptr(), beta=bd.data_ptr(), cbias=None,
                            cb_stride=0, B=case.B, HW=case.HW, C=case.C, G=1, act=L.ACT_NONE, dtype=L.DS_BF16)
        p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = gpart.data_ptr(), 65, float(case.count), R.EPS
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    L.call("ds_gn_apply", C.byref(params()), L.current_stream())                       # the plain launch is fine
    for bad in (dict(G=8), dict(gn_ab=ab.data_ptr()), dict(gn_parts=0), dict(gn_count=0.0)):
        with pytest.raises(L.DsError, match="partials need"):
            L.call("ds_gn_apply", C.byref(params(**bad)), L.current_stream())
    H().sync()


# ================================================================================================ part A: convolutions
def stats_close(st, want, rtol, atol0, both=True):
    s = st.double().sum(1).cpu()
    wd = want.double().flatten(1)
    if both:
        np.testing.assert_allclose(s[:, 0], wd.sum(1), rtol=rtol, atol=atol0)
    np.testing.assert_allclose(s[:, 1], (wd * wd).sum(1), rtol=rtol)


@pytest.mark.parametrize("args", R.IGEMM, ids=lambda a: "%s_%dx%d" % (a[0], a[3], a[3]))
def test_conv_igemm_from_partials(args):
    """The generic implicit-GEMM kernel's prologue (conv_gn_prologue -> gn_from_partials): the 3x3 fold case with GELU + residual +
    statistics on TILE_128x192 and the 1x1 fold case on TILE_128x192 and TILE_256x96, both dtypes."""
    case = R.conv_case(*args)
    h = H()
    dt = DT[case.mode]
    xd = h.to_nhwc(case.x, dt)
    rd = h.to_nhwc(case.r, dt) if case.r is not None else None
    for tile in ((L.TILE_128x192,) if case.k == 3 else (L.TILE_128x192, L.TILE_256x96)):
        pc = h.PackedConv(case.w, case.b, dt, tile, gamma=case.g, beta=case.be)
        kw = dict(pad=case.k // 2, act=ACT[case.act], res=rd, want_stats=case.k == 3)
        for parts in case.parts:
            gpart, ab = device_partials(case, parts)
            y, st = h.run_conv(pc, xd, gn_part=(gpart, parts, case.count, R.EPS), **kw)
            want = case.ref(ab)
            check(h.from_nhwc(y), want, case.tol, (case.id, tile, parts))
            if st is not None:                                       # the assertions of test_conv3x3_gn_fold_gelu_stats_residual
                stats_close(st, want, 5e-3 if dt else 1e-4, 1e-2)
            y2, st2 = h.run_conv(pc, xd, gn_ab=finalize(gpart, case.count), **kw)
            assert torch.equal(bits(y), bits(y2)), (case.id, tile, parts)
            if st is not None:
                assert torch.equal(bits(st), bits(st2))


def legal_ksplit(cin, want):
    """K slices are whole 32-channel source chunks: a count that does not divide them is refused by the library (96 channels: 1 and 3;
    64: 1 and 2; 32: 1)."""
    return [ks for ks in want if (cin // 32) % ks == 0]


@pytest.mark.parametrize("shape,cout", R.HALO_BF16, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv3x3_halo_from_partials(shape, cout):
    """The halo kernel's two-phase prologue in bf16: gn_partials_issue (4 x 64 range-checked pair loads: partials beyond `parts` must read
    as zeros, not as the next sample or the guard) and gn_partials_finish (the tail walk beyond 256) on all three patch widths, GELU +
    residual + statistics; with K slices the partials are reduced by ds_conv_splitk_reduce instead."""
    case = R.conv_case("bf16", shape, cout, 3, "gelu", True, None, True)
    h = H()
    dt = L.DS_BF16
    xd, rd = h.to_nhwc(case.x, dt), h.to_nhwc(case.r, dt)
    pc = h.PackedConv(case.w, case.b, dt, L.TILE_HALO3_256x96, gamma=case.g, beta=case.be)
    for ks in legal_ksplit(shape[1], (1, 2, 3)):
        kw = dict(pad=1, act=L.ACT_GELU, res=rd, want_stats=True, ksplit=ks)
        for parts in case.parts:
            gpart, ab = device_partials(case, parts)
            y, st = h.run_conv(pc, xd, gn_part=(gpart, parts, case.count, R.EPS), **kw)
            want = case.ref(ab)
            check(h.from_nhwc(y), want, case.tol, (case.id, ks, parts))
            stats_close(st, want, 1e-2, 0.5)                         # the assertions of test_conv3x3_halo_matches_conv2d
            y2, st2 = h.run_conv(pc, xd, gn_ab=finalize(gpart, case.count), **kw)
            assert torch.equal(bits(y), bits(y2)) and torch.equal(bits(st), bits(st2)), (case.id, ks, parts)


def conv_params(x, w, out, out_C, B, Cin_stored, Hh, Ww, cout, cout_pad, **kw):
    p = L.ConvParams(src0=x.data_ptr(), src1=None, C0=Cin_stored, C1=0, H=Hh, W=Ww, H1=0, W1=0, off_h1=0, off_w1=0, wpk=w.data_ptr(), Cout=cout,
                     cout_pad=cout_pad, KH=3, KW=3, stride=1, pad_h=1, pad_w=1, Ho=Hh, Wo=Ww, transposed=0, out=out.data_ptr(), out_C=out_C,
                     out_c0=0, out_nchw_f32=0, bias=None, gn_ab=None, fold_t1=None, fold_t2=None, ncls=9, act=L.ACT_NONE, res=None,
                     stats_part=None, B=B, dtype=L.DS_BF16, tile=L.TILE_HALO3_256x96, wk_order=1)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def launch_conv(p, B, ks=1, slab_elems=0):
    """One ds_conv_igemm launch (+ ds_conv_splitk_reduce for K slices) with fresh statistics partials; returns them."""
    p.ksplit, p.slab, p.stats_part = ks, None, None
    slab = None
    if ks > 1:
        slab = torch.full((ks * slab_elems,), NAN, device="cuda")
        p.slab = slab.data_ptr()
    st = torch.zeros(B, L.load().ds_conv_stats_parts(C.byref(p)), 2, device="cuda")
    p.stats_part = st.data_ptr()
    L.call("ds_conv_igemm", C.byref(p), L.current_stream())
    if ks > 1:
        L.call("ds_conv_splitk_reduce", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    return st


class X3Conv:
    """Operands of one split-precision 3x3 halo launch (DS_CONV_F_SPLIT_IN): weights [W_hi | W_lo | W_hi] with the GroupNorm gain folded,
    fold tables, bias."""

    def __init__(self, w, b, g, be):
        from diffusynth_amd.engine import split3_weight
        h = H()
        self.cout, self.cin = w.shape[0], w.shape[1]
        self.pc = h.PackedConv(split3_weight(w, g), b, L.DS_BF16, L.TILE_HALO3_256x96)
        self.t1, self.t2 = torch.empty(9 * self.cout, device="cuda"), torch.empty(9 * self.cout, device="cuda")
        wd, gd, bd = w.cuda().contiguous(), g.cuda(), be.cuda()
        L.call("ds_conv_fold_tables", wd.data_ptr(), self.pc.bias.data_ptr(), gd.data_ptr(), bd.data_ptr(), self.cout, self.cin, 3, 3,
               self.t1.data_ptr(), self.t2.data_ptr(), L.current_stream())
        h.sync()

    def run(self, xs, B, Hh, Ww, split_out, gelu, rd=None, ks=1, gpart=None, count=None, gn_ab=None):
        """xs: hi / lo planes [B][H][W][2 Cin] bf16.  Returns (result NCHW fp32 on the host, raw output tensor, statistics partials)."""
        cout = self.cout
        if split_out:
            out = torch.full((B, Hh, Ww, 2 * cout), NAN, device="cuda").bfloat16()
        else:
            out = torch.full((B, Hh, Ww, cout), NAN, device="cuda")
        p = conv_params(xs, self.pc.w, out, 2 * cout if split_out else cout, B, 2 * self.cin, Hh, Ww, cout, self.pc.cout_pad,
                        bias=self.pc.bias.data_ptr(), fold_t1=self.t1.data_ptr(), fold_t2=self.t2.data_ptr(), gn_ab=L.ptr(gn_ab),
                        act=L.ACT_GELU if gelu else L.ACT_NONE, res=L.ptr(rd), flags=1 | (2 if split_out else 4))
        if gpart is not None:
            set_part(p, gpart, count)
        st = launch_conv(p, B, ks, B * Hh * Ww * ((cout + 7) // 8 * 8))
        got = out.float()
        if split_out:
            got = got[..., :cout] + got[..., cout:]
        return got.permute(0, 3, 1, 2).cpu(), out, st


@pytest.mark.parametrize("out_mode", ["split_gelu", "f32_res"])
@pytest.mark.parametrize("shape,cout", R.HALO_X3, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv3x3_halo3_split_precision_from_partials(shape, cout, out_mode):
    """The split-precision instantiation (flags 1|2: GELU, hi / lo planes out; 1|4: fp32 out + fp32 residual), including PAIR — two samples
    per block on images of at most 16 x 8, whose SECOND sample's partials are reduced by a separate gn_from_partials; the odd batch
    leaves the last block with one sample — and K slices (ds_conv_splitk_reduce reduces the partials; PAIR is off there)."""
    from diffusynth_amd.engine import to_split_planes
    gelu = out_mode == "split_gelu"
    case = R.conv_case("x3", shape, cout, 3, "gelu" if gelu else "none", not gelu, None, True)
    B, Cin, Hh, Ww = shape
    cv = X3Conv(case.w, case.b, case.g, case.be)
    xs = to_split_planes(R.nhwc(case.x)).cuda()
    rd = R.nhwc(case.r).cuda() if case.r is not None else None
    for ks in legal_ksplit(Cin, (1, 2, 3)):
        for parts in case.parts:
            gpart, ab = device_partials(case, parts)
            got, raw, st = cv.run(xs, B, Hh, Ww, gelu, gelu, rd, ks, gpart=gpart, count=case.count)
            want = case.ref(ab)
            check(got, want, case.tol, (case.id, ks, parts))
            s = st.double().sum(1).cpu()                           # test_conv3x3_halo3_split_precision asserts the sum of squares at 1e-4; the
            wd = want.flatten(1)                                   # plain sum is held to the same 1e-4 of its magnitude sum (a signed sum cancels)
            np.testing.assert_allclose(s[:, 1], (wd * wd).sum(1), rtol=1e-4)
            assert ((s[:, 0] - wd.sum(1)).abs() <= 1e-4 * wd.abs().sum(1)).all()
            _, raw2, st2 = cv.run(xs, B, Hh, Ww, gelu, gelu, rd, ks, gn_ab=finalize(gpart, case.count))
            assert torch.equal(bits(raw), bits(raw2)) and torch.equal(bits(st), bits(st2)), (case.id, ks, parts)


def test_conv3x3_halo_fused_res_conv_from_partials():
    """ConvNeXt conv2 + the block's 1x1 res_conv in one launch ((2,96,9,27), sources (96, 96) with pad offsets): the GroupNorm factor from
    the partials also divides the res_conv accumulator in registers."""
    shape, cout, (c0, c1) = R.HALO_RC
    case = R.conv_case("bf16", shape, cout, 3, "none", False, (c0, c1), True)
    h = H()
    dt = L.DS_BF16
    B, Cin, Hh, Ww = shape
    pc = h.PackedConv(case.w, case.b, dt, L.TILE_HALO3_256x96, gamma=case.g, beta=case.be)
    lib = L.load()
    rpk = torch.empty(lib.ds_pack_conv_elems(c0 + c1, 1, 1, pc.cout_pad, 0), dtype=torch.bfloat16, device="cuda")
    wrd = case.wr.float().contiguous().cuda()
    pp = L.PackConvParams(w=wrd.data_ptr(), gamma=None, dst=rpk.data_ptr(), dtype=dt, Cout=cout, Cin=c0 + c1, cin_pad=c0 + c1, KH=1, KW=1,
                          cout_pad=pc.cout_pad, transposed=0, k_order=1)
    L.call("ds_pack_conv_weight", C.byref(pp), L.current_stream())
    wall = torch.cat([rpk, pc.w])
    brd = case.br.cuda()
    gd, x0d, x1d = h.to_nhwc(case.x, dt), h.to_nhwc(case.x0, dt), h.to_nhwc(case.x1, dt)

    def run(gpart=None, gn_ab=None):
        out = torch.full((B, Hh, Ww, cout), NAN, device="cuda").bfloat16()
        p = conv_params(gd, wall, out, cout, B, Cin, Hh, Ww, cout, pc.cout_pad, bias=pc.bias.data_ptr(), fold_t1=pc.t1.data_ptr(),
                        fold_t2=pc.t2.data_ptr(), gn_ab=L.ptr(gn_ab), res_src0=x0d.data_ptr(), res_src1=x1d.data_ptr(), res_C0=c0, res_C1=c1,
                        res_H1=case.h1, res_W1=case.w1, res_off_h1=case.oh, res_off_w1=case.ow, res_steps=(c0 + c1) // 32, res_bias=brd.data_ptr())
        if gpart is not None:
            set_part(p, gpart, case.count)
        return out, launch_conv(p, B)

    for parts in case.parts:
        gpart, ab = device_partials(case, parts)
        out, st = run(gpart=gpart)
        want = case.ref(ab)
        check(h.from_nhwc(out), want, case.tol, (case.id, parts))
        stats_close(st, want, 1e-2, 0.0, both=False)                # the assertion of test_conv3x3_halo2_with_fused_res_conv
        out2, st2 = run(gn_ab=finalize(gpart, case.count))
        assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(st), bits(st2)), (case.id, parts)


# ================================================================================================ part A: attention
class AttnOperands:
    def __init__(self, case):
        sd, tag, Cc = case.sd, case.tag, case.C
        dev = lambda t: t.float().contiguous().cuda()
        self.wq, self.wo = dev(sd[tag + ".fn.fn.to_qkv.weight"].reshape(384, Cc)), dev(sd[tag + ".fn.fn.to_out.0.weight"].reshape(Cc, 128))
        self.g, self.be = dev(sd[tag + ".fn.norm.weight"]), dev(sd[tag + ".fn.norm.bias"])
        self.t1, self.t2 = torch.empty(384, device="cuda"), torch.empty(384, device="cuda")
        L.call("ds_conv_fold_tables", self.wq.data_ptr(), None, self.g.data_ptr(), self.be.data_ptr(), 384, Cc, 1, 1, self.t1.data_ptr(),
               self.t2.data_ptr(), L.current_stream())
        self.lq = None
        if case.c is not None:
            self.lq = dev(F.linear(case.c, sd[tag + ".fn.fn.label_query.weight"], sd[tag + ".fn.fn.label_query.bias"]))
        self.bo = dev(sd[tag + ".fn.fn.to_out.0.bias"])
        self.go, self.bo2 = dev(sd[tag + ".fn.fn.to_out.1.weight"]), dev(sd[tag + ".fn.fn.to_out.1.bias"])


def output_norm(y, xd, ops, sp, B, N, Cc, dt):
    """The block's tail as the existing attention tests run it: ds_gn_finalize of y's partials, ds_gn_apply with res = x."""
    st = L.current_stream()
    aby = torch.empty(B, 2, device="cuda")
    L.call("ds_gn_finalize", sp.data_ptr(), B, sp.shape[1], float(Cc * N), 1e-5, aby.data_ptr(), st)
    out = torch.full_like(y, NAN)
    gp = L.GnApplyParams(x=y.data_ptr(), res=xd.data_ptr(), out=out.data_ptr(), gn_ab=aby.data_ptr(), gamma=ops.go.data_ptr(),
                         beta=ops.bo2.data_ptr(), cbias=None, cb_stride=0, B=B, HW=N, C=Cc, G=1, act=L.ACT_NONE, dtype=dt)
    L.call("ds_gn_apply", C.byref(gp), st)
    H().sync()
    return out


def run_attn_fused(case, ops, xd, w16, nseg, v2, gpart=None, gn_ab=None):
    B, Cc, N = case.B, case.C, case.hw[0] * case.hw[1]
    wq16, wo16 = w16
    st = L.current_stream()
    part = torch.empty(L.load().ds_linattn_part_floats(B, 4, nseg), device="cuda")
    ctx = torch.empty(B * 4 * 1024, device="cuda")
    y = torch.full((B, case.hw[0], case.hw[1], Cc), NAN, device="cuda").bfloat16()
    p = L.AttnFusedParams(x=xd.data_ptr(), B=B, N=N, C=Cc, nseg=nseg, wqkv=wq16.data_ptr(), t1=ops.t1.data_ptr(), t2=ops.t2.data_ptr(),
                          gn_ab=L.ptr(gn_ab), label_q=L.ptr(ops.lq), lq_stride=128, scale=32 ** -0.5, part=part.data_ptr(),
                          ctx=ctx.data_ptr(), wout_perm=wo16.data_ptr(), bias_out=ops.bo.data_ptr(), y=y.data_ptr(), stats_part=None)
    if gpart is not None:
        set_part(p, gpart, case.count)
    mf = torch.empty(B * Cc * 128, dtype=torch.bfloat16, device="cuda") if v2 else None
    p.mfold = L.ptr(mf)
    p.gen = 2 if v2 else 1
    sp = torch.zeros(B, L.load().ds_attn_fused_stats_parts(C.byref(p)), 2, device="cuda")
    p.stats_part = sp.data_ptr()
    L.call("ds_attn_fused_context", C.byref(p), st)
    L.call("ds_attn_fused_output", C.byref(p), st)
    H().sync()
    return y, sp


@pytest.mark.parametrize("Cc,hw,cond", R.ATTN, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_attn_fused_from_partials(Cc, hw, cond):
    """ds_attn_fused_context / _output, first and second generation (attn_fused.hip, attn_out2.hpp): BOTH passes reduce the PreNorm's
    partials — the context pass for k and v, the output pass for q.  Whole block against the float64 oracle with the contract's
    statistics at the tolerance of test_fused_attention_block_matches_oracle."""
    case = R.attn_case("bf16", Cc, hw, cond)
    h = H()
    ops = AttnOperands(case)
    xd = h.to_nhwc(case.x, L.DS_BF16)
    wq16 = torch.empty(384 * Cc, dtype=torch.bfloat16, device="cuda")
    wo16 = torch.empty(Cc * 128, dtype=torch.bfloat16, device="cuda")
    L.call("ds_pack_attn_fused", ops.wq.data_ptr(), ops.g.data_ptr(), ops.wo.data_ptr(), wq16.data_ptr(), wo16.data_ptr(), Cc, L.current_stream())
    N = hw[0] * hw[1]
    for v2 in (False, True):
        for parts in case.parts:
            gpart, ab = device_partials(case, parts)
            y, sp = run_attn_fused(case, ops, xd, (wq16, wo16), 3, v2, gpart=gpart)
            out = output_norm(y, xd, ops, sp, case.B, N, Cc, L.DS_BF16)
            check(h.from_nhwc(out), case.ref(ab), case.tol, (case.id, v2, parts))
            y2, sp2 = run_attn_fused(case, ops, xd, (wq16, wo16), 3, v2, gn_ab=finalize(gpart, case.count))
            assert torch.equal(bits(y), bits(y2)) and torch.equal(bits(sp), bits(sp2)), (case.id, v2, parts)


def run_attn_x3(case, ops, xd, whl, nseg, gpart=None, gn_ab=None):
    lib = L.load()
    B, Cc, N = case.B, case.C, case.hw[0] * case.hw[1]
    st = L.current_stream()
    part = torch.empty(lib.ds_linattn_part_floats(B, 4, nseg), device="cuda")
    ctx = torch.empty(B * 4 * 1024, device="cuda")
    qpl = torch.empty(lib.ds_attn_x3_qplane_bytes(B, N), dtype=torch.uint8, device="cuda")
    mf = torch.empty(lib.ds_attn_x3_mfold_bytes(B, Cc), dtype=torch.uint8, device="cuda")
    y = torch.full((B, case.hw[0], case.hw[1], Cc), NAN, device="cuda")
    p = L.AttnX3Params(x=xd.data_ptr(), B=B, N=N, C=Cc, nseg=nseg, wqkv_hl=whl.data_ptr(), t1=ops.t1.data_ptr(), t2=ops.t2.data_ptr(),
                       gn_ab=L.ptr(gn_ab), label_q=L.ptr(ops.lq), lq_stride=128, scale=32 ** -0.5, part=part.data_ptr(),
                       ctx=ctx.data_ptr(), qplanes=qpl.data_ptr(), mfold=mf.data_ptr(), wout=ops.wo.data_ptr(), bias_out=ops.bo.data_ptr(),
                       y=y.data_ptr(), stats_part=None)
    if gpart is not None:
        set_part(p, gpart, case.count)
    sp = torch.zeros(B, lib.ds_attn_x3_stats_parts(C.byref(p)), 2, device="cuda")
    p.stats_part = sp.data_ptr()
    L.call("ds_attn_x3_context", C.byref(p), st)
    L.call("ds_attn_x3_output", C.byref(p), st)
    H().sync()
    return y, sp


@pytest.mark.parametrize("Cc,hw,cond", R.ATTN, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_attn_x3_from_partials(Cc, hw, cond):
    """ds_attn_x3_context / _output (split precision, fp32 tensors): the context pass reduces the partials for all three projections, the
    output pass (form A) does not normalise x again; against the float64 oracle at the 2e-5 of test_attn_x3_block_matches_oracle, with that
    test's assertion on the partials of y."""
    case = R.attn_case("x3", Cc, hw, cond)
    h = H()
    lib = L.load()
    ops = AttnOperands(case)
    xd = h.to_nhwc(case.x, L.DS_F32)
    whl = torch.empty(2 * 384 * Cc, dtype=torch.bfloat16, device="cuda")
    L.call("ds_pack_attn_x3", ops.wq.data_ptr(), ops.g.data_ptr(), whl.data_ptr(), Cc, L.current_stream())
    B, N = case.B, hw[0] * hw[1]
    for nseg in sorted({3, lib.ds_attn_x3_segments(B, N, Cc)}):
        for parts in case.parts:
            gpart, ab = device_partials(case, parts)
            y, sp = run_attn_x3(case, ops, xd, whl, nseg, gpart=gpart)
            assert torch.isfinite(y).all()
            s, yd = sp.double().sum(1).cpu(), y.double().cpu().reshape(B, -1)
            assert torch.allclose(s[:, 0], yd.sum(1), rtol=1e-5, atol=1e-2) and torch.allclose(s[:, 1], (yd * yd).sum(1), rtol=1e-5)
            out = output_norm(y, xd, ops, sp, B, N, Cc, L.DS_F32)
            check(h.from_nhwc(out), case.ref(ab), case.tol, (case.id, nseg, parts))
            y2, sp2 = run_attn_x3(case, ops, xd, whl, nseg, gn_ab=finalize(gpart, case.count))
            assert torch.equal(bits(y), bits(y2)) and torch.equal(bits(sp), bits(sp2)), (case.id, nseg, parts)


# ================================================================================================ part B: the depthwise producers
class DwOperands:
    """ds_dwconv7 on B = 3 distinct samples: one or two sources (the second one pixel / three pixels short: pad offsets (1, 3) // 2), bias
    and a time bias read at an offset inside a wider row, as test_dwconv7_two_source_time_bias_stats."""

    def __init__(self, tag, dt, c01, hw, wexp=False):
        h = H()
        self.dt, (self.c0, self.c1), (self.Hh, self.Ww) = dt, c01, hw
        self.B, self.Cc = 3, c01[0] + c01[1]
        B, Cc, Hh, Ww = self.B, self.Cc, self.Hh, self.Ww
        enc = R.distinct_samples("gp_dw_e%s%s%s" % (tag, c01, hw), (B, self.c0, Hh, Ww))
        self.w = synth_w = R.synth_input("gp_dw_w%d" % Cc, (Cc, 1, 7, 7), 0.2)
        self.b = R.synth_input("gp_dw_b%d" % Cc, (Cc,))
        self.tb = R.synth_input("gp_dw_tb%d" % Cc, (B, Cc + 12))
        self.x0 = h.to_nhwc(enc, dt)
        cat = h.from_nhwc(self.x0)
        self.x1 = None
        if self.c1:
            dec = R.distinct_samples("gp_dw_d%s%s%s" % (tag, c01, hw), (B, self.c1, Hh - 1, Ww - 3))
            self.x1 = h.to_nhwc(dec, dt)
            cat = torch.cat([cat, F.pad(h.from_nhwc(self.x1), (1, 2, 0, 1))], 1)            # offsets (1 // 2, 3 // 2) = (0, 1)
        wref = R.bf16r(synth_w) if wexp else synth_w                                         # the matrix-core path holds the taps in bf16
        self.want = F.conv2d(cat.double(), wref.double(), self.b.double(), padding=3, groups=Cc) + self.tb[:, 5:5 + Cc, None, None].double()
        wd = self.w.contiguous().cuda()
        self.wt = torch.empty(49 * Cc, device="cuda")
        L.call("ds_pack_dw_weight", wd.data_ptr(), Cc, self.wt.data_ptr(), L.current_stream())
        self.we = None
        if wexp:
            self.we = torch.empty(Cc * 6 * 64 * 8, dtype=torch.bfloat16, device="cuda")
            L.call("ds_pack_dw_weight_mfma", wd.data_ptr(), Cc, self.we.data_ptr(), L.current_stream())
        self.bd, self.tbd = self.b.cuda(), self.tb.cuda().contiguous()
        h.sync()

    def params(self, out, out_split=0, strip=0):
        return L.DwconvParams(src0=self.x0.data_ptr(), src1=L.ptr(self.x1), C0=self.c0, C1=self.c1, H=self.Hh, W=self.Ww,
                              H1=(self.Hh - 1 if self.c1 else 0), W1=(self.Ww - 3 if self.c1 else 0), off_h1=0, off_w1=1, wt=self.wt.data_ptr(),
                              bias=self.bd.data_ptr(), tbias=self.tbd.data_ptr() + 4 * 5, tb_stride=self.Cc + 12, out=out.data_ptr(),
                              stats_part=None, B=self.B, dtype=self.dt, wexp=L.ptr(self.we), out_split=out_split, strip=strip)

    def run(self, out_split=0, strip=0):
        """Returns (family name, partials per sample, stored result as NHWC fp32 [hi + lo for planes], raw output, partials)."""
        lib = L.load()
        if out_split:
            out = torch.full((self.B, self.Hh, self.Ww, 2 * self.Cc), NAN, device="cuda").bfloat16()
        else:
            out = torch.full((self.B, self.Hh, self.Ww, self.Cc), NAN, device="cuda").to(H().TDT[self.dt])
        p = self.params(out, out_split, strip)
        fam, rng, spc = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        L.call("ds_dwconv_launch_choice", C.byref(p), C.byref(fam), C.byref(rng), C.byref(spc))
        parts = lib.ds_dwconv_stats_parts(C.byref(p))
        st = torch.zeros(self.B, parts, 2, device="cuda")
        p.stats_part = st.data_ptr()
        L.call("ds_dwconv7", C.byref(p), L.current_stream())
        H().sync()
        val = out.float()
        if out_split:
            val = val[..., :self.Cc] + val[..., self.Cc:]
        return L.DW_FAMILY[fam.value], parts, val, out, st

    def check(self, val, st, what):
        """The assertions of test_dwconv7_two_source_time_bias_stats: the result against F.conv2d in float64, ds_gn_finalize of the partials
        against the float64 statistics."""
        h = H()
        bf = self.dt == L.DS_BF16
        assert torch.isfinite(val).all(), what
        err = rel_err(h.from_nhwc(val), self.want)
        assert err < (1e-2 if bf else 1e-5), (what, err)
        ab = finalize(st, self.Cc * self.Hh * self.Ww)
        h.sync()
        np.testing.assert_allclose(ab.cpu(), R.ab_direct(self.want).float(), rtol=2e-3 if bf else 1e-5, atol=1e-4 if bf else 1e-6)


def ceil_div(a, b):
    return -(-a // b)


# (tag, dtype, (C0, C1), (H, W), matrix-core weights, out_split, strip, family, (tile rows, tile columns, channels per block) or None)
# Tile kernels (dwconv7.hip: a block holds 2048 / NV pixels of NV channel vectors; columns 8 / 16 / 32 by lt_twl): bf16 and fp32 NV = 4
# 512 pixels = 64 x 8 (W <= 8), 32 x 16 (W <= 16), 16 x 32; fp32 NV = 8 256 pixels = 32 x 8 (W <= 8), 16 x 16.
DW_ROWS = [("direct", L.DS_BF16, (40, 0), (10, 9), False, 0, 0, "direct", None),
           ("direct", L.DS_F32, (20, 0), (10, 9), False, 0, 0, "direct", None),
           ("direct", L.DS_BF16, (24, 40), (10, 9), False, 0, 0, "direct", None),              # (the direct kernel's second-source branch)
           ("direct", L.DS_F32, (12, 20), (10, 9), False, 0, 0, "direct", None)]
for _w, _tile in ((7, (64, 8)), (12, (32, 16)), (40, (16, 32))):
    DW_ROWS.append(("tile", L.DS_BF16, (32, 64), (19, _w), False, 0, 0, "tile", _tile + (32,)))
    DW_ROWS.append(("tile", L.DS_F32, (48, 0), (19, _w), False, 0, 0, "tile", _tile + (16,)))
    DW_ROWS.append(("tile", L.DS_F32, (16, 32), (19, _w), False, 0, 0, "tile", _tile + (16,)))
for _hw, _tile in (((16, 8), (32, 8)), ((19, 24), (16, 16))):
    for _split in (0, 1):
        DW_ROWS.append(("tile8", L.DS_F32, (96, 0), _hw, False, _split, 0, "tile", _tile + (32,)))
DW_ROWS += [("strip", L.DS_F32, (96, 0), (64, 16), False, 1, 1, "strip", None), ("strip", L.DS_F32, (32, 64), (70, 37), False, 1, 1, "strip", None),
            ("mfma", L.DS_BF16, (96, 192), (40, 16), True, 0, 0, "mfma", None), ("mfma", L.DS_BF16, (96, 192), (37, 70), True, 0, 0, "mfma", None)]


@pytest.mark.parametrize("row", DW_ROWS, ids=lambda r: "%s_%s_%d+%d_%dx%d%s" % (r[0], "bf16" if r[1] else "f32", r[2][0], r[2][1], r[3][0], r[3][1], "_split" if r[5] else ""))
def test_dwconv7_family_matrix(row):
    """Every family ds_dwconv7 dispatches to and every instantiation of its tile kernel, named by ds_dwconv_launch_choice and (tile
    kernels) by the number of partials their tile size implies: direct kernel (channel counts no tile takes), bf16 and fp32 NV = 4 tiles
    8 / 16 / 32 columns wide, fp32 NV = 8 tiles (8 and 16 columns, fp32 and hi / lo plane output), strip kernel, both matrix-core forms."""
    tag, dt, c01, hw, wexp, split, strip, family, tile = row
    ops = DwOperands(tag, dt, c01, hw, wexp)
    fam, parts, val, _, st = ops.run(split, strip)
    assert fam == family, (fam, family)
    if tile is not None:
        th, tw, cb = tile
        assert parts == ceil_div(hw[0], th) * ceil_div(hw[1], tw) * ((c01[0] + c01[1]) // cb), (parts, tile)
    ops.check(val, st, row[:4])


# ================================================================================================ part B: producer -> consumer chains
def drift(st, stored_nhwc, count, what):
    """Statistics from the producer's fp32 partials against the float64 statistics of the tensor it stored (reported, not asserted: the
    engine-level tolerances rest on it).  Returns the direct float64 statistics."""
    direct = R.ab_direct(stored_nhwc)
    fromp = R.ab_from_partials(st.cpu(), count)
    d = ((fromp - direct).abs() / direct.abs()).max(0).values
    note("chain %-44s partials-vs-direct statistics drift: rstd %.2e, rstd*mean %.2e (%d partials)" % (what, d[0].item(), d[1].item(), st.shape[1]))
    return direct


def chain_weights(tag, c_in, c_mid):
    w1 = R.synth_input("gp_ch_w1%s" % tag, (c_mid, c_in, 3, 3), 0.05)
    w2 = R.synth_input("gp_ch_w2%s" % tag, (c_in, c_mid, 3, 3), 0.05)
    b1, b2 = R.synth_input("gp_ch_b1%s" % tag, (c_mid,)), R.synth_input("gp_ch_b2%s" % tag, (c_in,))
    g1, be1 = 1 + 0.2 * R.synth_input("gp_ch_g1%s" % tag, (c_in,)), 0.3 * R.synth_input("gp_ch_be1%s" % tag, (c_in,))
    g2, be2 = 1 + 0.2 * R.synth_input("gp_ch_g2%s" % tag, (c_mid,)), 0.3 * R.synth_input("gp_ch_be2%s" % tag, (c_mid,))
    return (w1, b1, g1, be1), (w2, b2, g2, be2)


def conv_ref(stored_nhwc, ab, w, b, g, be, gelu, res_nchw=None):
    y = F.conv2d(R.gn(stored_nhwc.permute(0, 3, 1, 2), ab, g, be), w.double(), b.double(), padding=1)
    y = F.gelu(y) if gelu else y
    return y + res_nchw.double() if res_nchw is not None else y


@pytest.mark.parametrize("hw,strip", [((16, 8), 0), ((19, 24), 0), ((64, 16), 1)], ids=["16x8_tile_pair", "19x24_tile", "64x16_strip"])
def test_chain_dwconv_split_halo_x3(hw, strip):
    """A ConvNeXt block of the split-precision tier without ds_gn_finalize: fp32 depthwise (tile kernel; strip kernel where forced: another
    partial count) writing hi / lo planes -> 3x3 (flags 1|2, GELU, statistics) -> 3x3 (flags 1|4 + residual).  Each producer's stats_part
    pointer and ds_*_stats_parts count are the consumer's gn_part / gn_parts; each consumer is held, at its own 3e-5, to the float64
    operation on the producer's STORED output."""
    B, Cc, Cm, (Hh, Ww) = 3, 96, 192, hw
    dw = DwOperands("chain", L.DS_F32, (Cc, 0), hw)
    fam, parts0, val0, planes0, st0 = dw.run(out_split=1, strip=strip)
    assert fam == ("strip" if strip else "tile")
    dw.check(val0, st0, ("chain dw", hw))
    (w1, b1, g1, be1), (w2, b2, g2, be2) = chain_weights("x3", Cc, Cm)
    c1, c2 = X3Conv(w1, b1, g1, be1), X3Conv(w2, b2, g2, be2)
    count0, count1 = Cc * Hh * Ww, Cm * Hh * Ww
    ab0 = drift(st0, val0.cpu(), count0, "%s dw -> conv1 (x3) %dx%d" % (fam, Hh, Ww))
    got1, planes1, st1 = c1.run(planes0, B, Hh, Ww, True, True, gpart=st0, count=count0)
    check(got1, conv_ref(val0.cpu(), ab0, w1, b1, g1, be1, True), 3e-5, ("chain conv1", hw))
    val1 = (planes1.float()[..., :Cm] + planes1.float()[..., Cm:]).cpu()
    ab1 = drift(st1, val1, count1, "conv1 -> conv2 (x3) %dx%d" % (Hh, Ww))
    r = R.synth_input("gp_ch_r%s" % (hw,), (B, Cc, Hh, Ww))
    got2, _, _ = c2.run(planes1, B, Hh, Ww, False, False, rd=R.nhwc(r).cuda(), gpart=st1, count=count1)
    check(got2, conv_ref(val1, ab1, w2, b2, g2, be2, False, r), 3e-5, ("chain conv2", hw))
    # ... and the same conv1 as three K slices (what the engine runs at small batches): ds_conv_splitk_reduce reduces st0
    got1k, _, _ = c1.run(planes0, B, Hh, Ww, True, True, ks=3, gpart=st0, count=count0)
    check(got1k, conv_ref(val0.cpu(), ab0, w1, b1, g1, be1, True), 3e-5, ("chain conv1 split-K", hw))


def test_chain_dwconv_mfma_halo_bf16():
    """The same block in the bf16 tier at (3,96,37,70): matrix-core depthwise -> bf16 halo 3x3 (GELU, statistics) -> bf16 halo 3x3 +
    residual, partials handed on raw; consumers at the bf16 tolerance 2e-2 against the float64 operation on the stored producer output."""
    h = H()
    dt = L.DS_BF16
    B, Cc, Cm, (Hh, Ww) = 3, 96, 192, (37, 70)
    dw = DwOperands("chainb", dt, (Cc, 0), (Hh, Ww), wexp=True)
    fam, parts0, val0, out0, st0 = dw.run()
    assert fam == "mfma"
    dw.check(val0, st0, "chain mfma dw")
    (w1, b1, g1, be1), (w2, b2, g2, be2) = chain_weights("bf", Cc, Cm)
    p1 = h.PackedConv(w1, b1, dt, L.TILE_HALO3_256x96, gamma=g1, beta=be1)
    p2 = h.PackedConv(w2, b2, dt, L.TILE_HALO3_256x96, gamma=g2, beta=be2)
    count0, count1 = Cc * Hh * Ww, Cm * Hh * Ww
    ab0 = drift(st0, val0.cpu(), count0, "mfma dw -> conv1 (bf16) 37x70")
    y1, st1 = h.run_conv(p1, out0, pad=1, gn_part=(st0, parts0, count0, R.EPS), act=L.ACT_GELU, want_stats=True)
    check(h.from_nhwc(y1), conv_ref(val0.cpu(), ab0, w1, b1, g1, be1, True), 2e-2, "chain bf16 conv1")
    val1 = y1.float().cpu()
    ab1 = drift(st1, val1, count1, "conv1 -> conv2 (bf16) 37x70")
    rd = h.to_nhwc(R.synth_input("gp_ch_rb", (B, Cc, Hh, Ww)), dt)
    y2, _ = h.run_conv(p2, y1, pad=1, gn_part=(st1, st1.shape[1], count1, R.EPS), res=rd)
    check(h.from_nhwc(y2), conv_ref(val1, ab1, w2, b2, g2, be2, False, h.from_nhwc(rd)), 2e-2, "chain bf16 conv2")


@pytest.mark.parametrize("Cc,hw,cond", R.ATTN[:2], ids=["96_5x10", "192_33x32"])
def test_chain_attn_output_gn_apply_fast(Cc, hw, cond):
    """What the bf16 engine runs behind an attention block: ds_attn_fused_output's partials of y straight into ds_gn_apply's fast form
    with res = x (no ds_gn_finalize), against GroupNorm of the STORED y in float64 at ds_gn_apply's 1e-2."""
    case = R.attn_case("bf16", Cc, hw, cond)
    h = H()
    ops = AttnOperands(case)
    xd = h.to_nhwc(case.x, L.DS_BF16)
    wq16 = torch.empty(384 * Cc, dtype=torch.bfloat16, device="cuda")
    wo16 = torch.empty(Cc * 128, dtype=torch.bfloat16, device="cuda")
    L.call("ds_pack_attn_fused", ops.wq.data_ptr(), ops.g.data_ptr(), ops.wo.data_ptr(), wq16.data_ptr(), wo16.data_ptr(), Cc, L.current_stream())
    B, N = case.B, hw[0] * hw[1]
    gpart, _ = device_partials(case, 65)
    for v2 in (False, True):
        y, sp = run_attn_fused(case, ops, xd, (wq16, wo16), 3, v2, gpart=gpart)
        ys = y.float().cpu()
        aby = drift(sp, ys, Cc * N, "attn_fused_output gen %d -> gn_apply fast C=%d %dx%d" % (2 if v2 else 1, Cc, hw[0], hw[1]))
        out = torch.full_like(y, NAN)
        gp = L.GnApplyParams(x=y.data_ptr(), res=xd.data_ptr(), out=out.data_ptr(), gn_ab=None, gamma=ops.go.data_ptr(), beta=ops.bo2.data_ptr(),
                             cbias=None, cb_stride=0, B=B, HW=N, C=Cc, G=1, act=L.ACT_NONE, dtype=L.DS_BF16)
        gp.gn_part, gp.gn_parts, gp.gn_count, gp.gn_eps = sp.data_ptr(), sp.shape[1], float(Cc * N), 1e-5
        L.call("ds_gn_apply", C.byref(gp), L.current_stream())
        h.sync()
        sd, tag = case.sd, case.tag
        want = R.gn(ys.permute(0, 3, 1, 2), aby, sd[tag + ".fn.fn.to_out.1.weight"], sd[tag + ".fn.fn.to_out.1.bias"]) + case.x.double()
        check(h.from_nhwc(out), want, 1e-2, (case.id, v2))
