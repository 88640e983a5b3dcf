"""The two plain linear-attention files on every path their launchers take, through the C ABI: csrc/linattn.hip (ds_linattn_context,
ds_linattn_output: the fp32 tier of the U-Net and of the VQGAN, and attn_ctx_combine, which merges the partials of every fused attention
kernel too) and csrc/vq_attn.hip (ds_vq_attn_context, ds_vq_attn_output: the bf16 decoder / encoder attention).

Exact cases (tests/linattn_ref.py says why they are exact, tests/test_linattn_ref_cpu.py proves it without a GPU and shows that every defect
model changes what a case here compares): torch.equal against the float64 reference rounded once.  No tolerance.  The shapes are the
smallest that reach each path; tests/test_linattn_ref_cpu.py asserts by the path predicates that they do.

  attn_ctx_partial<T>    segment lengths 1, R - 1, R, R + 1, 63, 64, 65, 4R - 1, 4R, 4R + 1, 8R + 1 (R = 32 fp32, 64 bf16 rows per load), a ragged
                         last segment, empty segments (N = 10 in 7), heads 1, 4, 8, B 1, 3
  attn_ctx_combine       nseg 1, 31, 32, 33, 64, 65 at N = 130, segments without a zero key, the token absent / dominating / negligible, label
                         strides of heads * 32 + 8 with NaN in the gap
  attn_out_kernel<T>     N 1, 63, 64, 65, 255, 256, 257, 513, heads 1, 4, 7, 8, q_softmax 0 and 1 (scale 0.25), label_q NULL and strided
  vq_attn_ctx/fold/apply C 80 and 160, N 1 .. 657, nseg from ds_vq_attn_segments and by hand (one block over six groups, blocks of 3 + 2
                         groups, an empty block, one block per group), wnin and stats_ws NULL and set; wfold, part, ctx, stats_ws prefilled
                         with NaN; wfold rows >= C are +0, an empty block's statistics are 0, every slot holds the exact sums of the stored y

Random-data cases hold what exact data cannot (scale = 32 ** -0.5, generic softmax weights, a y that rounds).  Their error is taken PER
ROW and scaled by the row's own L-infinity norm (linattn_ref.row_errors): a fault confined to one pixel row is as large as in a tensor of
that row alone.  fp32 linattn follows the measured rule of tests/test_hip_timbre.py: no row of the device may lie further from float64
than four times the worst row of the fp32 restatement (the kernel's own segment order in torch fp32) - rounding errors of two summation
orders are not correlated row by row, so the restatement's worst row is the extent of the distribution every row's error is drawn from.
The bf16 kernels keep the tolerances of the existing tests (1e-2 on out / y, 6e-3 on the vq context), now per row; W_b, which no test
bounded, gets the one bf16 rounding it is stored with (2^-8 of the row's largest).  The bf16 restatement (P and V rounded to bf16 as the
matrix cores take them, W_b and y rounded once) is recorded beside each and lies inside them: no per-row bound had to be widened.
No bound is taken from a kernel's output.  Every input and output lives in a NaN-guarded slab; the guards are checked after every case.
Figures are printed, and appended to $DS_LINATTN_PARITY_LOG when that is set (profiles/linattn_paths_parity.txt keeps one green run's)."""
import ctypes as C
import os

import pytest
import torch

import exact_ref as E
import linattn_ref as R
import support_ref as S
from diffusynth_amd import _lib as L

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def note(line):
    print(line)
    path = os.environ.get("DS_LINATTN_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def sync():
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def unchanged(view, src):
    assert torch.equal(bits(view).cpu(), bits(src.to(view.dtype)))


# ================================================================================================= linattn
def _run_linattn(c, out=True):
    """ds_linattn_context (+ ds_linattn_output) on case c; returns (ctx fp32 cpu, out cpu or None)."""
    lib = L.load()
    dt = BF if c.bf16 else torch.float32
    qkv_c = R.linattn_qkv(c)
    qkv = S.slab(qkv_c)
    part = S.nan_slab((lib.ds_linattn_part_floats(c.B, c.heads, c.nseg),))
    ctx = S.nan_slab((c.B, c.heads, 32, 32))
    o = S.nan_slab((c.B, c.N, c.HD), dt)
    lab = {n: (S.slab(getattr(c, n + "_full").float()) if getattr(c, n + "_full") is not None else None) for n in ("lk", "lv", "lqv")}
    p = L.AttnParams(qkv=qkv.data_ptr(), B=c.B, N=c.N, heads=c.heads, dtype=L.DS_BF16 if c.bf16 else L.DS_F32, nseg=c.nseg, part=part.data_ptr(),
                     ctx=ctx.data_ptr(), label_q=L.ptr(lab["lqv"]), label_k=L.ptr(lab["lk"]), label_v=L.ptr(lab["lv"]), lq_stride=c.stride,
                     lk_stride=c.stride, lv_stride=c.stride, q_softmax=c.q_softmax, scale=c.scale, out=o.data_ptr())
    st = L.current_stream()
    L.call("ds_linattn_context", C.byref(p), st)
    if out:
        L.call("ds_linattn_output", C.byref(p), st)
    sync()
    views = [qkv, part, ctx, o] + [t for t in lab.values() if t is not None]
    S.check_guards(*views)
    unchanged(qkv, qkv_c)
    for n, t in lab.items():
        if t is not None:
            unchanged(t, getattr(c, n + "_full").float())
    assert bool(torch.isfinite(part.view(-1, R.PARTF)[:, 32:]).all()), "every partial is written (an empty segment: sum 0, context 0)"
    if not out:
        assert bool(torch.isnan(o.float()).all())
    return ctx.cpu(), (o.cpu() if out else None)


@pytest.mark.parametrize("a", R.linattn_args(), ids=lambda a: R.linattn_case(**a).id)
def test_linattn_exact(a):
    c = R.linattn_case(**a)
    ctx, out = _run_linattn(c)
    paths = sorted(p for p in R.seg_paths(c.N, c.nseg, c.bf16) if not p.startswith("len")) + sorted(R.out_paths(c.N, c.bf16))
    E.assert_bits_equal(ctx, c.want_ctx, "ds_linattn_context " + c.id)
    E.assert_bits_equal(out, c.want_out, "ds_linattn_output " + c.id)
    note("linattn exact %s: ctx and out equal to float64 bit for bit; out margin %.4g of 2^24; paths %s" % (c.id, c.out_margin, " ".join(paths)))


def _rows_rule(what, dev, twin, f64, tol=None):
    """Per row.  tol None (fp32): no row of dev further from f64 than 4 x the worst row of twin.  tol given (bf16): no row further than tol, the
    tolerance of the existing test or of the number format; the restatement's worst row is recorded beside it and must itself stay inside."""
    assert tuple(dev.shape) == tuple(f64.shape) == tuple(twin.shape) and bool(torch.isfinite(dev.float()).all()), what
    e_dev, e_twin = R.row_errors(dev, f64), R.row_errors(twin, f64)
    worst, yard = e_dev.max().item(), e_twin.max().item()
    bound = 4 * yard if tol is None else tol
    note("%s: worst row of the device vs float64 %.3e (row %d of %d), worst row of the restatement %.3e, bound %.3e" %
         (what, worst, int(e_dev.argmax()), e_dev.numel(), yard, bound))
    assert 0 < yard <= bound and worst <= bound, (what, worst, yard, bound)


@pytest.mark.parametrize("a", R.LINATTN_RANDOM, ids=lambda a: "_".join(map(str, a)))
def test_linattn_random_rows(a):
    c = R.linattn_random_case(*a)
    ctx, out = _run_linattn(c)
    ctx64 = R.linattn_ctx_walk(c, nseg=1, dtype=torch.float64)
    ctx32 = R.linattn_ctx_walk(c)
    _rows_rule("ds_linattn_context %s ctx" % c.id, ctx, ctx32, ctx64)
    # pass 2 on the context the device stored: its own error, not pass 1's again
    out64 = R.linattn_out_walk(c, ctx, dtype=torch.float64)
    out32 = R.linattn_out_walk(c, ctx)
    if c.bf16:
        _rows_rule("ds_linattn_output %s out" % c.id, out, out32.bfloat16(), out64, tol=1e-2)
    else:
        _rows_rule("ds_linattn_output %s out" % c.id, out, out32, out64)


def test_linattn_refusals():
    """heads = 9 and nseg = N + 1 are refused before anything is launched (the limits the header states)."""
    c = R.linattn_case(False, 1, 2, 1, 2)
    qkv = S.slab(R.linattn_qkv(c))
    part, ctx, o = S.nan_slab((9 * 3 * R.PARTF,)), S.nan_slab((9, 32, 32)), S.nan_slab((1, 2, 32))
    for heads, nseg in ((9, 1), (1, 3)):
        p = L.AttnParams(qkv=qkv.data_ptr(), B=1, N=2, heads=heads, dtype=L.DS_F32, nseg=nseg, part=part.data_ptr(), ctx=ctx.data_ptr(), lq_stride=32,
                         lk_stride=32, lv_stride=32, q_softmax=0, scale=1.0, out=o.data_ptr())
        for fn in ("ds_linattn_context", "ds_linattn_output"):
            with pytest.raises(L.DsError):
                L.call(fn, C.byref(p), L.current_stream())
    sync()
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(ctx).all()) and bool(torch.isnan(o).all())
    S.check_guards(qkv, part, ctx, o)


# ================================================================================================= vq_attn
def _run_vq(c, nseg, with_stats):
    """ds_vq_attn_context + ds_vq_attn_output; returns (ctx, wfold [B][CP][C] bf16, y [B][N][C] bf16, stats [B][nseg / 4][C][2] or None) on the cpu."""
    lib = L.load()
    srcs = {"x": c.x.float().bfloat16(), "wqkv": c.wqkv.float().bfloat16(), "wq": c.wq.float(), "wout": c.wout.float(), "bias": c.bias.float(),
            "wnin": c.wnin.float() if c.wnin is not None else None}
    d = {n: (S.slab(t) if t is not None else None) for n, t in srcs.items()}
    assert lib.ds_vq_attn_wfold_bytes(c.B, c.C) == c.B * c.CP * c.C * 2
    part = S.nan_slab((lib.ds_linattn_part_floats(c.B, 1, nseg),))
    ctx, wfold, y = S.nan_slab((c.B, 32, 32)), S.nan_slab((c.B, c.CP, c.C), BF), S.nan_slab((c.B, c.N, c.C), BF)
    ws = S.nan_slab((c.B, nseg // 4, c.C, 2)) if with_stats else None
    p = L.VqAttnParams(x=d["x"].data_ptr(), B=c.B, N=c.N, C=c.C, nseg=nseg, wqkv=d["wqkv"].data_ptr(), wq=d["wq"].data_ptr(), wout=d["wout"].data_ptr(),
                       wnin=L.ptr(d["wnin"]), bias=d["bias"].data_ptr(), part=part.data_ptr(), ctx=ctx.data_ptr(), wfold=wfold.data_ptr(), y=y.data_ptr(),
                       stats_ws=L.ptr(ws))
    st = L.current_stream()
    L.call("ds_vq_attn_context", C.byref(p), st)
    L.call("ds_vq_attn_output", C.byref(p), st)
    sync()
    S.check_guards(*([t for t in d.values() if t is not None] + [part, ctx, wfold, y] + ([ws] if with_stats else [])))
    for n, t in srcs.items():
        if t is not None:
            unchanged(d[n], t)
    pc = part.cpu().view(c.B, nseg, R.PARTF)
    assert bool(torch.isfinite(pc[:, :, 32:]).all()) and not bool(torch.isnan(pc).any()), "every wave writes its partial (no tile: max -inf, sum 0, context 0)"
    wf = wfold.cpu()
    assert not bool(bits(wf[:, c.C:]).any()), "the rows [C, roundup(C, 32)) of wfold are +0"
    return ctx.cpu(), wf, y.cpu(), (ws.cpu() if with_stats else None)


def _vq_id(a):
    return "C%d_B%d_N%d_%s_s%d_%s" % (a[0], a[1], a[2], "skip" if a[3] else "noskip", a[4], "stats" if a[5] else "nostats")


def test_vq_attn_segments_rule():
    lib = L.load()
    for Cc in (80, 160):
        for B in (1, 2, 8, 9, 64, 128, 600):
            for N in range(1, 701):
                assert lib.ds_vq_attn_segments(B, N, Cc) == R.vq_segments_rule(B, N, Cc), (B, N, Cc)


@pytest.mark.parametrize("a", R.vq_args(), ids=_vq_id)
def test_vq_attn_exact(a):
    Cc, B, N, skip, nseg, with_stats = a
    c = R.vq_case(Cc, B, N, skip)
    if nseg == R.vq_segments_rule(B, N, Cc):
        assert L.load().ds_vq_attn_segments(B, N, Cc) == nseg
    want = R.vq_expect(c, nseg)
    ctx, wfold, y, ws = _run_vq(c, nseg, with_stats)
    what = "ds_vq_attn " + _vq_id(a)
    E.assert_bits_equal(ctx, want.ctx, what + " ctx")
    E.assert_bits_equal(wfold, want.wfold, what + " wfold")
    E.assert_bits_equal(y, want.y, what + " y")
    if with_stats:
        E.assert_bits_equal(ws.double(), want.stats, what + " statistics slots")
        for i, (p0, p1) in enumerate(R.vq_block_pixels(N, nseg)):
            if p0 >= p1:
                assert not bool(bits(ws[:, i]).any()), "the slots of a block without a group are +0"
    note("vq_attn exact %s: ctx, wfold, y%s equal to float64 bit for bit; W_b entries over 8 bits %.3f, y margin %.4g of 2^24; paths %s" %
         (_vq_id(a), ", statistics" if with_stats else "", c.wide_share, c.y_margin, " ".join(sorted(R.vq_paths(N, nseg)))))


@pytest.mark.parametrize("a", R.VQ_RANDOM, ids=lambda a: "_".join(map(str, a)))
def test_vq_attn_random_rows(a):
    c = R.vq_random_case(*a)
    nseg = L.load().ds_vq_attn_segments(c.B, c.N, c.C)
    assert nseg == R.vq_segments_rule(c.B, c.N, c.C)
    ctx, wfold, y, ws = _run_vq(c, nseg, True)
    ctx64 = R.vq_ctx_walk(c, 4, dtype=torch.float64)
    ctxb = R.vq_ctx_walk(c, nseg, round_pv=True)
    _rows_rule("ds_vq_attn_context %s ctx" % c.id, ctx, ctxb, ctx64, tol=6e-3)
    # the output pass on the context the device stored
    _, y64 = R.vq_out_walk(c, ctx, nseg, dtype=torch.float64)                    # (rounded to bf16 once, as y is stored)
    wfb, yb = R.vq_out_walk(c, ctx, nseg)
    wb64 = torch.einsum("oe,bec->boc", c.wout, torch.einsum("bde,dc->bec", ctx.double(), c.wq)) + (c.wnin if c.wnin is not None else 0.0)
    _rows_rule("ds_vq_attn_output %s wfold" % c.id, wfold[:, :c.C], wfb[:, :c.C], wb64, tol=2.0 ** -8 * 1.001)   # one bf16 rounding: half an ulp of 8 bits at most, of the row's largest at most; 0.1 % for the fp32 fold in front
    ye = torch.einsum("boc,bnc->bno", wfold[:, :c.C].double(), c.x) + c.bias      # y from the W_b the device stored, before its own rounding
    _rows_rule("ds_vq_attn_output %s y" % c.id, y, ye.float().bfloat16(), ye, tol=1e-2)
    # the statistics: fp32 sums of the stored y in some order; n terms are off by at most n 2^-24 sum |.|
    yd = y.double()
    for i, (p0, p1) in enumerate(R.vq_block_pixels(c.N, nseg)):
        blk = yd[:, p0:p1]
        for j, t in enumerate((blk, blk * blk)):
            err = (ws[:, i, :, j].double() - t.sum(1)).abs()
            assert bool((err <= (p1 - p0) * 2.0 ** -24 * t.abs().sum(1)).all()), (c.id, i, j, err.max().item())
