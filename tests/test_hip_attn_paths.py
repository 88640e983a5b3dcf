"""The fused attention of both tiers on every path its launchers take, through the C ABI.  Split precision (csrc/attn_x3.hip: attn_x3_pass1<6,2>,
<12,2> + q-only <12,4>, <24,1> + q-only <24,2>, attn_x3_fold, attn_x3_qz<6> and attn_x3_z in modes 0, 1 + 2 (form B), out_planes with and
without out): the second half of this file.  The bf16 tier: ds_attn_fused_context / ds_attn_fused_output in
both kernel generations (csrc/attn_fused.hip: attn_fused_ctx<6,1>, <6,2>, <12,1>, <24,1>, attn_fused_out<..>; csrc/attn_out2.hpp:
attn_ctx2<6,4,4,1>, <12,8,4,1>, <24,8,2,2>, attn_fold_out, attn_out2<6,4>, <12,8>), attn_ctx_combine behind them, ds_pack_attn_fused,
ds_conv_fold_tables as attention calls it, and the launch-decision functions.

Exact cases only (tests/attn_ref.py says why they are exact; tests/test_attn_ref_cpu.py proves the preconditions without a GPU, shows that
the step-by-step restatement of every context form meets the float64 reference, and that every defect model changes what a case here
compares): the context buffer, M_b and y are compared bit for bit with float64 rounded once.  No tolerance on a tensor.  The (sum, sum of
squares) slots are compared bit for bit where the case keeps every partial sum an integer below 2^24 units ('small' cases); the 'wide'
cases, whose y really rounds, bound the summed slots by the fp32 rounding of that many additions.

Every input, scratch buffer and output lives in a NaN-guarded slab (support_ref.slab); guards and inputs are checked after every launch
pair.  Figures are printed, and appended to $DS_ATTN_PARITY_LOG when that is set (profiles/attn_paths_parity.txt keeps one green run's)."""
import ctypes as C
import os

import pytest
import torch

import attn_ref as R
import exact_ref as E
import support_ref as S
from diffusynth_amd import _lib as L

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def note(line):
    print(line)
    path = os.environ.get("DS_ATTN_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                               # a device fault: nothing more is started on this GPU by this session
        pytest.exit("device error after an attention launch: %s" % e, returncode=3)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def unchanged(view, src):
    assert torch.equal(bits(view).cpu(), bits(src.to(view.dtype)))


def wout_perm_ref(wout):
    """ds_pack_attn_fused's copy of to_out: inside each head's 32 columns, position s*16 + h*8 + j holds e = 16 s + 8 (j >> 2) + 4 h + (j & 3)."""
    pos = torch.arange(32)
    s, h, j = pos // 16, (pos // 8) % 2, pos % 8
    e = 16 * s + 8 * (j // 4) + 4 * h + (j % 4)
    C_ = wout.shape[0]
    return wout.view(C_, 4, 32)[:, :, e].reshape(C_, 128)


def mfold_ref(mb):
    """attn_fold_out's layout of M_b [B][C][4][32]: row m of a 32-channel block holds channel 16 ((m >> 2) & 1) + (m & 3) + 4 (m >> 3), column
    h*32 + s*16 + kg*8 + j holds d = 16 s + 8 (j >> 2) + 4 kg + (j & 3)."""
    B, C_ = mb.shape[:2]
    m = torch.arange(32)
    ch = 16 * ((m // 4) % 2) + (m % 4) + 4 * (m // 8)
    rows = (torch.arange(C_ // 32).view(-1, 1) * 32 + ch.view(1, -1)).flatten()
    pos = torch.arange(32)
    s, kg, j = pos // 16, (pos // 8) % 2, pos % 8
    d = 16 * s + 8 * (j // 4) + 4 * kg + (j % 4)
    return mb[:, rows][:, :, :, d].reshape(B, C_, 128)


_PACKED = {}


def packed(c):
    """Device operands of a case through ds_pack_attn_fused and ds_conv_fold_tables (bias NULL), each checked bit for bit, in guarded slabs."""
    key = c.id
    if key in _PACKED:
        return _PACKED[key]
    Cc = c.C
    src = {"wqkv": S.slab(c.wqkv.float()), "gamma": S.slab(c.gamma.float()), "beta": S.slab(c.beta.float()), "wout": S.slab(c.wout.float())}
    wq16, wo16 = S.nan_slab((384, Cc), BF), S.nan_slab((Cc, 128), BF)
    t1, t2 = S.nan_slab((384,)), S.nan_slab((384,))
    st = L.current_stream()
    L.call("ds_pack_attn_fused", src["wqkv"].data_ptr(), src["gamma"].data_ptr(), src["wout"].data_ptr(), wq16.data_ptr(), wo16.data_ptr(), Cc, st)
    L.call("ds_conv_fold_tables", src["wqkv"].data_ptr(), None, src["gamma"].data_ptr(), src["beta"].data_ptr(), 384, Cc, 1, 1, t1.data_ptr(),
           t2.data_ptr(), st)
    sync()
    S.check_guards(wq16, wo16, t1, t2, *src.values())
    E.assert_bits_equal(wq16.cpu(), E.rne_bf16(c.wpk), "ds_pack_attn_fused wqkv " + c.id)
    E.assert_bits_equal(wo16.cpu(), E.rne_bf16(wout_perm_ref(c.wout)), "ds_pack_attn_fused wout_perm " + c.id)
    E.assert_bits_equal(t1.cpu(), c.t1.float(), "ds_conv_fold_tables t1 " + c.id)
    E.assert_bits_equal(t2.cpu(), c.t2.float(), "ds_conv_fold_tables t2 " + c.id)
    d = dict(wq16=wq16, wo16=wo16, t1=t1, t2=t2, x=S.slab(c.x.float().bfloat16()), bias=S.slab(c.bias.float()),
             gn_ab=S.slab(E.gn_ab_tensor(c.a, c.mean)), label=S.slab(c.label_full.float()) if c.label_full is not None else None)
    part, count, eps = R.gn_partials(c)
    d["gn_part"], d["gn_count"], d["gn_eps"], d["gn_part_src"] = S.slab(part), count, eps, part
    _PACKED[key] = d
    return d


def launch(c, k, nseg, gen_ctx, gen_out, gn):
    """ds_attn_fused_context + ds_attn_fused_output.  Returns (ctx, y, stats [B][parts][2], mfold or None, parts, reported generations) on the cpu."""
    lib = L.load()
    d = packed(c)
    B, N, Cc = c.B, c.N, c.C
    part = S.nan_slab((lib.ds_linattn_part_floats(B, 4, nseg),))
    ctx, y = S.nan_slab((B, 4, 32, 32)), S.nan_slab((B, N, Cc), BF)
    mf = S.nan_slab((B, Cc, 128), BF) if k["mfold"] else None
    p = L.AttnFusedParams(x=d["x"].data_ptr(), B=B, N=N, C=Cc, nseg=nseg, wqkv=d["wq16"].data_ptr(), t1=d["t1"].data_ptr(), t2=d["t2"].data_ptr(),
                          label_q=L.ptr(d["label"]), lq_stride=c.lq_stride, scale=c.scale, part=part.data_ptr(), ctx=ctx.data_ptr(),
                          wout_perm=d["wo16"].data_ptr(), bias_out=d["bias"].data_ptr(), y=y.data_ptr(), stats_part=None, mfold=L.ptr(mf),
                          batch_hint=k["hint"])
    if gn == "ab":
        p.gn_ab = d["gn_ab"].data_ptr()
    else:
        p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = d["gn_part"].data_ptr(), d["gn_part_src"].shape[1], d["gn_count"], d["gn_eps"]
    p.gen = gen_out
    parts = lib.ds_attn_fused_stats_parts(C.byref(p))
    sp = S.nan_slab((B, parts, 2))
    p.stats_part = sp.data_ptr()
    st = L.current_stream()
    p.gen = gen_ctx
    g_ctx = lib.ds_attn_fused_generations(C.byref(p)) & 1
    L.call("ds_attn_fused_context", C.byref(p), st)
    sync()
    assert bool(torch.isnan(y.float()).all()) and bool(torch.isnan(sp).all()), "the context pass stores no output"
    ctx_after_pass1 = ctx.cpu()
    p.gen = gen_out
    g_out = lib.ds_attn_fused_generations(C.byref(p)) & 2
    L.call("ds_attn_fused_output", C.byref(p), st)
    sync()
    views = [part, ctx, y, sp] + ([mf] if mf is not None else [])
    S.check_guards(*views, *[v for n, v in d.items() if hasattr(v, "slab_guard")])
    unchanged(d["x"], c.x.float().bfloat16())
    unchanged(d["bias"], c.bias.float())
    unchanged(d["gn_part"], d["gn_part_src"])
    if d["label"] is not None:
        unchanged(d["label"], c.label_full.float())
    assert torch.equal(bits(ctx.cpu()), bits(ctx_after_pass1)), "the output pass leaves the context alone"
    pc = part.cpu().view(B, 4, nseg, R.PARTF)
    assert bool(torch.isfinite(pc[..., 32:]).all()) and not bool(torch.isnan(pc).any()), "every segment's partial is written (empty: max -inf, sum 0, context 0)"
    return ctx_after_pass1, y.cpu(), sp.cpu(), (mf.cpu() if mf is not None else None), parts, g_ctx | g_out


def check(c, k, nseg, res, what):
    ctx, y, sp, mf, parts, gens = res
    cf, of, batch = R.forms(k)
    assert gens == R.generations(k["B"], k["N"], k["C"], k["gen"], k["hint"], k["mfold"]), what
    assert parts == R.stats_parts(k["B"], k["N"], k["C"], k["gen"], k["hint"], k["mfold"]), what
    E.assert_bits_equal(ctx, c.want_ctx, what + " ctx")
    E.assert_bits_equal(y, c.want_y, what + " y")
    gen2_out = of[0] == "out2"
    if gen2_out:
        E.assert_bits_equal(mf, E.rne_bf16(mfold_ref(c.mb64)), what + " M_b")
    elif mf is not None:
        assert bool(torch.isnan(mf.float()).all()), "the first-generation output pass leaves mfold alone"
    want = R.block_stats(c, of, batch, rounded=gen2_out)
    assert tuple(sp.shape) == tuple(want.shape), what
    if c.stats_exact:
        E.assert_bits_equal(sp.double(), want, what + " statistics slots")
        E.assert_stats_exact(sp.double().sum(1), (c.want_y.double() if gen2_out else c.z64), what)
    else:
        # fp32 sums of n values in some order: each of at most n additions is off by at most 2^-24 of a partial sum, itself at most sum |.|
        v = (c.want_y.double() if gen2_out else c.z64).flatten(1)
        n = v.shape[1]
        for j, t in enumerate((v, v * v)):
            err = (sp.double().sum(1)[:, j] - t.sum(1)).abs()
            assert bool((err <= n * 2.0 ** -24 * t.abs().sum(1)).all()), (what, j, err.max().item())
    return cf, of, batch


@pytest.mark.parametrize("k", R.gpu_cases(), ids=R.case_id)
def test_attn_fused_exact(k):
    lib = L.load()
    c = R.build(k)
    nseg = R.resolve_nseg(k)
    if k["nseg"] == "lib":
        hb = R.fused_batch(k["B"], k["hint"]) if k["gen"] == 0 else k["B"]
        assert lib.ds_attn_fused_segments_gen(hb, k["N"], k["C"], k["gen"]) == nseg
    what = "ds_attn_fused " + R.case_id(k)
    res = launch(c, k, nseg, k["gen"], k["gen"], k["gn"])
    cf, of, batch = check(c, k, nseg, res, what)
    extra = ""
    if k["gn"] == "part":                                   # the other statistics form: the same bits
        res2 = launch(c, k, nseg, k["gen"], k["gen"], "ab")
        for a, b in zip(res[:4], res2[:4]):
            assert (a is None and b is None) or torch.equal(bits(a), bits(b)), what + ": gn_ab and gn_part store different bits"
        extra += "; gn_ab == gn_part"
    if k["gen"] == 0:                                       # the forced generations it reports: the same bits
        gens = res[5]
        res2 = launch(c, k, nseg, 2 if gens & 1 else 1, 2 if gens & 2 else 1, k["gn"])
        for a, b in zip(res[:4], res2[:4]):
            assert (a is None and b is None) or torch.equal(bits(a), bits(b)), what + ": gen = 0 and the forced generations store different bits"
        extra += "; gen 0 == forced (ctx %d, out %d)" % (2 if gens & 1 else 1, 2 if gens & 2 else 1)
    note("attn exact %s: %s nseg %d, %s batch %d; ctx, y%s equal to float64 bit for bit; statistics %s (margin %.3g of 2^24); y rounds on %.4f (%d ties); margins "
         "proj %.0f ctx %.0f z %.0f%s; paths %s | %s" %
         (R.case_id(k), "<".join(map(str, cf)), nseg, "<".join(map(str, of)), batch, ", M_b" if of[0] == "out2" else "", "per slot exact" if c.stats_exact else "bounded",
          c.stats_margin / E.LIMIT, c.round_share, c.round_ties, c.margin_proj, c.margin_ctx, c.margin_z, extra,
          " ".join(sorted(R.ctx_paths(cf, k["N"], nseg))), " ".join(sorted(R.out_paths(of, k["N"], k["C"], batch)))))


def test_launch_rules():
    """ds_attn_fused_generations, _segments(_gen), _stats_parts against the restatement of tests/attn_ref.py."""
    lib = L.load()
    n = 0
    for Cc in (96, 192, 384):
        for B in (1, 2, 3, 31, 32, 95, 96, 97, 256, 600, 3000):
            for N in (1, 31, 32, 33, 127, 128, 129, 1023, 1024, 1056, 4095, 4096, 4129, 16384):
                for gen in (0, 1, 2):
                    assert lib.ds_attn_fused_segments_gen(B, N, Cc, gen) == R.segments_gen(B, N, Cc, gen), (B, N, Cc, gen)
                    if gen == 0:
                        assert lib.ds_attn_fused_segments(B, N, Cc) == R.segments_gen(B, N, Cc, 0)
                    for hint in (0, 31, 32, 95, 96, 512):
                        for mfold in (False, True):
                            p = L.AttnFusedParams(B=B, N=N, C=Cc, nseg=1, gen=gen, batch_hint=hint, mfold=(16 if mfold else None))
                            assert lib.ds_attn_fused_generations(C.byref(p)) == R.generations(B, N, Cc, gen, hint, mfold), (B, N, Cc, gen, hint, mfold)
                            assert lib.ds_attn_fused_stats_parts(C.byref(p)) == R.stats_parts(B, N, Cc, gen, hint, mfold), (B, N, Cc, gen, hint, mfold)
                            n += 1
    note("attn launch rules: %d (B, N, C, gen, hint, mfold) points agree with the restatement" % n)


def test_pack_rounds_and_permutes():
    """ds_pack_attn_fused on weights whose products with gamma need a real bf16 rounding (with ties), and a to_out whose every element is
    distinct (the permutation is then checked element by element); ds_conv_fold_tables (bias NULL) on the same weights."""
    for Cc in (96, 192, 384):
        g = E.gen(77 + Cc)
        w = E.ints(g, (384, Cc), -1023, 1023)                                   # 10 bits: w gamma rounds to 8, with ties (x.5 ulp when gamma = 3)
        gamma = E.choice(g, (Cc,), [0.5, 1.0, 2.0, 3.0, -1.0])
        beta = E.ints(g, (Cc,), -3, 3)
        wo = (torch.randperm(Cc * 128, generator=g).double() - Cc * 64).view(Cc, 128)      # distinct integers below 2^16: most round
        prod = w * gamma.view(1, Cc)
        E.check_rounding(prod)
        E.check_rounding(wo)
        assert wo.unique().numel() == wo.numel()
        src = [S.slab(t.float()) for t in (w, gamma, wo, beta)]
        wq16, wo16, t1, t2 = S.nan_slab((384, Cc), BF), S.nan_slab((Cc, 128), BF), S.nan_slab((384,)), S.nan_slab((384,))
        st = L.current_stream()
        L.call("ds_pack_attn_fused", src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), wq16.data_ptr(), wo16.data_ptr(), Cc, st)
        L.call("ds_conv_fold_tables", src[0].data_ptr(), None, src[1].data_ptr(), src[3].data_ptr(), 384, Cc, 1, 1, t1.data_ptr(), t2.data_ptr(), st)
        sync()
        S.check_guards(wq16, wo16, t1, t2, *src)
        E.assert_bits_equal(wq16.cpu(), E.rne_bf16(prod), "pack wqkv C=%d" % Cc)
        # the permutation on the fp32 values (distinct), then the one rounding
        E.assert_bits_equal(wo16.cpu(), E.rne_bf16(wout_perm_ref(wo)), "pack wout_perm C=%d" % Cc)
        E.check_exact(max((w.abs() @ beta.abs()).max().item(), (w.abs() @ gamma.abs()).max().item() / 0.5))
        E.assert_bits_equal(t1.cpu(), (w @ beta).float(), "fold tables t1 C=%d" % Cc)
        E.assert_bits_equal(t2.cpu(), (w @ gamma).float(), "fold tables t2 C=%d" % Cc)
        share, ties = E.rounding_profile(prod)
        note("attn pack C=%d: wqkv, wout_perm, t1, t2 equal to float64 bit for bit; w gamma rounds on %.3f (%d ties)" % (Cc, share, ties))


def test_rejections_store_nothing():
    """C = 80, nseg = 0, a negative batch_hint and a misaligned x are refused with the documented message before anything is launched."""
    k = dict(C=96, B=1, N=33, gen=1, nseg=2, hint=0, wide=True, label=True, mfold=True, gn="ab")
    c = R.build(k)
    d = packed(c)
    part, ctx, y, sp = S.nan_slab((2 * 4 * R.PARTF,)), S.nan_slab((1, 4, 32, 32)), S.nan_slab((1, 33, 96), BF), S.nan_slab((1, 64, 2))
    xmis = S.slab(c.x.float().bfloat16(), offset_floats=1)
    base = dict(x=d["x"].data_ptr(), B=1, N=33, C=96, nseg=2, wqkv=d["wq16"].data_ptr(), t1=d["t1"].data_ptr(), t2=d["t2"].data_ptr(),
                gn_ab=d["gn_ab"].data_ptr(), label_q=d["label"].data_ptr(), lq_stride=c.lq_stride, scale=c.scale, part=part.data_ptr(), ctx=ctx.data_ptr(),
                wout_perm=d["wo16"].data_ptr(), bias_out=d["bias"].data_ptr(), y=y.data_ptr(), stats_part=sp.data_ptr(), gen=1)
    for change, msg in ((dict(C=80), "unsupported"), (dict(nseg=0), "bad sizes"), (dict(batch_hint=-1), "batch_hint"), (dict(x=xmis.data_ptr()), "16-byte aligned"),
                        (dict(gn_ab=None), "null pointer")):
        p = L.AttnFusedParams(**{**base, **change})
        for fn in ("ds_attn_fused_context", "ds_attn_fused_output"):
            with pytest.raises(L.DsError, match=msg):
                L.call(fn, C.byref(p), L.current_stream())
    sync()
    for t in (part, ctx, y, sp):
        assert bool(torch.isnan(t.float()).all())
    S.check_guards(part, ctx, y, sp, xmis)


# ================================================================================================= the split-precision tier (csrc/attn_x3.hip)
def x3_mfold_ref(c):
    """attn_x3_fold's two planes [B][2][C][128] in the operand layout of pass 2 (mfold_ref per plane)."""
    hi, lo = E.split_hi_lo(c.mb64)
    return torch.stack([E.rne_bf16(mfold_ref(hi)), E.rne_bf16(mfold_ref(lo))], 1)


_X3_PACKED = {}


def x3_packed(c):
    if c.id in _X3_PACKED:
        return _X3_PACKED[c.id]
    Cc = c.C
    src = {"wqkv": S.slab(c.wqkv.float()), "gamma": S.slab(c.gamma.float()), "beta": S.slab(c.beta.float())}
    whl, t1, t2 = S.nan_slab((2, 384, Cc), BF), S.nan_slab((384,)), S.nan_slab((384,))
    st = L.current_stream()
    L.call("ds_pack_attn_x3", src["wqkv"].data_ptr(), src["gamma"].data_ptr(), whl.data_ptr(), Cc, st)
    L.call("ds_conv_fold_tables", src["wqkv"].data_ptr(), None, src["gamma"].data_ptr(), src["beta"].data_ptr(), 384, Cc, 1, 1, t1.data_ptr(), t2.data_ptr(), st)
    sync()
    S.check_guards(whl, t1, t2, *src.values())
    hi, lo = E.split_hi_lo(c.wpk)
    E.assert_bits_equal(whl.cpu(), torch.stack([E.rne_bf16(hi), E.rne_bf16(lo)]), "ds_pack_attn_x3 " + c.id)
    E.assert_bits_equal(t1.cpu(), c.t1.float(), "ds_conv_fold_tables t1 " + c.id)
    E.assert_bits_equal(t2.cpu(), c.t2.float(), "ds_conv_fold_tables t2 " + c.id)
    on_gamma = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.arange(Cc) % 3]       # powers of two: the scale and shift rows are exact products
    on_beta = (torch.arange(Cc) % 5 - 2).double()
    part, count, eps = R.gn_partials(c)
    d = dict(whl=whl, t1=t1, t2=t2, x=S.slab(c.x.float()), wout=S.slab(c.wout.float()), bias=S.slab(c.bias.float()), gn_ab=S.slab(E.gn_ab_tensor(c.a, c.mean)),
             label=S.slab(c.label_full.float()) if c.label_full is not None else None, on_gamma=S.slab(on_gamma.float()), on_beta=S.slab(on_beta.float()),
             gn_part=S.slab(part), gn_count=count, gn_eps=eps, gn_part_src=part, on_gamma64=on_gamma, on_beta64=on_beta)
    _X3_PACKED[c.id] = d
    return d


def x3_stats_check(c, sp, want, what):
    if c.stats_exact:
        E.assert_bits_equal(sp.double(), want, what + " statistics slots")
        E.assert_stats_exact(sp.double().sum(1), c.z64, what)
    else:
        v = c.z64.flatten(1)
        for j, t in enumerate((v, v * v)):
            err = (sp.double().sum(1)[:, j] - t.sum(1)).abs()
            assert bool((err <= v.shape[1] * 2.0 ** -24 * t.abs().sum(1)).all()), (what, j, err.max().item())


@pytest.mark.parametrize("k", R.x3_gpu_cases(), ids=R.x3_case_id)
def test_attn_x3_exact(k):
    lib = L.load()
    c = R.x3_build(k)
    d = x3_packed(c)
    B, N, Cc = c.B, c.N, c.C
    nseg = R.x3_resolve_nseg(k)
    batch = R.fused_batch(B, k["hint"])
    if k["nseg"] == "lib":
        assert lib.ds_attn_x3_segments(batch, N, Cc) == nseg
    what = "ds_attn_x3 " + R.x3_case_id(k)
    OE = 1e-5

    def run(gn, form, planes=False, keep_out=True):
        """context + output.  form 'A': y and statistics; 'B': out = x + GroupNorm(y) (statistics from the first of two passes)."""
        part = S.nan_slab((lib.ds_linattn_part_floats(B, 4, nseg),))
        ctx = S.nan_slab((B, 4, 32, 32))
        qpl = S.nan_slab((lib.ds_attn_x3_qplane_bytes(B, N) // 4,))
        mf = S.nan_slab((B, 2, Cc, 128), BF)
        assert lib.ds_attn_x3_mfold_bytes(B, Cc) == mf.numel() * 2
        y = S.nan_slab((B, N, Cc))
        pl = S.nan_slab((B, N, 2 * Cc), BF) if planes else None
        p = L.AttnX3Params(x=d["x"].data_ptr(), B=B, N=N, C=Cc, nseg=nseg, wqkv_hl=d["whl"].data_ptr(), t1=d["t1"].data_ptr(), t2=d["t2"].data_ptr(),
                           label_q=L.ptr(d["label"]), lq_stride=c.lq_stride, scale=c.scale, part=part.data_ptr(), ctx=ctx.data_ptr(), qplanes=qpl.data_ptr(),
                           mfold=mf.data_ptr(), wout=d["wout"].data_ptr(), bias_out=d["bias"].data_ptr(), stats_part=None, batch_hint=k["hint"])
        if gn == "ab":
            p.gn_ab = d["gn_ab"].data_ptr()
        else:
            p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = d["gn_part"].data_ptr(), d["gn_part_src"].shape[1], d["gn_count"], d["gn_eps"]
        parts = lib.ds_attn_x3_stats_parts(C.byref(p))
        assert parts == R.x3_stats_parts(B, N, Cc, k["hint"])
        sp = S.nan_slab((B, parts, 2))
        p.stats_part = sp.data_ptr()
        if form == "A":
            p.y = y.data_ptr()
        else:
            p.out = y.data_ptr() if keep_out else None
            p.out_planes, p.on_gamma, p.on_beta, p.on_eps = L.ptr(pl), d["on_gamma"].data_ptr(), d["on_beta"].data_ptr(), OE
        st = L.current_stream()
        L.call("ds_attn_x3_context", C.byref(p), st)
        sync()
        ctx1 = ctx.cpu()
        L.call("ds_attn_x3_output", C.byref(p), st)
        sync()
        S.check_guards(part, ctx, qpl, mf, y, sp, *([pl] if planes else []), *[v for v in d.values() if hasattr(v, "slab_guard")])
        unchanged(d["x"], c.x.float())
        unchanged(d["wout"], c.wout.float())
        if d["label"] is not None:
            unchanged(d["label"], c.label_full.float())
        assert torch.equal(bits(ctx.cpu()), bits(ctx1))
        pc = part.cpu().view(B, 4, nseg, R.PARTF)
        assert bool(torch.isfinite(pc[..., 32:]).all()) and not bool(torch.isnan(pc).any())
        if form == "B" and not keep_out:
            assert bool(torch.isnan(y).all()), "form B without `out` stores no fp32 tensor"
        return ctx1, y.cpu(), sp.cpu(), mf.cpu(), (pl.cpu() if planes else None)

    ctx, y, sp, mf, _ = run(k["gn"], "A")
    E.assert_bits_equal(ctx, c.want_ctx, what + " ctx")
    E.assert_bits_equal(mf, x3_mfold_ref(c), what + " M_b planes")
    E.assert_bits_equal(y, c.want_y, what + " y")
    want_slots = R.x3_block_stats(c, batch)
    assert tuple(sp.shape) == tuple(want_slots.shape)
    x3_stats_check(c, sp, want_slots, what)
    extra = ""
    if k["gn"] == "part":
        r2 = run("ab", "A")
        for a, b in zip((ctx, y, sp, mf), r2[:4]):
            assert torch.equal(bits(a), bits(b)), what + ": gn_ab and gn_part store different bits"
        extra += "; gn_ab == gn_part"
    # form B: the first pass's partials (checked as above), then out from exactly those partials
    ctxb, outb, spb, _, _ = run(k["gn"], "B")
    x3_stats_check(c, spb, want_slots, what + " form B")
    want_out, want_hi, want_lo = R.x3_form_b(c, spb, d["on_gamma64"], d["on_beta64"], OE)
    E.assert_bits_equal(outb, want_out, what + " form B out")
    for keep in (True, False):
        _, outc, spc, _, pl = run(k["gn"], "B", planes=True, keep_out=keep)
        assert torch.equal(bits(spc), bits(spb))
        if keep:
            E.assert_bits_equal(outc, want_out, what + " form B out beside the planes")
        E.assert_bits_equal(pl[..., :Cc].contiguous(), want_hi, what + " out_planes hi (out %s)" % keep)
        E.assert_bits_equal(pl[..., Cc:].contiguous(), want_lo, what + " out_planes lo (out %s)" % keep)
    lo_share = E.split_profile(want_out.double())
    note("attn x3 exact %s: nseg %d batch %d; ctx, M_b planes, y, form B out and out_planes equal to float64 bit for bit; statistics %s (margin %.3g of 2^24); "
         "margins of 2^24: proj %.3f ctx %.3f z %.3f; shares lo != 0: x %.3f (third part dropped %.3f) W gamma v rows %.3f V %.3f M_b %.3f q~ %.3f, out lo %.3f (dropped %.3f)%s; "
         "paths %s | %s" % (R.x3_case_id(k), nseg, batch, "per slot exact" if c.stats_exact else "bounded", c.stats_margin / E.LIMIT, c.margin_proj / E.LIMIT,
                            c.margin_ctx / E.LIMIT, c.margin_z / E.LIMIT, c.share["x_lo"], c.share["x_wide3"], c.share["wv_lo"], c.share["v_lo"], c.share["mb_lo"],
                            c.share["q_lo"], lo_share[0], lo_share[1], extra, " ".join(sorted(R.x3_ctx_paths(Cc, N, nseg, B))),
                            " ".join(sorted(R.x3_out_paths(N, Cc, batch)))))


def test_x3_launch_rules():
    lib = L.load()
    n = 0
    for Cc in (96, 192, 384):
        for B in (1, 2, 3, 31, 32, 96, 128, 256, 600, 3000):
            for N in (1, 31, 32, 33, 129, 255, 256, 257, 1056, 4096, 4129, 16384):
                assert lib.ds_attn_x3_segments(B, N, Cc) == R.x3_segments(B, N, Cc), (B, N, Cc)
                for hint in (0, 32, 96, 512):
                    p = L.AttnX3Params(B=B, N=N, C=Cc, nseg=1, batch_hint=hint)
                    assert lib.ds_attn_x3_stats_parts(C.byref(p)) == R.x3_stats_parts(B, N, Cc, hint), (B, N, Cc, hint)
                    n += 1
    note("attn x3 launch rules: %d (B, N, C, hint) points agree with the restatement" % n)


def test_x3_rejections_store_nothing():
    """C = 80, nseg = 0, a negative batch_hint, a misaligned x and form B without stats_part are refused before anything is launched."""
    k = dict(C=96, B=2, N=33, nseg=2, flavour="wlo", hint=0, label=True, gn="ab")
    c = R.x3_build(k)
    d = x3_packed(c)
    lib = L.load()
    part, ctx, y, sp = S.nan_slab((2 * 2 * 4 * R.PARTF,)), S.nan_slab((2, 4, 32, 32)), S.nan_slab((2, 33, 96)), S.nan_slab((2, 64, 2))
    mf, qpl = S.nan_slab((2, 2, 96, 128), BF), S.nan_slab((lib.ds_attn_x3_qplane_bytes(2, 33) // 4,))
    xmis = S.slab(c.x.float(), offset_floats=1)
    base = dict(x=d["x"].data_ptr(), B=2, N=33, C=96, nseg=2, wqkv_hl=d["whl"].data_ptr(), t1=d["t1"].data_ptr(), t2=d["t2"].data_ptr(), gn_ab=d["gn_ab"].data_ptr(),
                label_q=d["label"].data_ptr(), lq_stride=c.lq_stride, scale=c.scale, part=part.data_ptr(), ctx=ctx.data_ptr(), qplanes=qpl.data_ptr(), mfold=mf.data_ptr(),
                wout=d["wout"].data_ptr(), bias_out=d["bias"].data_ptr(), y=y.data_ptr(), stats_part=sp.data_ptr())
    for change, msg in ((dict(C=80), "unsupported"), (dict(nseg=0), "bad sizes"), (dict(batch_hint=-1), "batch_hint"), (dict(x=xmis.data_ptr()), "16-byte aligned")):
        p = L.AttnX3Params(**{**base, **change})
        for fn in ("ds_attn_x3_context", "ds_attn_x3_output"):
            with pytest.raises(L.DsError, match=msg):
                L.call(fn, C.byref(p), L.current_stream())
    p = L.AttnX3Params(**{**base, **dict(y=None, out=y.data_ptr(), stats_part=None, on_gamma=d["on_gamma"].data_ptr(), on_beta=d["on_beta"].data_ptr(), on_eps=1e-5)})
    with pytest.raises(L.DsError, match="form B needs"):
        L.call("ds_attn_x3_output", C.byref(p), L.current_stream())
    sync()
    for t in (part, ctx, y, sp, mf, qpl):
        assert bool(torch.isnan(t.float()).all())
    S.check_guards(part, ctx, y, sp, mf, qpl, xmis)
