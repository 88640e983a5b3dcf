#!/usr/bin/env python3
"""Bit equality of two builds of the library on one device: python tools/lib_equivalence.py --family FAMILY PARENT.so [NEW.so] [-o FILE]

One fresh child process per library (DS_LIB=<file name under diffusynth_amd/>) runs the family's cases on the same synthetic inputs and
prints the sha256 of every buffer the entry points write; this process (which never opens the device) lists them, one line per case:
`<case>  <buffer>=<sha256 of the parent's bytes> ...  == parent`, or `<buffer>=<parent's>!=<new library's>` and `!= parent`; `<buffer>=^`
stands for the digest that buffer has in the line above (a buffer that an input of the case cannot reach).  Exit status 1 if any buffer differs.
A family is a generator of (case label, {buffer name: tensor}); add one here for the next refactor that has to keep every bit."""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rand(gen, *shape):
    import torch
    return torch.randn(*shape, generator=gen)


def attn_bf16_cases():
    """ds_attn_fused_context + _output (both generations) and ds_vq_attn_context + _output."""
    import torch
    from diffusynth_amd import _lib as L
    lib, st = L.load(), L.current_stream()
    for (Cc, H, W), gen, nseg_req, from_part, label, hint in itertools.product(
            ((96, 5, 10), (96, 16, 16), (96, 64, 64), (192, 33, 32), (384, 8, 6), (384, 32, 33)), (1, 2), (1, 3, 0), (False, True), (False, True), (0, 128)):
        B, N = 2, H * W
        g = torch.Generator().manual_seed(1000 * Cc + N)
        x = (_rand(g, B, N, Cc) * 1.3 + 0.2).bfloat16().cuda()
        wq = (_rand(g, 384 * Cc) * Cc ** -0.5).bfloat16().cuda()
        wo = (_rand(g, Cc * 128) * 128 ** -0.5).bfloat16().cuda()
        t1, t2, lq, bo = (_rand(g, 384) * 0.1).cuda(), (_rand(g, 384) * 0.1).cuda(), _rand(g, B, 128).cuda(), _rand(g, Cc).cuda()
        xf = x.float().reshape(B, -1)
        var, mean = torch.var_mean(xf, 1, unbiased=False)
        ab = torch.stack([torch.rsqrt(var + 1e-5), torch.rsqrt(var + 1e-5) * mean], 1).contiguous()
        gpart = torch.stack([xf.sum(1), (xf * xf).sum(1)], 1)[:, None, :].repeat(1, 5, 1).div(5.0).contiguous()      # five equal partials per sample
        nseg = nseg_req or lib.ds_attn_fused_segments_gen(hint or B, N, Cc, gen)
        part = torch.zeros(lib.ds_linattn_part_floats(B, 4, nseg), device="cuda")
        ctx, mf = torch.zeros(B * 4 * 1024, device="cuda"), torch.zeros(B * Cc * 128, dtype=torch.bfloat16, device="cuda")
        y = torch.zeros(B, N, Cc, dtype=torch.bfloat16, device="cuda")
        p = L.AttnFusedParams(x=x.data_ptr(), B=B, N=N, C=Cc, nseg=nseg, wqkv=wq.data_ptr(), t1=t1.data_ptr(), t2=t2.data_ptr(),
                              gn_ab=None if from_part else ab.data_ptr(), label_q=lq.data_ptr() if label else None, lq_stride=128,
                              scale=32 ** -0.5, part=part.data_ptr(), ctx=ctx.data_ptr(), wout_perm=wo.data_ptr(), bias_out=bo.data_ptr(),
                              y=y.data_ptr(), stats_part=None)
        if from_part:
            p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = gpart.data_ptr(), 5, float(N * Cc), 1e-5
        p.mfold, p.gen, p.batch_hint = (mf.data_ptr() if Cc in (96, 192) else None), gen, hint
        sp = torch.zeros(B, lib.ds_attn_fused_stats_parts(C.byref(p)), 2, device="cuda")
        p.stats_part = sp.data_ptr()
        L.call("ds_attn_fused_context", C.byref(p), st)
        L.call("ds_attn_fused_output", C.byref(p), st)
        yield (f"fused C={Cc} HxW={H}x{W} B={B} gen={gen} nseg={nseg_req or 'own:%d' % nseg} gn={'part' if from_part else 'ab'} "
               f"label_q={int(label)} hint={hint}"), dict(part=part, ctx=ctx, mfold=mf, y=y, stats_part=sp)
    for (dim, H, W, B), skip in itertools.product(((80, 4, 8, 1), (80, 19, 45, 3), (160, 9, 70, 2), (160, 32, 64, 3)), (False, True)):
        N = H * W
        g = torch.Generator().manual_seed(7000 + dim + N)
        x = (_rand(g, B, N, dim) * 1.3 + 0.1).bfloat16().cuda()
        wqkv = _rand(g, 96, dim) * (2.0 / dim ** 0.5)
        wout, bias, wnin = (_rand(g, dim, 32) * 0.2).cuda(), (_rand(g, dim) * 0.3).cuda(), (_rand(g, dim, dim) * dim ** -0.5).cuda()
        wqkv_d, wq_d = wqkv.bfloat16().contiguous().cuda(), wqkv[:32].contiguous().cuda()
        nseg = lib.ds_vq_attn_segments(B, N, dim)
        part, cx = torch.zeros(lib.ds_linattn_part_floats(B, 1, nseg), device="cuda"), torch.zeros(B, 32, 32, device="cuda")
        wfold = torch.zeros(lib.ds_vq_attn_wfold_bytes(B, dim), dtype=torch.uint8, device="cuda")
        y, ws = torch.zeros(B, N, dim, dtype=torch.bfloat16, device="cuda"), torch.zeros(B, nseg // 4, dim, 2, device="cuda")
        p = L.VqAttnParams(x=x.data_ptr(), B=B, N=N, C=dim, nseg=nseg, wqkv=wqkv_d.data_ptr(), wq=wq_d.data_ptr(), wout=wout.data_ptr(),
                           wnin=wnin.data_ptr() if skip else None, bias=bias.data_ptr(), part=part.data_ptr(), ctx=cx.data_ptr(),
                           wfold=wfold.data_ptr(), y=y.data_ptr(), stats_ws=ws.data_ptr())
        L.call("ds_vq_attn_context", C.byref(p), st)
        L.call("ds_vq_attn_output", C.byref(p), st)
        yield f"vq C={dim} HxW={H}x{W} B={B} wnin={int(skip)}", dict(part=part, ctx=cx, wfold=wfold, y=y, stats_ws=ws)


def row_kernels_cases():
    """Every entry point of sampler_step.hip, window.hip and stft_window.hip at the smallest shapes where they can go wrong: both forms
    (16-byte / scalar, by size and by address), duplicates, and one malformed row of every class.  Output buffers start from a fixed
    pattern, so a row that must not be written shows in the digest."""
    import numpy as np
    import torch
    from diffusynth_amd import _lib as L
    from diffusynth_amd.windowed import _Layout, window_plan
    st = L.current_stream()
    SR, QS, EN, CR, CC, WM = L.SR, L.QS, L.EN, L.CR, L.CC, L.WM
    keep = []                                             # the device tables of a launch live until the case has been hashed

    def dev(t, off=False):
        """t on the device; off: one element behind an allocation's start (4 bytes off every 16-byte boundary)."""
        t = t.contiguous()
        if not off:
            d = t.cuda()
        else:
            flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
            flat[1:] = t.reshape(-1).cuda()
            d = flat[1:].view(t.shape)
        keep.append(d)
        return d

    def pat(*shape):
        n = int(np.prod(shape))
        return ((torch.arange(n, dtype=torch.float32) % 97) * 0.5 - 7.0).reshape(shape)

    def coefs(g, n, last=True):
        c = torch.rand(n, 5, generator=g) + 0.25
        if not last:
            c[:, 4] = 0
        return c

    for (Cc, H, W), off in (((4, 8, 20), False), ((4, 8, 64), False), ((3, 5, 7), False), ((4, 8, 20), True)):
        B, HW, CHW = 3, H * W, Cc * H * W
        tag = "CxHxW=%dx%dx%d%s" % (Cc, H, W, " +4B" if off else "")
        g = torch.Generator().manual_seed(31 * CHW + int(off))
        rnd = lambda *s: _rand(g, *s)                                                         # noqa: E731
        x, eps, epsc, noise = (dev(rnd(B, Cc, H, W), off) for _ in range(4))
        guide, init = dev(rnd(B, Cc, H, W), off), dev(rnd(B, Cc, H, W), off)
        mask1, maskc = dev((torch.rand(B, 1, H, W, generator=g) > 0.5).float(), off), dev((torch.rand(B, Cc, H, W, generator=g) > 0.5).float(), off)
        cf, cf1, qc = dev(coefs(g, B)), dev(coefs(g, B, last=False)), dev(torch.rand(B, 2, generator=g) + 0.1)

        # ---- call forms of the step kernels
        for cfg, (blend, mask) in itertools.product((False, True), ((0, None), (1, mask1), (1, maskc), (2, mask1), (2, maskc))):
            out = dev(pat(B, Cc, H, W), off)
            p = L.StepParams(x=x.data_ptr(), eps=eps.data_ptr(), eps_cond=epsc.data_ptr() if cfg else None, noise=noise.data_ptr(),
                             out=out.data_ptr(), coef=cf.data_ptr(), cfg_scale=3.5, blend_mode=blend, B=B, CHW=CHW, HW=HW)
            if blend:
                p.guide, p.init_noise, p.mask, p.qcoef, p.mask_chw = guide.data_ptr(), init.data_ptr(), mask.data_ptr(), qc.data_ptr(), int(mask is maskc)
            L.call("ds_ddim_step", C.byref(p), st)
            yield "ddim_step %s cfg=%d blend=%d mask=%s" % (tag, cfg, blend, "-" if mask is None else "chw" if mask is maskc else "hw"), dict(out=out)
        for second, cfg, (blend, mask) in itertools.product((False, True), (False, True), ((0, None), (1, maskc), (2, mask1))):
            out, hist = dev(pat(B, Cc, H, W), off), dev(rnd(B, Cc, H, W), off)
            p = L.DpmStepParams(x=x.data_ptr(), eps=eps.data_ptr(), eps_cond=epsc.data_ptr() if cfg else None, hist=hist.data_ptr(),
                                out=out.data_ptr(), coef=(cf if second else cf1).data_ptr(), cfg_scale=3.5, blend_mode=blend, B=B, C=Cc, H=H, W=W)
            if blend:
                p.guide, p.init_noise, p.mask, p.qcoef, p.mask_chw = guide.data_ptr(), init.data_ptr(), mask.data_ptr(), qc.data_ptr(), int(mask is maskc)
            L.call("ds_dpm_step", C.byref(p), st)
            yield "dpm_step %s order=%d cfg=%d blend=%d" % (tag, 1 + second, cfg, blend), dict(out=out, hist=hist)

        # ---- rows forms: x of 4 rows, eps of 6, out of 9 (row 8 is never named); a draw of 2 x C x H x (W + 3) behind a repeat column table
        draw_w, n_cols = W + 3, 2 * W
        xs, es, draw = dev(rnd(4, Cc, H, W), off), dev(rnd(6, Cc, H, W), off), dev(rnd(2, Cc, H, draw_w), off)
        cols = dev(torch.randint(0, draw_w, (n_cols,), generator=g, dtype=torch.int32))
        g_off = dev(rnd(Cc, H, W), True)                                                       # a guide 4 bytes off, whatever the launch's form

        def step_table(rows):
            """rows: dicts of the fields that differ from a plain row (x 0, eps 0, no cfg, out r, no dup, no blend, no noise)."""
            R = len(rows)
            ir, fr, pr = torch.zeros(R, SR["DS_SR_NI"], dtype=torch.int32), torch.zeros(R, SR["DS_SR_NF"]), torch.zeros(R, SR["DS_SR_NP"], dtype=torch.int64)
            hr = torch.zeros(R, dtype=torch.int64)
            fr[:, :5] = coefs(g, R)
            fr[:, SR["DS_SR_Q0"]], fr[:, SR["DS_SR_Q1"]], fr[:, SR["DS_SR_CFG"]] = 0.8, 0.6, 2.5
            for r, d in enumerate(rows):
                ir[r, SR["DS_SR_EPSC"]], ir[r, SR["DS_SR_DUP"]], ir[r, SR["DS_SR_OUT"]] = -1, -1, r
                ir[r, SR["DS_SR_DRAW_ROWS"]], ir[r, SR["DS_SR_DRAW_W"]] = 2, draw_w
                pr[r, SR["DS_SR_DRAW"]], pr[r, SR["DS_SR_SEED"]], pr[r, SR["DS_SR_OFFSET"]] = draw.data_ptr(), 1234 + r, 77
                for k, v in d.items():
                    if k == "hist":
                        hr[r] = v
                    elif k == "c4":
                        fr[r, 4] = v
                    elif "DS_SR_" + k in ("DS_SR_GUIDE", "DS_SR_INIT", "DS_SR_MASKP", "DS_SR_DRAW"):
                        pr[r, SR["DS_SR_" + k]] = v
                    else:
                        ir[r, SR["DS_SR_" + k]] = v
            return dev(ir), dev(fr), dev(pr), dev(hr)

        blend1 = dict(BLEND=1, GUIDE=guide[1].data_ptr(), INIT=init[1].data_ptr(), MASKP=mask1[1].data_ptr())
        blend2 = dict(BLEND=2, MASK_CHW=1, GUIDE=g_off.data_ptr(), MASKP=maskc[2].data_ptr())
        rows = [dict(X=1, EPS=2),                                                              # no noise
                dict(X=0, EPS=1, EPSC=3, DUP=7, NOISE=1, SAMPLE=1, COLS=0, **blend1),          # a draw, CFG, a duplicate row
                dict(X=3, EPS=5, NOISE=2, SAMPLE=0, COLS=W, **blend2),                         # Philox, the second half of the column table
                dict(X=4, EPS=0),                                                              # x out of range
                dict(X=0, EPS=0, BLEND=3),                                                     # unknown blend
                dict(X=0, EPS=0, BLEND=2, MASKP=mask1[0].data_ptr()),                          # missing guide
                dict(X=0, EPS=0, NOISE=1, SAMPLE=2),                                           # bad noise fields: a sample beyond the draw's rows
                dict(X=0, EPS=0, OUT=9)]                                                       # out-of-range output row
        ir, fr, pr, _ = step_table(rows)
        out = dev(pat(9, Cc, H, W), off)
        p = L.StepRowsParams(x=xs.data_ptr(), eps=es.data_ptr(), out=out.data_ptr(), irow=ir.data_ptr(), frow=fr.data_ptr(), prow=pr.data_ptr(),
                             cols=cols.data_ptr(), R=len(rows), C=Cc, H=H, W=W, Bx=4, Beps=6, Bout=9, n_cols=n_cols)
        L.call("ds_step_rows", C.byref(p), st)
        yield "step_rows " + tag, dict(out=out)

        hists = [dev(rnd(Cc, H, W), off), dev(rnd(Cc, H, W), True)]
        rows = [dict(X=1, EPS=2, c4=0.0),                                                      # first order, no history
                dict(X=0, EPS=1, EPSC=3, DUP=7, hist=hists[0].data_ptr()),                     # second order, CFG, a duplicate row
                dict(X=3, EPS=5, hist=hists[1].data_ptr(), **blend1),                          # second order, a history 4 bytes off, a blend
                dict(X=2, EPS=4),                                                              # second order without a history
                dict(X=0, EPS=0, c4=0.0, NOISE=1, SAMPLE=0),                                   # the solver draws no noise
                dict(X=0, EPS=0, c4=0.0, OUT=9)]                                               # out-of-range output row
        ir, fr, pr, hr = step_table(rows)
        out = dev(pat(9, Cc, H, W), off)
        p = L.StepRowsParams(x=xs.data_ptr(), eps=es.data_ptr(), out=out.data_ptr(), irow=ir.data_ptr(), frow=fr.data_ptr(), prow=pr.data_ptr(),
                             cols=None, R=len(rows), C=Cc, H=H, W=W, Bx=4, Beps=6, Bout=9, n_cols=0)
        L.call("ds_dpm_step_rows", C.byref(p), hr.data_ptr(), st)
        yield "dpm_step_rows " + tag, dict(out=out, hist0=hists[0], hist1=hists[1])

        # ---- the edit kernels
        rows = [(0, 0, 1, 1, 1, 0), (2, 2, -1, 2, 0, W), (1, 3, -1, 0, 1, 0), (3, 4, -1, 1, 0, 0)]      # src, out, dup, noise, sample, cols
        ir, fr, pr = torch.zeros(4, QS["DS_QS_NI"], dtype=torch.int32), torch.rand(4, QS["DS_QS_NF"], generator=g) + 0.1, torch.zeros(4, QS["DS_QS_NP"], dtype=torch.int64)
        for r, (src, orow, dup, nz, sample, co) in enumerate(rows):                             # row 2: no noise mode; row 3: a source out of range
            ir[r] = torch.tensor([src, orow, dup, nz, sample, 2, draw_w, co], dtype=torch.int32)
            pr[r] = torch.tensor([draw.data_ptr(), 99 + r, 5], dtype=torch.int64)
        assert [QS[k] for k in ("DS_QS_SRC", "DS_QS_OUT", "DS_QS_DUP", "DS_QS_NOISE", "DS_QS_SAMPLE", "DS_QS_DRAW_ROWS", "DS_QS_DRAW_W", "DS_QS_COLS")] == list(range(8))
        assert [QS[k] for k in ("DS_QS_DRAW", "DS_QS_SEED", "DS_QS_OFFSET")] == [0, 1, 2]
        ir, fr, pr = dev(ir), dev(fr), dev(pr)
        x0, out = dev(rnd(3, Cc, H, W), off), dev(pat(6, Cc, H, W), off)
        p = L.QSampleRowsParams(x0=x0.data_ptr(), out=out.data_ptr(), irow=ir.data_ptr(), frow=fr.data_ptr(), prow=pr.data_ptr(), cols=cols.data_ptr(),
                                R=4, C=Cc, H=H, W=W, Bx0=3, Bout=6, n_cols=n_cols)
        L.call("ds_q_sample_rows", C.byref(p), st)
        yield "q_sample_rows " + tag, dict(out=out)

        prev_a, prev_o = dev(rnd(Cc, H, W), off), dev(rnd(Cc, H, W), True)
        rows = [(0, 1, 2, -1, 0, 0, None), (1, -1, 0, 3, 1, prev_o.data_ptr(), None), (2, 3, 1, -1, 2, 0, 0.0), (4, 0, 0, -1, 3, 0, None),
                (0, -1, 0, -1, 4, 0, None), (3, -1, 5, 4, 5, prev_a.data_ptr(), None)]          # x, prev, eps, eps_c, out, prev address, coef[4]
        assert [EN[k] for k in ("DS_EN_X", "DS_EN_PREV", "DS_EN_EPS", "DS_EN_EPSC", "DS_EN_OUT")] == list(range(5))
        ir, fr, pr = torch.zeros(6, EN["DS_EN_NI"], dtype=torch.int32), torch.zeros(6, EN["DS_EN_NF"]), torch.zeros(6, EN["DS_EN_NP"], dtype=torch.int64)
        fr[:, :5], fr[:, EN["DS_EN_CFG"]] = coefs(g, 6), 2.5
        for r, (xr, pv, er, ecr, orow, addr, c4) in enumerate(rows):                            # row 2: coef[4] == 0; row 3: x out of range; row 4: no x_prev
            ir[r] = torch.tensor([xr, pv, er, ecr, orow], dtype=torch.int32)
            pr[r, EN["DS_EN_PREVP"]] = addr
            if c4 is not None:
                fr[r, 4] = c4
        ir, fr, pr = dev(ir), dev(fr), dev(pr)
        z = dev(pat(7, Cc, H, W), off)
        p = L.EditNoiseRowsParams(X=xs.data_ptr(), eps=es.data_ptr(), z=z.data_ptr(), irow=ir.data_ptr(), frow=fr.data_ptr(), prow=pr.data_ptr(),
                                  R=6, C=Cc, H=H, W=W, Bx=4, Beps=6, Bz=7)
        L.call("ds_edit_noise_rows", C.byref(p), st)
        yield "edit_noise_rows " + tag, dict(z=z)

        # ---- the guidance kernels
        for phi in (0.0, 0.7):
            out, gain = dev(pat(B, Cc, H, W), off), dev(pat(B))
            p = L.CfgRescaleParams(eps_u=eps.data_ptr(), eps_c=epsc.data_ptr(), out=out.data_ptr(), gain=gain.data_ptr(), cfg_scale=3.5, phi=phi, B=B, CHW=CHW)
            L.call("ds_cfg_rescale", C.byref(p), st)
            yield "cfg_rescale %s phi=%g" % (tag, phi), dict(out=out, gain=gain)
            e7, gain = dev(torch.cat([rnd(4, Cc, H, W), pat(3, Cc, H, W)]), off), dev(pat(4))
            ir = dev(torch.tensor([[0, 1, 4], [2, 3, 2], [0, 7, 5], [0, 1, 7]], dtype=torch.int32))      # row 1 writes its own u; row 2: c out of range; row 3: out
            fr = dev(torch.tensor([[3.5, phi], [2.0, phi], [3.5, phi], [3.5, phi]]))
            p = L.CfgRescaleRowsParams(eps=e7.data_ptr(), irow=ir.data_ptr(), frow=fr.data_ptr(), gain=gain.data_ptr(), R=4, CHW=CHW, Beps=7)
            L.call("ds_cfg_rescale_rows", C.byref(p), st)
            yield "cfg_rescale_rows %s phi=%g" % (tag, phi), dict(eps=e7, gain=gain)
        for K, per_col, phi in itertools.product((1, 3, 8), (False, True), (0.0, 0.7)):
            ww = W if per_col else 1
            ck, wt = dev(rnd(K, B, Cc, H, W), off), dev(torch.rand(2 * K * ww, generator=g), off)
            out, gain = dev(pat(B, Cc, H, W), off), dev(pat(B))
            p = L.CfgComposeParams(eps_u=eps.data_ptr(), eps_c=ck.data_ptr(), wt=wt.data_ptr(), out=out.data_ptr(), gain=gain.data_ptr(), cfg_scale=3.5,
                                   phi=phi, B=B, K=K, CHW=CHW, W=W, wt_w=ww)
            L.call("ds_cfg_compose", C.byref(p), st)
            yield "cfg_compose %s K=%d wt_w=%d phi=%g" % (tag, K, ww, phi), dict(out=out, gain=gain)
            # eps of 14 rows: u 0, c 1..8, outputs 10 / 11 / 12, 13 never named.  Row 1 walks its c rows downwards and takes the second table
            e14, gain = dev(torch.cat([rnd(9, Cc, H, W), pat(5, Cc, H, W)]), off), dev(pat(4))
            assert [CC[k] for k in ("DS_CC_U", "DS_CC_OUT", "DS_CC_K", "DS_CC_C0", "DS_CC_CSTRIDE", "DS_CC_WT", "DS_CC_WTW")] == list(range(7))
            ir = dev(torch.tensor([[0, 10, K, 1, 1, 0, ww], [0, 11, K, K, -1, K * ww, ww], [0, 12, K, 14 - K + 1, 1, 0, ww], [0, 14, K, 1, 1, 0, ww]],
                                  dtype=torch.int32))                                            # row 2: c_K out of range; row 3: out out of range
            fr = dev(torch.tensor([[3.5, phi], [2.0, phi], [3.5, phi], [3.5, phi]]))
            p = L.CfgComposeRowsParams(eps=e14.data_ptr(), irow=ir.data_ptr(), frow=fr.data_ptr(), wt=wt.data_ptr(), gain=gain.data_ptr(), R=4, CHW=CHW,
                                       W=W, Beps=14, n_wt=2 * K * ww)
            L.call("ds_cfg_compose_rows", C.byref(p), st)
            yield "cfg_compose_rows %s K=%d wt_w=%d phi=%g" % (tag, K, ww, phi), dict(eps=e14, gain=gain)

        # ---- the other kernels of sampler_step.hip
        buf = dev(torch.cat([rnd(4, Cc, H, W), pat(2, Cc, H, W)]), off)
        pairs = dev(torch.tensor([[0, 4], [1, 1], [2, 9], [3, 5]], dtype=torch.int32))         # (1, 1) and (2, 9) copy nothing
        L.call("ds_copy_rows", buf.data_ptr(), pairs.data_ptr(), 4, CHW, 6, st)
        yield "copy_rows " + tag, dict(buf=buf)
        gout = dev(pat(2 * Cc * H, W), off)
        L.call("ds_gather_cols", draw.data_ptr(), 2 * Cc * H, draw_w, cols.data_ptr(), W, gout.data_ptr(), st)
        yield "gather_cols " + tag, dict(out=gout)
        nrm = dev(pat(12), off)
        L.call("ds_philox_normal", nrm.data_ptr(), 10, 4321, 9, st)
        yield "philox_normal n=10 " + tag, dict(out=nrm)
        keep.clear()

    # ---- the window kernels: C = 2, H = 3, B = 2; the STFT merge at F = 5 on the frame plans of scale 4
    Cc, H, B, F = 2, 3, 2, 5
    for W, window, stride, loop in ((40, 16, 8, False), (40, 16, 8, True), (37, 16, 5, True)):
        tag = "W=%d window=%d stride=%d loop=%d" % (W, window, stride, loop)
        g = torch.Generator().manual_seed(9000 + W + int(loop))
        plan = window_plan(W, window, stride, loop)
        lay = _Layout(plan, B, False, None)
        x, rows = dev(_rand(g, B, Cc, H, W)), torch.from_numpy(lay.rows.copy())
        for bad in (False, True):
            if bad:
                rows[1, L.WS["DS_WS_OFF"]], rows[2, L.WS["DS_WS_SRC"]], rows[3, L.WS["DS_WS_DST"]] = W, B, lay.Rw
            xw, rd = dev(pat(lay.Rw, Cc, H, window)), dev(rows)
            p = L.WindowSplitParams(x=x.data_ptr(), out=xw.data_ptr(), rows=rd.data_ptr(), R=lay.Rw, C=Cc, H=H, W=W, w=window, Bx=B, Bout=lay.Rw)
            L.call("ds_window_split", C.byref(p), st)
            yield "window_split %s%s" % (tag, " malformed rows" if bad else ""), dict(out=xw)

        def merge_tables(pl, what):
            """(erow, wcol, wcoef) of plan pl: as planned, with an erow entry out of range, or with two malformed column entries."""
            erow = torch.from_numpy(lay.erow.copy())
            wcol = torch.from_numpy(np.ascontiguousarray(np.stack([pl.win.T, pl.col.T], axis=2)))
            if what == "erow":
                erow[1, 0] = lay.Rw
            if what == "wcol":
                wcol[0, 5, WM["DS_WM_COL"]] = pl.window                                        # a column beyond the window
                wcol[1, 9, WM["DS_WM_WIN"]] = pl.n                                             # a window that does not exist
            return dev(erow), dev(wcol), dev(torch.from_numpy(np.ascontiguousarray(pl.coef.T)))

        epsw = dev(_rand(g, lay.Rw, Cc, H, window))
        fplan = window_plan(4 * W, 4 * window, 4 * stride, loop)
        assert fplan.n == plan.n
        enc = _rand(g, lay.Rw, 3, F, 4 * window)
        encw = dev(torch.stack([enc[:, 0].abs(), torch.tanh(enc[:, 1]), torch.tanh(enc[:, 2])], 1))
        for what in ("plan", "erow", "wcol", "plan +4B"):                                      # +4B: the scalar form forced by the address
            off = what.endswith("+4B")
            if off:
                epsw, encw = dev(epsw, True), dev(encw, True)
            erow, wcol, wcoef = merge_tables(plan, what)
            out = dev(pat(B + 1, Cc, H, W), off)
            p = L.WindowMergeParams(eps=epsw.data_ptr(), out=out.data_ptr(), erow=erow.data_ptr(), wcol=wcol.data_ptr(), wcoef=wcoef.data_ptr(),
                                    R=B, n=plan.n, C=Cc, H=H, W=W, w=window, Beps=lay.Rw, Bout=B + 1)
            L.call("ds_window_merge", C.byref(p), st)
            yield "window_merge %s tables=%s" % (tag, what), dict(out=out)
            erow, wcol, wcoef = merge_tables(fplan, what)
            out = dev(pat(B + 1, 3, F, 4 * W), off)
            p = L.StftWindowMergeParams(encw=encw.data_ptr(), out=out.data_ptr(), erow=erow.data_ptr(), wcol=wcol.data_ptr(), wcoef=wcoef.data_ptr(),
                                        R=B, n=fplan.n, F=F, T=4 * W, w=4 * window, Bw=lay.Rw, Bout=B + 1)
            L.call("ds_stft_window_merge", C.byref(p), st)
            yield "stft_window_merge %s F=%d scale=4 tables=%s" % (tag, F, what), dict(out=out)
        keep.clear()


def conv_c80_cases():
    """Every entry point of conv3x3_c80.hip and convt4x4_c80.hip: one tile per run (B = 1, 3), ragged tiles, and the batches at which a
    9 x 70 sample is cut into runs of 2, 2, 2, 2, 1 and 0 tiles.  Outputs and statistics slots start from a fixed pattern, so an unwritten
    pixel or slot shows in the digest."""
    import torch
    from diffusynth_amd import _lib as L
    lib, st, G = L.load(), L.current_stream(), 16

    def pat(dtype, *shape):
        n = 1
        for d in shape:
            n *= d
        return ((torch.arange(n, dtype=torch.float32, device="cuda") % 97) * 0.5 - 7.0).reshape(shape).to(dtype)

    def gn_ab(x, B, HW, cin):
        ab = torch.empty(B, G, 2, device="cuda")
        L.call("ds_gn_stats", x.data_ptr(), L.DS_BF16, B, HW, cin, G, 1e-6, ab.data_ptr(), st)
        return ab

    g = torch.Generator().manual_seed(80)
    w3 = (_rand(g, 80, 80, 3, 3) * 0.04).contiguous().cuda()
    wp3 = pat(torch.bfloat16, lib.ds_conv3x3_c80_weight_elems())
    L.call("ds_pack_conv3x3_c80", w3.data_ptr(), 80, 80, wp3.data_ptr(), st)
    yield "pack_conv3x3_c80", dict(wpk=wp3)
    wpt = {}
    for cin in (80, 160):
        wt = (_rand(g, cin, 80, 4, 4) * 0.05).contiguous().cuda()
        wpt[cin] = pat(torch.bfloat16, lib.ds_convt4x4_c80_weight_elems(cin))
        L.call("ds_pack_convt4x4_c80", wt.data_ptr(), cin, 80, wpt[cin].data_ptr(), st)
        yield "pack_convt4x4_c80 cin=%d" % cin, dict(wpk=wpt[cin])
    bias = _rand(g, 80).cuda()

    for B, H, W in ((1, 3, 5), (3, 4, 32), (3, 19, 45), (40, 9, 70)):
        x = (_rand(g, B, H, W, 80) * 1.5 + 0.2).bfloat16().cuda()
        gamma, beta, ab = (_rand(g, 80) * 0.3 + 1.0).cuda(), (_rand(g, 80) * 0.5).cuda(), gn_ab(x, B, H * W, 80)
        slots = lib.ds_conv3x3_c80_stats_slots(B, H, W)
        norm = (ab.data_ptr(), G, gamma.data_ptr(), beta.data_ptr())
        for form, args, stats in (("plain", (None, 0, None, None, L.ACT_NONE, 0), False), ("gn+silu+x+stats", norm + (L.ACT_SILU, 1), True),
                                  ("gn+relu", norm + (L.ACT_RELU, 0), False)):
            for b in (bias, None):
                out, ws = pat(torch.bfloat16, B, H, W, 80), pat(torch.float32, B, slots, 80, 2)
                L.call("ds_conv3x3_c80", x.data_ptr(), B, H, W, wp3.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(), *args,
                       ws.data_ptr() if stats else None, st)
                yield "conv3x3_c80 B=%d HxW=%dx%d %s bias=%d" % (B, H, W, form, b is not None), dict(out=out, stats_ws=ws)
        for b in (bias, None):
            res = (_rand(g, B, H, W, 80) * 1.5).bfloat16().cuda()
            out, ws = pat(torch.bfloat16, B, H, W, 80), pat(torch.float32, B, slots, 80, 2)
            L.call("ds_conv3x3_c80_res", x.data_ptr(), res.data_ptr(), B, H, W, wp3.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(),
                   ws.data_ptr(), st)
            yield "conv3x3_c80_res B=%d HxW=%dx%d bias=%d" % (B, H, W, b is not None), dict(out=out, stats_ws=ws)

    for cin, shapes in ((80, ((3, 8, 32), (3, 19, 45), (20, 9, 70))), (160, ((3, 4, 32), (3, 19, 45), (10, 9, 70)))):
        for B, H, W in shapes:
            x = (_rand(g, B, H, W, cin) * 1.5 + 0.2).bfloat16().cuda()
            gamma, beta, ab = (_rand(g, cin) * 0.3 + 1.0).cuda(), (_rand(g, cin) * 0.5).cuda(), gn_ab(x, B, H * W, cin)
            slots = lib.ds_convt4x4_c80_stats_slots(B, H, W, cin)
            for form, args, stats in (("plain", (None, 0, None, None), False), ("gn+stats", (ab.data_ptr(), G, gamma.data_ptr(), beta.data_ptr()), True)):
                for b in (bias, None):
                    out, ws = pat(torch.bfloat16, B, 2 * H, 2 * W, 80), pat(torch.float32, B, slots, 80, 2)
                    L.call("ds_convt4x4_c80", x.data_ptr(), B, H, W, cin, wpt[cin].data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(),
                           *args, ws.data_ptr() if stats else None, st)
                    yield "convt4x4_c80 cin=%d B=%d HxW=%dx%d %s bias=%d" % (cin, B, H, W, form, b is not None), dict(out=out, stats_ws=ws)


def norms_cases():
    """Every entry point of groupnorm.hip on each path its launcher takes, and the LayerNorm / L2-norm rows of misc.hip and clap_text.hip at
    row lengths around the 256 threads of their tree sum.  Outputs start from a fixed pattern, so an unwritten element shows in the digest."""
    import torch
    from diffusynth_amd import _lib as L
    lib, st = L.load(), L.current_stream()
    TDT = {L.DS_F32: torch.float32, L.DS_BF16: torch.bfloat16}
    NAME = {L.DS_F32: "fp32", L.DS_BF16: "bf16"}
    g = torch.Generator().manual_seed(2718)

    def pat(dtype, *shape):
        n = 1
        for d in shape:
            n *= d
        return ((torch.arange(n, dtype=torch.float32, device="cuda") % 97) * 0.5 - 7.0).reshape(shape).to(dtype)

    def image(dt, B, HW, Cc):
        return (_rand(g, B, HW, Cc) * 1.5 + 0.3).to(TDT[dt]).cuda()

    def partials(x, n):
        """n equal (sum, sum of squares) partials per sample of x [B][HW][C]"""
        xf = x.float().reshape(x.shape[0], -1)
        return torch.stack([xf.sum(1), (xf * xf).sum(1)], 1)[:, None, :].repeat(1, n, 1).div(float(n)).contiguous()

    # ---- ds_gn_finalize: fewer partials than threads, one per thread, a ragged second trip, several trips; a constant image (variance ~ 0: the clamp)
    for parts, const in ((1, False), (64, False), (257, False), (600, False), (64, True)):
        x = torch.full((3, parts, 64), 0.7) if const else _rand(g, 3, parts, 64) * 1.3 + 0.2
        part = torch.stack([x.sum(2), (x * x).sum(2)], 2).contiguous().cuda()
        ab = pat(torch.float32, 3, 2)
        L.call("ds_gn_finalize", part.data_ptr(), 3, parts, float(parts * 64), 1e-5, ab.data_ptr(), st)
        yield "gn_finalize B=3 parts=%d%s" % (parts, " constant" if const else ""), dict(ab=ab)

    # ---- statistics
    for dt, (Cc, G, HW) in itertools.product((L.DS_F32, L.DS_BF16), ((96, 1, 60), (96, 8, 60), (160, 16, 7))):
        x, ab = image(dt, 2, HW, Cc), pat(torch.float32, 2, G, 2)
        L.call("ds_gn_stats", x.data_ptr(), dt, 2, HW, Cc, G, 1e-6, ab.data_ptr(), st)
        yield "gn_stats %s C=%d G=%d HW=%d" % (NAME[dt], Cc, G, HW), dict(ab=ab)
    for (Cc, dt, Gs), HW in itertools.product(((80, L.DS_BF16, (1, 16)), (96, L.DS_F32, (1, 8)), (160, L.DS_BF16, (1, 16))), (7, 60, 1500)):
        x = image(dt, 2, HW, Cc)
        nws = lib.ds_gn_stats_ws_floats(2, HW, Cc)
        for G in Gs:
            ws, ab, ab2 = pat(torch.float32, nws), pat(torch.float32, 2, G, 2), pat(torch.float32, 2, G, 2)
            L.call("ds_gn_stats_stream", x.data_ptr(), dt, 2, HW, Cc, G, 1e-6, ws.data_ptr(), ab.data_ptr(), st)
            L.call("ds_gn_stats_finish", ws.data_ptr(), 2, nws // (2 * Cc * 2), Cc, G, HW, 1e-6, ab2.data_ptr(), st)
            yield "gn_stats_stream + finish %s C=%d G=%d HW=%d" % (NAME[dt], Cc, G, HW), dict(ws=ws, ab=ab, ab_finish=ab2)

    # ---- ds_gn_apply, one block of cases per path of its launcher
    def apply(dt, B, HW, Cc, G, act, cbias, res, part):
        x, r, out = image(dt, B, HW, Cc), image(dt, B, HW, Cc), pat(TDT[dt], B, HW, Cc)
        gamma, beta, cb = (_rand(g, Cc) * 0.2 + 1.0).cuda(), (_rand(g, Cc) * 0.3).cuda(), _rand(g, B, Cc + 4).cuda()
        p = L.GnApplyParams(x=x.data_ptr(), res=r.data_ptr() if res else None, out=out.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                            cbias=cb.data_ptr() if cbias else None, cb_stride=Cc + 4, B=B, HW=HW, C=Cc, G=G, act=act, dtype=dt)
        if part:
            gp = partials(x, 5).cuda()
            p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = gp.data_ptr(), 5, float(HW * Cc), 1e-5
        else:
            ab = torch.empty(B, G, 2, device="cuda")
            L.call("ds_gn_stats", x.data_ptr(), dt, B, HW, Cc, G, 1e-5, ab.data_ptr(), st)
            p.gn_ab = ab.data_ptr()
        L.call("ds_gn_apply", C.byref(p), st)
        torch.cuda.synchronize()                                  # (the inputs die with this frame)
        return ("%s C=%d G=%d HW=%d act=%d cbias=%d res=%d" % (NAME[dt], Cc, G, HW, act, cbias, res)), dict(out=out)

    for Cc, res, HW in itertools.product((96, 192, 384, 768), (False, True), (3, 130)):
        label, bufs = apply(L.DS_BF16, 3, HW, Cc, 1, L.ACT_NONE, False, res, True)
        yield "gn_apply lazy-fast " + label, bufs
    for (dt, Cc, act, cbias), HW in itertools.product(((L.DS_F32, 96, L.ACT_NONE, False), (L.DS_BF16, 96, L.ACT_SILU, False),
                                                       (L.DS_BF16, 96, L.ACT_NONE, True), (L.DS_BF16, 80, L.ACT_NONE, False)), (3, 130)):
        label, bufs = apply(dt, 3, HW, Cc, 1, act, cbias, True, True)
        yield "gn_apply lazy " + label, bufs
    for dt, G, act, cbias, res in itertools.product((L.DS_F32, L.DS_BF16), (1, 8), (L.ACT_NONE, L.ACT_GELU, L.ACT_SILU, L.ACT_RELU), (False, True), (False, True)):
        label, bufs = apply(dt, 3, 60, 96, G, act, cbias, res, False)
        yield "gn_apply table " + label, bufs
    for dt, G in itertools.product((L.DS_F32, L.DS_BF16), (1, 4)):
        label, bufs = apply(dt, 2, 5, 1028 if dt == L.DS_F32 else 2056, G, L.ACT_SILU, True, True, False)
        yield "gn_apply generic " + label, bufs

    # ---- the LayerNorm and L2-norm rows
    for D in (1, 255, 256, 257, 768):
        a, r, out = (_rand(g, 3, D) * 1.2 + 0.1).cuda(), _rand(g, 3, D).cuda(), pat(torch.float32, 3, D)
        gamma, beta = (_rand(g, D) * 0.2 + 1.0).cuda(), (_rand(g, D) * 0.3).cuda()
        L.call("ds_add_layernorm", a.data_ptr(), r.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 3, D, 1e-5, out.data_ptr(), st)
        yield "add_layernorm B=3 D=%d" % D, dict(out=out)
    ids = torch.tensor([[0, 9, 1, 23, 2, 1, 1], [0, 48, 17, 5, 31, 12, 2]], dtype=torch.int64).cuda()      # pad = 1: one inside, two at the end
    for Hd in (5, 768):
        word, pos, type0 = _rand(g, 50, Hd).cuda(), _rand(g, 16, Hd).cuda(), _rand(g, Hd).cuda()
        gamma, beta, out = (_rand(g, Hd) * 0.2 + 1.0).cuda(), (_rand(g, Hd) * 0.3).cuda(), pat(torch.float32, 2, 7, Hd)
        L.call("ds_text_embed", ids.data_ptr(), 2, 7, 1, word.data_ptr(), 50, pos.data_ptr(), 16, type0.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
               Hd, 1e-5, out.data_ptr(), st)
        yield "text_embed B=2 S=7 H=%d" % Hd, dict(out=out)
    for D in (1, 257, 512):
        x, out = _rand(g, 3, D), pat(torch.float32, 3, D)
        x[1] = 0                                                  # an all-zero row stays zero
        x = x.cuda()
        L.call("ds_text_tail", x.data_ptr(), 3, D, L.TAIL["DS_TAIL_L2NORM"], 1e-12, out.data_ptr(), st)
        yield "text_tail l2norm B=3 D=%d" % D, dict(out=out)


FAMILIES = {"attn_bf16": attn_bf16_cases, "row_kernels": row_kernels_cases, "conv_c80": conv_c80_cases, "norms": norms_cases}


def child(family):
    import torch
    for label, bufs in FAMILIES[family]():
        torch.cuda.synchronize()
        for name, t in bufs.items():
            print("%s|%s|%s" % (label, name, hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()), flush=True)


def run(family, lib, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--family", family, "--child"], env=dict(os.environ, DS_LIB=lib),
                       stdout=subprocess.PIPE, text=True, timeout=timeout)
    if r.returncode:
        sys.exit("lib_equivalence: the run of %s exited with status %d" % (lib, r.returncode))
    return [tuple(line.split("|")) for line in r.stdout.splitlines() if line.count("|") == 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=sorted(FAMILIES))
    ap.add_argument("--child", action="store_true", help="(internal) run the cases with the library DS_LIB names and print the digests")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per library")
    ap.add_argument("-o", "--out", help="also write the listing to this file")
    ap.add_argument("libs", nargs="*", help="PARENT.so [NEW.so]: file names under diffusynth_amd/ (NEW defaults to the product build)")
    a = ap.parse_args()
    if a.child:
        return child(a.family)
    if not a.libs:
        ap.error("PARENT.so is required")
    old = run(a.family, a.libs[0], a.timeout)
    new = run(a.family, a.libs[1] if len(a.libs) > 1 else "libdiffusynth_hip.so", a.timeout)
    if [r[:2] for r in old] != [r[:2] for r in new]:
        sys.exit("lib_equivalence: the two libraries ran different cases")
    # one line per case: every buffer with the sha256 of the parent's bytes, then the verdict (the new library's digest where it differs)
    cases, bad, prev = {}, 0, {}
    for o, n in zip(old, new):
        bad += o[2] != n[2]
        same = o[2] == n[2] and prev.get(o[1]) == o[2]           # `^`: the digest this buffer has in the line above (both libraries)
        prev[o[1]] = o[2] if o[2] == n[2] else None
        cases.setdefault(o[0], []).append("%s=^" % o[1] if same else "%s=%s" % (o[1], o[2]) if o[2] == n[2] else "%s=%s!=%s" % (o[1], o[2], n[2]))
    lines = ["%s  %s  %s" % (c, " ".join(b), "!= parent" if any("!=" in x for x in b) else "== parent") for c, b in cases.items()]
    lines.append("# %d cases, %d written buffers, %d differ" % (len(cases), len(old), bad))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
