#!/usr/bin/env python3
"""Device time per launch of the row kernels (sampler_step.hip, window.hip, stft_window.hip) in their 16-byte form, through the C ABI:

    python tools/row_kernels_bench.py [--rounds 5] [--reps 50]          (DS_LIB=<library under diffusynth_amd/>, as tools/ab.sh -m rows sets it)

One line per figure, `rows <figure> us <median over the rounds of (time of reps launches in a row) / reps>`, at the shapes of the other
benches: rows of (4, 128, 64) at 1 and 64 rows for the step, guidance and edit kernels (guidance_bench.py, compose_bench.py,
edit_bench.py), W = 1024 with window 64 / stride 32 for the split and the blend (window_bench.py: 2 rows of n windows, H = 128) and
for the STFT blend (decode_bench.py: one looping row, F = 512, frames of scale 4).  The tables are the plain ones of a batcher tick:
CFG rows with a duplicate, step noise gathered from a draw."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def figures():
    """(name, launch closure) of every figure; the buffers live in the closures."""
    import torch
    from diffusynth_amd import _lib as L
    from diffusynth_amd.windowed import _Layout, window_plan
    st = L.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)                              # noqa: E731
    Cc, H, W = 4, 128, 64
    CHW = Cc * H * W
    out = []

    def add(name, entry, p, *more):
        out.append((name, lambda: L.call(entry, C.byref(p), *more, st)))

    for R in (1, 64):
        x, eu, ec, nz, o, hist = (rnd(R, Cc, H, W) for _ in range(6))
        e2 = torch.cat([eu, ec])
        cf = torch.rand(R, 5, device="cuda", generator=g) + 0.25
        add("ddim_step rows=%d" % R, "ds_ddim_step", L.StepParams(x=x.data_ptr(), eps=eu.data_ptr(), eps_cond=ec.data_ptr(), noise=nz.data_ptr(), out=o.data_ptr(),
                                                                   coef=cf.data_ptr(), cfg_scale=3.0, blend_mode=0, B=R, CHW=CHW, HW=H * W))
        add("dpm_step rows=%d" % R, "ds_dpm_step", L.DpmStepParams(x=x.data_ptr(), eps=eu.data_ptr(), eps_cond=ec.data_ptr(), hist=hist.data_ptr(), out=o.data_ptr(),
                                                                  coef=cf.data_ptr(), cfg_scale=3.0, blend_mode=0, B=R, C=Cc, H=H, W=W))
        # a tick's table: row r steps x[r] with eps (r, R + r) into out[r] and its CFG duplicate out[R + r]
        S = L.SR
        ir = torch.zeros(R, S["DS_SR_NI"], dtype=torch.int32)
        fr = torch.zeros(R, S["DS_SR_NF"])
        pr = torch.zeros(R, S["DS_SR_NP"], dtype=torch.int64)
        r_ = torch.arange(R, dtype=torch.int32)
        ir[:, S["DS_SR_X"]], ir[:, S["DS_SR_EPS"]], ir[:, S["DS_SR_EPSC"]], ir[:, S["DS_SR_OUT"]], ir[:, S["DS_SR_DUP"]] = r_, r_, R + r_, r_, R + r_
        ir[:, S["DS_SR_NOISE"]], ir[:, S["DS_SR_SAMPLE"]], ir[:, S["DS_SR_DRAW_ROWS"]], ir[:, S["DS_SR_DRAW_W"]] = 1, r_, R, W
        fr[:, :5], fr[:, S["DS_SR_CFG"]] = cf.cpu(), 3.0
        pr[:, S["DS_SR_DRAW"]] = nz.data_ptr()
        o2, cols = torch.empty(2 * R, Cc, H, W, device="cuda"), torch.arange(W, dtype=torch.int32, device="cuda")
        hr = torch.tensor([hist[r].data_ptr() for r in range(R)], dtype=torch.int64).cuda()
        irn = ir.clone()
        irn[:, S["DS_SR_NOISE"]] = 0
        t = [v.cuda() for v in (ir, fr, pr, irn)]
        add("step_rows rows=%d" % R, "ds_step_rows", L.StepRowsParams(x=x.data_ptr(), eps=e2.data_ptr(), out=o2.data_ptr(), irow=t[0].data_ptr(), frow=t[1].data_ptr(),
                                                                      prow=t[2].data_ptr(), cols=cols.data_ptr(), R=R, C=Cc, H=H, W=W, Bx=R, Beps=2 * R, Bout=2 * R, n_cols=W))
        add("dpm_step_rows rows=%d" % R, "ds_dpm_step_rows", L.StepRowsParams(x=x.data_ptr(), eps=e2.data_ptr(), out=o2.data_ptr(), irow=t[3].data_ptr(), frow=t[1].data_ptr(),
                                                                              prow=t[2].data_ptr(), cols=None, R=R, C=Cc, H=H, W=W, Bx=R, Beps=2 * R, Bout=2 * R, n_cols=0), hr.data_ptr())
        Q = L.QS
        iq, fq, pq = torch.zeros(R, Q["DS_QS_NI"], dtype=torch.int32), torch.rand(R, Q["DS_QS_NF"]) + 0.1, torch.zeros(R, Q["DS_QS_NP"], dtype=torch.int64)
        iq[:, Q["DS_QS_SRC"]], iq[:, Q["DS_QS_OUT"]], iq[:, Q["DS_QS_DUP"]], iq[:, Q["DS_QS_NOISE"]] = r_, r_, R + r_, 1
        iq[:, Q["DS_QS_SAMPLE"]], iq[:, Q["DS_QS_DRAW_ROWS"]], iq[:, Q["DS_QS_DRAW_W"]] = r_, R, W
        pq[:, Q["DS_QS_DRAW"]] = nz.data_ptr()
        tq = [v.cuda() for v in (iq, fq, pq)]
        add("q_sample_rows rows=%d" % R, "ds_q_sample_rows", L.QSampleRowsParams(x0=x.data_ptr(), out=o2.data_ptr(), irow=tq[0].data_ptr(), frow=tq[1].data_ptr(),
                                                                                 prow=tq[2].data_ptr(), cols=cols.data_ptr(), R=R, C=Cc, H=H, W=W, Bx0=R, Bout=2 * R, n_cols=W))
        E = L.EN
        ie, fe, pe = torch.zeros(R, E["DS_EN_NI"], dtype=torch.int32), torch.zeros(R, E["DS_EN_NF"]), torch.zeros(R, E["DS_EN_NP"], dtype=torch.int64)
        ie[:, E["DS_EN_X"]], ie[:, E["DS_EN_PREV"]], ie[:, E["DS_EN_EPS"]], ie[:, E["DS_EN_EPSC"]], ie[:, E["DS_EN_OUT"]] = r_, R + r_, r_, R + r_, r_
        fe[:, :5], fe[:, E["DS_EN_CFG"]] = cf.cpu(), 3.0
        te = [v.cuda() for v in (ie, fe, pe)]
        x2 = torch.cat([x, hist])
        add("edit_noise_rows rows=%d" % R, "ds_edit_noise_rows", L.EditNoiseRowsParams(X=x2.data_ptr(), eps=e2.data_ptr(), z=o.data_ptr(), irow=te[0].data_ptr(),
                                                                                       frow=te[1].data_ptr(), prow=te[2].data_ptr(), R=R, C=Cc, H=H, W=W, Bx=2 * R, Beps=2 * R, Bz=R))
        add("cfg_rescale rows=%d" % R, "ds_cfg_rescale", L.CfgRescaleParams(eps_u=eu.data_ptr(), eps_c=ec.data_ptr(), out=o.data_ptr(), gain=None, cfg_scale=6.0, phi=0.7, B=R, CHW=CHW))
        e3 = torch.cat([eu, ec, o])
        ic = torch.stack([r_, R + r_, 2 * R + r_], 1).contiguous().cuda()
        fc = torch.tensor([[6.0, 0.7]] * R).cuda()
        add("cfg_rescale_rows rows=%d" % R, "ds_cfg_rescale_rows", L.CfgRescaleRowsParams(eps=e3.data_ptr(), irow=ic.data_ptr(), frow=fc.data_ptr(), gain=None, R=R, CHW=CHW, Beps=3 * R))
        K = 2
        ck, wt = rnd(K, R, Cc, H, W), torch.rand(K, device="cuda", generator=g)
        add("cfg_compose K=2 rows=%d" % R, "ds_cfg_compose", L.CfgComposeParams(eps_u=eu.data_ptr(), eps_c=ck.data_ptr(), wt=wt.data_ptr(), out=o.data_ptr(), gain=None,
                                                                                cfg_scale=6.0, phi=0.7, B=R, K=K, CHW=CHW, W=W, wt_w=1))
        e4 = torch.cat([eu, ck.reshape(K * R, Cc, H, W), o])
        icc = torch.stack([r_, 3 * R + r_, torch.full_like(r_, K), R + r_, torch.full_like(r_, R), torch.zeros_like(r_), torch.ones_like(r_)], 1).contiguous().cuda()
        add("cfg_compose_rows K=2 rows=%d" % R, "ds_cfg_compose_rows", L.CfgComposeRowsParams(eps=e4.data_ptr(), irow=icc.data_ptr(), frow=fc.data_ptr(), wt=wt.data_ptr(), gain=None,
                                                                                              R=R, CHW=CHW, W=W, Beps=4 * R, n_wt=K))
        pairs = torch.stack([r_, R + r_], 1).contiguous().cuda()
        out.append(("copy_rows rows=%d" % R, lambda b=o2, p=pairs, R=R: L.call("ds_copy_rows", b.data_ptr(), p.data_ptr(), R, CHW, 2 * R, st)))
        out[-1][1].keep = (x, eu, ec, nz, o, hist, e2, cf, t, o2, cols, hr, tq, te, x2, e3, ic, fc, ck, wt, e4, icc, pairs)

    Wl, window, stride = 1024, 64, 32
    plan = window_plan(Wl, window, stride, False)
    lay = _Layout(plan, 2, True, None)
    x, xw = rnd(2, Cc, H, Wl), torch.empty(lay.Rw, Cc, H, window, device="cuda")
    rows, erow = torch.from_numpy(lay.rows).cuda(), torch.from_numpy(lay.erow).cuda()
    tables = lambda pl: (torch.from_numpy(np.ascontiguousarray(np.stack([pl.win.T, pl.col.T], axis=2))).cuda(),      # noqa: E731
                         torch.from_numpy(np.ascontiguousarray(pl.coef.T)).cuda())
    wcol, wcoef = tables(plan)
    mo = torch.empty(2, Cc, H, Wl, device="cuda")
    add("window_split W=1024", "ds_window_split", L.WindowSplitParams(x=x.data_ptr(), out=xw.data_ptr(), rows=rows.data_ptr(), R=lay.Rw, C=Cc, H=H, W=Wl, w=window, Bx=2, Bout=lay.Rw))
    add("window_merge W=1024", "ds_window_merge", L.WindowMergeParams(eps=xw.data_ptr(), out=mo.data_ptr(), erow=erow.data_ptr(), wcol=wcol.data_ptr(), wcoef=wcoef.data_ptr(),
                                                                      R=2, n=plan.n, C=Cc, H=H, W=Wl, w=window, Beps=lay.Rw, Bout=2))
    F, UP = 512, 4
    lplan, fplan = window_plan(Wl, window, stride, True), window_plan(UP * Wl, UP * window, UP * stride, True)
    llay = _Layout(lplan, 1, False, None)
    fcol, fcoef = tables(fplan)
    encw = torch.rand(lplan.n, 3, F, UP * window, device="cuda", generator=g) * 2 - 1
    encw[:, 0] = encw[:, 0].abs() * 4
    so, lerow = torch.empty(1, 3, F, UP * Wl, device="cuda"), torch.from_numpy(llay.erow).cuda()
    add("stft_window_merge W=1024", "ds_stft_window_merge", L.StftWindowMergeParams(encw=encw.data_ptr(), out=so.data_ptr(), erow=lerow.data_ptr(), wcol=fcol.data_ptr(),
                                                                                   wcoef=fcoef.data_ptr(), R=1, n=fplan.n, F=F, T=UP * Wl, w=UP * window, Bw=lplan.n, Bout=1))
    out[-1][1].keep = (x, xw, rows, erow, wcol, wcoef, mo, fcol, fcoef, encw, so, lerow)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    import torch
    figs = figures()
    us = {name: [] for name, _ in figs}
    for r in range(a.rounds + 1):                         # (round 0: warm-up)
        for name, fn in figs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                us[name].append(1e3 * e0.elapsed_time(e1) / a.reps)
    for name, _ in figs:
        print("rows %-32s us %.2f" % (name, float(np.median(us[name]))), flush=True)


if __name__ == "__main__":
    main()
