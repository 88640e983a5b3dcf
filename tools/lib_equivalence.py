#!/usr/bin/env python3
"""Bit equality of two builds of the library on one device: python tools/lib_equivalence.py --family attn_bf16 PARENT.so [NEW.so] [-o FILE]

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


FAMILIES = {"attn_bf16": attn_bf16_cases}


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
