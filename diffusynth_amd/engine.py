"""Host-side execution plan of the U-Net forward pass (Python over the C ABI).

``UnetEngine`` packs the module's parameters once (GroupNorm gains folded into the packed
convolution weights, border-class shift tables, stacked conditioning matrices) and, per input
shape, builds a *plan*: a flat list of pre-bound C-ABI calls whose activation buffers are
carved at plan time from one arena (first-fit with explicit lifetimes, so the working set
stays small and hot in L2 / Infinity Cache).  Running a plan is a loop of ctypes calls on the
caller's current HIP stream — no allocation, no synchronisation, HIP-graph capturable.

Graph: model/diffusion.py:187-258.  Blocks: model/diffusion_components.py (cited per method).
"""
import ctypes as C
import os

import torch

from . import _lib as L

_ESIZE = {L.DS_F32: 4, L.DS_BF16: 2}
_TDT = {L.DS_F32: torch.float32, L.DS_BF16: torch.bfloat16}
KSPLIT_FILL = 256        # split K until this many blocks exist (256 CUs)


def _up(x, m):
    return (x + m - 1) // m * m


class _Arena:
    """Plan-time first-fit allocator over byte offsets (256-B aligned)."""

    def __init__(self):
        self.free = [[0, 1 << 62]]
        self.peak = 0

    def alloc(self, nbytes):
        nbytes = _up(max(int(nbytes), 1), 256)
        for seg in self.free:
            if seg[1] - seg[0] >= nbytes:
                off = seg[0]
                seg[0] += nbytes
                if seg[0] == seg[1]:
                    self.free.remove(seg)
                self.peak = max(self.peak, off + nbytes)
                return off, nbytes
        raise MemoryError("arena exhausted")

    def release(self, off, nbytes):
        self.free.append([off, off + nbytes])
        self.free.sort()
        merged = []
        for s in self.free:
            if merged and merged[-1][1] >= s[0]:
                merged[-1][1] = max(merged[-1][1], s[1])
            else:
                merged.append(s)
        self.free = merged


class _Act:
    """Channels-last activation [B][H][W][C] living at arena offset ``off``."""
    __slots__ = ("off", "nbytes", "C", "H", "W", "stats", "split", "planes")

    def __init__(self, off, nbytes, Cc, H, W):
        self.off, self.nbytes, self.C, self.H, self.W, self.stats = off, nbytes, Cc, H, W, None
        self.split = False       # split-precision tier: the buffer holds 2C bf16 channels per pixel (hi plane, lo plane), not C fp32
        self.planes = None       # ... or a second activation holding this tensor in that form (written by the producer for a Down / Upsample)


class _ConvW:
    """Packed convolution: weights (+ optional GroupNorm fold tables) for one tile family."""
    __slots__ = ("w", "bias", "t1", "t2", "ncls", "Cout", "cout_pad", "cin_pad", "cin_real", "KH", "KW", "bn", "transposed", "k_order",
                 "res_steps", "res_bias", "w_fused", "w_quad", "quad_cout_pad", "w_split", "w_n16", "w_x3", "x3_cout_pad", "w_init7", "w_f32n4", "w_init7x3")


def split3_weight(w, gamma=None):
    """[Cout][C][kh][kw] fp32 (times the GroupNorm gain per input channel) as the 3C-input-channel weight of the split-precision 3x3 kernel
    (DS_CONV_F_SPLIT_IN): per 32-channel source chunk c the three virtual chunks [W_hi_c | W_lo_c | W_hi_c] — the kernel multiplies the
    hi plane's chunk c with the first two (ONE staged halo serves both) and the lo plane's chunk c with the third.  W_hi = bf16(W),
    W_lo = W - W_hi (rounded to bf16 by the packer).  C must be a multiple of 32."""
    w = w.detach().float()
    if gamma is not None:
        w = w * gamma.detach().float().view(1, -1, 1, 1)
    hi = w.bfloat16().float()
    lo = w - hi
    Cout, Cin, kh, kw = w.shape
    assert Cin % 32 == 0, Cin
    hic, loc = hi.view(Cout, Cin // 32, 32, kh, kw), lo.view(Cout, Cin // 32, 32, kh, kw)
    return torch.stack([hic, loc, hic], 2).reshape(Cout, 3 * Cin, kh, kw).contiguous()


def pack_x3_1x1(w, gamma=None):
    """[Cout][Cin][1][1] fp32 (times the PreNorm gain per input channel) -> the operand of ds_conv1x1_x3:
    [chunk of 32 input channels][hi, lo][cout_pad][32] bf16, cout_pad = Cout rounded up to 96; hi = bf16(w), lo = bf16(w - hi)."""
    w = w.detach().float().reshape(w.shape[0], -1)
    if gamma is not None:
        w = w * gamma.detach().float().view(1, -1)
    Cout, Cin = w.shape
    cout_pad, ncc = _up(Cout, 96), _up(Cin, 32) // 32
    wp = torch.zeros(cout_pad, ncc * 32, dtype=torch.float32, device=w.device)
    wp[:Cout, :Cin] = w
    hi = wp.bfloat16()
    lo = (wp - hi.float()).bfloat16()
    planes = torch.stack([hi, lo], 0).view(2, cout_pad, ncc, 32).permute(2, 0, 1, 3)     # [chunk][plane][row][32]
    return planes.contiguous().view(-1), cout_pad


def to_split_planes(x_nhwc):
    """fp32 NHWC [..., C] -> bf16 [..., 2C]: the hi plane bf16(x), then the lo plane bf16(x - hi) (DS_CONV_F_SPLIT_IN input format)."""
    hi = x_nhwc.float().bfloat16()
    lo = (x_nhwc.float() - hi.float()).bfloat16()
    return torch.cat([hi, lo], -1).contiguous()


def pack_quad_weights(w, transposed, dtype=torch.bfloat16):
    """Weights of Conv2d(C, Cout, 4, 2, 1) / ConvTranspose2d(Cin, Cout, 4, 2, 1) as the quad tiles of DS_CONV_TILE_QUAD_HALO3
    (ds_conv_params.wk_order = 2): [chunk][tap t = 2a + b][cout_pad][32] with
      transposed (w [Cin][Cout][4][4]): chunk = Cin / 32 group, row phase * Cout + co (phase = 2 py + px) = w[ci][co][3 - py - 2a][3 - px - 2b];
      strided    (w [Cout][C][4][4]):   chunk = plane * (C / 32) + group (plane = 2 p + q), row co = w[co][ci][1 - p + 2a][1 - q + 2b].
    Returns (flat tensor, cout_pad)."""
    w = w.detach().float()
    if transposed:
        Cin, Cout = w.shape[:2]
        cc, cp = Cin // 32, 4 * Cout
        out = torch.zeros(cc, 4, cp, 32, device=w.device)
        for ph in range(4):
            py, px = ph >> 1, ph & 1
            for t in range(4):
                a, b = t >> 1, t & 1
                m = w[:, :, 3 - py - 2 * a, 3 - px - 2 * b]                       # [Cin][Cout]
                out[:, t, ph * Cout:(ph + 1) * Cout, :] = m.t().reshape(Cout, cc, 32).permute(1, 0, 2)
    else:
        Cout, Cin = w.shape[:2]
        cc, cp = Cin // 32, _up(Cout, 96)
        out = torch.zeros(4, cc, 4, cp, 32, device=w.device)
        for par in range(4):
            p_, q_ = par >> 1, par & 1
            for t in range(4):
                a, b = t >> 1, t & 1
                m = w[:, :, 1 - p_ + 2 * a, 1 - q_ + 2 * b]                       # [Cout][Cin]
                out[par, :, t, :Cout, :] = m.reshape(Cout, cc, 32).permute(1, 0, 2)
    return out.reshape(-1).to(dtype).contiguous(), cp


class _EngineBase:
    """Shared by the U-Net and the VQGAN-decoder engines: dtype bookkeeping and weight packing."""

    def _init_common(self, module, compute_dtype):
        L.load()
        self.m = module
        self.dt = L.DS_BF16 if compute_dtype == "bf16" else L.DS_F32
        # "bf16x3": the fp32 tier (fp32 tensors and kernels) whose 3x3 convolutions run on the bf16 matrix cores in split precision
        # (x_hi w_hi + x_lo w_hi + x_hi w_lo, fp32 accumulate; conv3x3_halo3.hip, DS_CONV_F_*)
        self.split3 = compute_dtype == "bf16x3"
        self.es = _ESIZE[self.dt]
        self.vec = 16 // self.es
        self.dev = next(module.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("parameters must live on a HIP device ('cuda'); diffusynth_amd has no CPU path")
        self.plans = {}
        self._keep = []          # packed tensors
        self.side_stream = None
        self._tb_total = 0
        self._lab_total = 0
        self._pack_tmp = []      # packing inputs kept alive until _pack_done(): ONE stream sync per model, not one per tensor

    def _pack_done(self):
        torch.cuda.current_stream(self.dev).synchronize()
        self._pack_tmp = []

    # ------------------------------------------------------------------ plan cache: bounded, ONE arena for every shape
    # A plan is a list of pre-bound C calls over buffers carved from an arena.  Serving variable-width notes
    # (text2sound.py:84, track_maker.py:245) and CFG (B and 2B) creates many (B, H, W, cond) keys; each used to keep its own
    # arena forever (1.1 GB at B = 16).  Now all plans of an engine live in ONE arena sized to the largest peak seen, at
    # most DS_MAX_PLANS (default 8) plans are kept (least recently used evicted), and growing the arena drops the cached
    # plans (they hold absolute addresses; rebuilding one is a few ms of Python).  Consequence, as before: forward() is
    # single-stream and not re-entrant per model instance — two plans share the same bytes.
    def _cached_plan(self, key, make):
        import collections
        import os
        if not isinstance(self.plans, collections.OrderedDict):
            self.plans = collections.OrderedDict(self.plans)
            self._arena, self._arena_base, self._arena_bytes = None, 0, 0
            self._max_plans = max(1, int(os.environ.get("DS_MAX_PLANS", "8")))
        plan = self.plans.get(key)
        if plan is not None:
            self.plans.move_to_end(key)
            return plan
        dry = make()
        dry.build(0)
        peak = dry.arena.peak
        if peak > self._arena_bytes:
            # (the old arena may still be read by kernels in flight on this stream: the caching allocator keeps the block
            # alive until they retire, and every plan that pointed into it is dropped here)
            self.plans.clear()
            self._arena_bytes = int(max(peak, 1.25 * self._arena_bytes))
            self._arena = torch.empty(self._arena_bytes + 256, dtype=torch.uint8, device=self.dev)
            self._arena_base = _up(self._arena.data_ptr(), 256)
        plan = make()
        plan.build(self._arena_base)
        plan.ws = self._arena
        self.plans[key] = plan
        while len(self.plans) > self._max_plans:
            self.plans.popitem(last=False)
        return plan

    def _f32(self, t):
        return t.detach().to(device=self.dev, dtype=torch.float32).contiguous()

    def _pack_conv(self, weight, bias, cin_pad=None, gamma=None, beta=None, transposed=False, small_out=False, halo=False):
        """halo=True: the layer is a single-source 3x3 stride-1 convolution of a ConvNeXt block, i.e. it will run on the
        hand-scheduled LDS-halo kernel (bf16), whose weights are packed chunk-major (k_order 1)."""
        w = self._f32(weight)
        if transposed:
            Cin, Cout = w.shape[0], w.shape[1]
            KH = KW = 2
        else:
            Cout, Cin, KH, KW = w.shape
        cin_pad = Cin if cin_pad is None else cin_pad
        if small_out:
            bn = 32
        elif Cout % 192 == 0:
            bn = 192
        else:
            bn = 96
        cw = _ConvW()
        cw.Cout, cw.cout_pad, cw.cin_pad, cw.KH, cw.KW, cw.bn, cw.transposed = Cout, _up(Cout, bn), cin_pad, KH, KW, bn, transposed
        cw.cin_real = Cin
        cw.k_order = 1 if (halo and self.dt == L.DS_BF16 and KH == 3 and KW == 3 and not transposed and cin_pad % 32 == 0
                           and bn in (96, 192)) else 0
        n = L.load().ds_pack_conv_elems(cin_pad, KH, KW, cw.cout_pad, 1 if transposed else 0)
        cw.w = torch.empty(n, dtype=_TDT[self.dt], device=self.dev)
        g = self._f32(gamma) if gamma is not None else None
        pp = L.PackConvParams(w=w.data_ptr(), gamma=L.ptr(g), dst=cw.w.data_ptr(), dtype=self.dt, Cout=Cout, Cin=Cin,
                              cin_pad=cin_pad, KH=KH, KW=KW, cout_pad=cw.cout_pad, transposed=1 if transposed else 0, k_order=cw.k_order)
        L.call("ds_pack_conv_weight", C.byref(pp), L.current_stream())
        cw.bias = self._f32(bias) if bias is not None else None
        cw.res_steps, cw.res_bias, cw.w_fused = 0, None, None
        cw.w_quad, cw.quad_cout_pad = None, 0
        cw.w_split = None
        cw.w_n16 = None
        cw.w_init7 = None
        cw.w_f32n4 = None
        cw.w_x3, cw.x3_cout_pad = None, 0
        if (self.dt == L.DS_F32 and gamma is None and KH == 3 and KW == 3 and not transposed and Cout <= 4 and cin_pad == Cin
                and Cin % 32 == 0):
            # few-output 3x3 of the fp32 / split-precision tiers (the final 96 -> 4 convolution): vector-ALU kernel, weights through scalar loads
            cw.w_f32n4 = torch.empty(L.load().ds_conv3x3_f32_n4_weight_floats(Cin), dtype=torch.float32, device=self.dev)
            L.call("ds_pack_conv3x3_f32_n4", w.data_ptr(), L.ptr(cw.bias), Cout, Cin, cw.w_f32n4.data_ptr(), L.current_stream())
        if self.split3 and KH == 1 and KW == 1 and not transposed and cin_pad == Cin and Cin % 32 == 0 and Cout % 8 == 0:
            # 1x1 convolutions of the split-precision tier (to_qkv, to_out, res_conv): pre-split weights for ds_conv1x1_x3
            cw.w_x3, cw.x3_cout_pad = pack_x3_1x1(weight.to(self.dev), gamma.to(self.dev) if gamma is not None else None)
        if (self.dt == L.DS_BF16 and gamma is None and KH == 3 and KW == 3 and not transposed and Cout <= 16
                and cin_pad == Cin and Cin % 32 == 0):
            # few-output 3x3 (the final 96 -> 4 convolution): chunk-major tiles with 16 output rows for conv3x3_smalln.hip
            n16 = L.load().ds_pack_conv_elems(Cin, 3, 3, 16, 0)
            cw.w_n16 = torch.empty(n16, dtype=torch.bfloat16, device=self.dev)
            pp16 = L.PackConvParams(w=w.data_ptr(), gamma=None, dst=cw.w_n16.data_ptr(), dtype=L.DS_BF16, Cout=Cout, Cin=Cin, cin_pad=Cin, KH=3, KW=3,
                                    cout_pad=16, transposed=0, k_order=1)
            L.call("ds_pack_conv_weight", C.byref(pp16), L.current_stream())
        # (Cout % 8: the split-precision kernels store bf16-style 8-channel groups into a tensor sized for fp32 (channels rounded to 4))
        if halo and self.split3 and KH == 3 and KW == 3 and not transposed and cin_pad == Cin and Cin % 32 == 0 and cw.cout_pad % 96 == 0 and Cout % 8 == 0:
            ws = split3_weight(weight, gamma)                                     # [Cout][3 Cin][3][3] fp32: per chunk W_hi | W_lo | W_hi (gain folded)
            ns = L.load().ds_pack_conv_elems(3 * Cin, 3, 3, cw.cout_pad, 0)
            cw.w_split = torch.empty(ns, dtype=torch.bfloat16, device=self.dev)
            pps = L.PackConvParams(w=ws.data_ptr(), gamma=None, dst=cw.w_split.data_ptr(), dtype=L.DS_BF16, Cout=Cout, Cin=3 * Cin,
                                   cin_pad=3 * Cin, KH=3, KW=3, cout_pad=cw.cout_pad, transposed=0, k_order=1)
            L.call("ds_pack_conv_weight", C.byref(pps), L.current_stream())
            self._pack_tmp.append(ws)
        wshape = tuple(weight.shape)
        if ((self.dt == L.DS_BF16 or (self.split3 and Cout % 8 == 0)) and gamma is None and cin_pad == Cin and Cin % 32 == 0 and wshape[2:] == (4, 4)
                and ((transposed and (Cin // 32) % 6 == 0 and Cout % 96 == 0) or (not transposed and (Cin // 32) % 3 == 0))):
            # Downsample / Upsample of the U-Net: also packed as quad tiles for the halo kernel (conv_quad_halo3.hip); in the split-precision
            # tier as [W_hi | W_hi | W_lo] over 3 Cin input channels (the kernel then reads hi / lo planes: DS_CONV_F_SPLIT_IN)
            wq = weight
            if self.split3:
                w32 = weight.detach().float()
                hi = w32.bfloat16().float()
                wq = torch.cat([hi, hi, w32 - hi], 0 if transposed else 1)
            cw.w_quad, cw.quad_cout_pad = pack_quad_weights(wq, transposed)
        cw.t1 = cw.t2 = None
        cw.ncls = 1
        if gamma is not None:
            cw.ncls = 9 if KH == 3 else 1
            cw.t1 = torch.empty(cw.ncls * Cout, dtype=torch.float32, device=self.dev)
            cw.t2 = torch.empty(cw.ncls * Cout, dtype=torch.float32, device=self.dev)
            b = self._f32(beta)
            L.call("ds_conv_fold_tables", w.data_ptr(), L.ptr(cw.bias), g.data_ptr(), b.data_ptr(), Cout, Cin, KH, KW,
                   cw.t1.data_ptr(), cw.t2.data_ptr(), L.current_stream())
            self._keep += [g, b]
        self._pack_tmp += [w, g]
        return cw


class UnetEngine(_EngineBase):
    use_cfg_pair = True      # shared prefix of a classifier-free-guidance batch computed once (tests switch it off to compare)

    def __init__(self, module, compute_dtype="fp32"):
        self._init_common(module, compute_dtype)
        self.cfg = module.config
        with torch.cuda.device(self.dev):
            self._pack()
            self._pack_done()

    # ================================================================== packing
    def _pack_block(self, blk, dim):
        d = {}
        if self.cfg["use_convnext"]:
            C_ = blk.ds_conv.weight.shape[0]
            dw = torch.empty(49 * C_, dtype=torch.float32, device=self.dev)
            w = self._f32(blk.ds_conv.weight)
            L.call("ds_pack_dw_weight", w.data_ptr(), C_, dw.data_ptr(), L.current_stream())
            self._pack_tmp.append(w)
            d["dw"], d["dw_bias"] = dw, self._f32(blk.ds_conv.bias)
            d["dw_exp"] = None
            if self.dt == L.DS_BF16 and C_ % 32 == 0:
                we = torch.empty(C_ * 6 * 64 * 8, dtype=torch.bfloat16, device=self.dev)
                L.call("ds_pack_dw_weight_mfma", w.data_ptr(), C_, we.data_ptr(), L.current_stream())
                d["dw_exp"] = we
            n0, c1, n3, c4 = blk.net[0], blk.net[1], blk.net[3], blk.net[4]
            d["conv1"] = self._pack_conv(c1.weight, c1.bias, gamma=n0.weight, beta=n0.bias, halo=True)
            d["conv2"] = self._pack_conv(c4.weight, c4.bias, gamma=n3.weight, beta=n3.bias, halo=True)
            d["dim"], d["dim_out"] = C_, c4.weight.shape[0]
        else:
            b1, b2 = blk.block1, blk.block2
            d["conv1"] = self._pack_conv(b1.proj.weight, b1.proj.bias)
            d["conv2"] = self._pack_conv(b2.proj.weight, b2.proj.bias, halo=True)      # (conv1 may read pad_and_concat: generic kernel)
            d["n1"] = (self._f32(b1.norm.weight), self._f32(b1.norm.bias))
            d["n2"] = (self._f32(b2.norm.weight), self._f32(b2.norm.bias))
            d["dim"], d["dim_out"] = b1.proj.weight.shape[1], b1.proj.weight.shape[0]
        d["res"] = None
        if isinstance(blk.res_conv, torch.nn.Conv2d):
            d["res"] = self._pack_conv(blk.res_conv.weight, blk.res_conv.bias)
            c2 = d["conv2"]
            cx = blk.res_conv.weight.shape[1]
            if c2.k_order == 1 and cx % 96 == 0:      # (the fused steps come in threes: the weight ring's phase)
                # components:128,139 fused into conv2's launch: the 1x1 tiles ([cx/32][cout_pad][32]) precede the 3x3 tiles
                # (a second copy: the unfused fallback — split-K at small batch — keeps reading cw.w)
                w = self._f32(blk.res_conv.weight)
                n = L.load().ds_pack_conv_elems(cx, 1, 1, c2.cout_pad, 0)
                rpk = torch.empty(n, dtype=_TDT[self.dt], device=self.dev)
                pp = L.PackConvParams(w=w.data_ptr(), gamma=None, dst=rpk.data_ptr(), dtype=self.dt, Cout=c2.Cout, Cin=cx, cin_pad=cx, KH=1, KW=1,
                                      cout_pad=c2.cout_pad, transposed=0, k_order=1)
                L.call("ds_pack_conv_weight", C.byref(pp), L.current_stream())
                c2.w_fused = torch.cat([rpk, c2.w])
                c2.res_steps, c2.res_bias = cx // 32, d["res"].bias
                self._pack_tmp.append(w)
        d["tb_off"] = None
        if getattr(blk, "mlp", None) is not None:
            d["tb_off"] = self._tb_total
            self._tb_w.append(self._f32(blk.mlp[1].weight))
            self._tb_b.append(self._f32(blk.mlp[1].bias))
            self._tb_total += blk.mlp[1].weight.shape[0]
        return d

    def _pack_attn(self, res):
        pre, a = res.fn, res.fn.fn
        d = {"C": a.to_qkv.weight.shape[1]}
        d["qkv"] = self._pack_conv(a.to_qkv.weight, None, gamma=pre.norm.weight, beta=pre.norm.bias)
        d["out"] = self._pack_conv(a.to_out[0].weight, a.to_out[0].bias)
        d["on"] = (self._f32(a.to_out[1].weight), self._f32(a.to_out[1].bias))
        d["l_off"] = self._lab_total
        d["fused"] = None
        Cc = d["C"]
        if self.dt == L.DS_BF16 and self.cfg["attn_type"] == "linear_add" and Cc in (96, 192, 384):
            wq = self._f32(a.to_qkv.weight).reshape(384, Cc).contiguous()
            wo = self._f32(a.to_out[0].weight).reshape(Cc, 128).contiguous()
            g = self._f32(pre.norm.weight)
            wq16 = torch.empty(384 * Cc, dtype=torch.bfloat16, device=self.dev)
            wo16 = torch.empty(Cc * 128, dtype=torch.bfloat16, device=self.dev)
            L.call("ds_pack_attn_fused", wq.data_ptr(), g.data_ptr(), wo.data_ptr(), wq16.data_ptr(), wo16.data_ptr(), Cc, L.current_stream())
            self._pack_tmp += [wq, wo, g]
            d["fused"] = (wq16, wo16)
        d["x3"] = None
        if self.split3 and self.cfg["attn_type"] == "linear_add" and Cc in (96, 192, 384):
            # split-precision tier: the whole block on attn_x3.hip (no qkv tensor): to_qkv * PreNorm gain as hi / lo bf16 planes, to_out in fp32
            wq = self._f32(a.to_qkv.weight).reshape(384, Cc).contiguous()
            g = self._f32(pre.norm.weight)
            whl = torch.empty(2 * 384 * Cc, dtype=torch.bfloat16, device=self.dev)
            L.call("ds_pack_attn_x3", wq.data_ptr(), g.data_ptr(), whl.data_ptr(), Cc, L.current_stream())
            self._pack_tmp += [wq, g]
            d["x3"] = (whl, self._f32(a.to_out[0].weight).reshape(Cc, 128).contiguous())
        if self.cfg["attn_type"] == "linear_add":
            # label_key only shifts k by a constant over n, which softmax over n removes: not computed
            self._lab_w.append(self._f32(a.label_query.weight))
            self._lab_b.append(self._f32(a.label_query.bias))
            self._lab_total += a.label_query.weight.shape[0]
        else:
            self._lab_w += [self._f32(a.label_key.weight), self._f32(a.label_value.weight)]
            self._lab_b += [self._f32(a.label_key.bias), self._f32(a.label_value.bias)]
            self._lab_total += 2 * a.label_key.weight.shape[0]
        return d

    def _pack(self):
        m, cfg = self.m, self.cfg
        self._tb_w, self._tb_b, self._tb_total = [], [], 0
        self._lab_w, self._lab_b, self._lab_total = [], [], 0
        self.cin0 = _up(cfg["in_dim"], self.vec)
        P = {}
        P["init"] = self._pack_conv(m.init_conv.weight, m.init_conv.bias, cin_pad=self.cin0)
        w0 = m.init_conv.weight
        if (self.dt == L.DS_BF16 and tuple(w0.shape[2:]) == (7, 7) and w0.shape[0] == 96 and w0.shape[1] <= 4
                and self.cin0 in (4, 8)):
            # the init convolution on its own kernel: four real channels = 8 bytes per pixel, a K step = one kernel row read straight from a halo
            wf = self._f32(w0)
            w7 = torch.empty(L.load().ds_conv7x7_c4_weight_elems(), dtype=torch.bfloat16, device=self.dev)
            L.call("ds_pack_conv7x7_c4", wf.data_ptr(), 96, int(w0.shape[1]), w7.data_ptr(), L.current_stream())
            self._pack_tmp.append(wf)
            P["init"].w_init7 = w7
        P["init"].w_init7x3 = None
        if (self.split3 and tuple(w0.shape[2:]) == (7, 7) and w0.shape[0] == 96 and w0.shape[1] <= 4 and self.cin0 == 4):
            # split-precision tier: the same kernel with the fp32 input split into hi / lo bf16 on its way to LDS, fp32 output
            wf = self._f32(w0)
            w7 = torch.empty(2 * L.load().ds_conv7x7_c4_weight_elems(), dtype=torch.bfloat16, device=self.dev)
            L.call("ds_pack_conv7x7_c4_x3", wf.data_ptr(), 96, int(w0.shape[1]), w7.data_ptr(), L.current_stream())
            self._pack_tmp.append(wf)
            P["init"].w_init7x3 = w7
        P["downs"] = []
        for blk1, at1, blk2, at2, down in m.downs:
            P["downs"].append((self._pack_block(blk1, None), self._pack_attn(at1), self._pack_block(blk2, None),
                               self._pack_attn(at2), self._pack_conv(down.weight, down.bias)))
        P["mid_left"] = [self._pack_block(b, None) for b in m.mid_left]
        P["mid_mid"] = (self._pack_block(m.mid_mid[0], None), self._pack_attn(m.mid_mid[1]), self._pack_block(m.mid_mid[2], None))
        P["mid_right"] = [self._pack_block(b, None) for b in m.mid_right]
        P["ups"] = []
        for b1, a1, up, b2, a2, b3, a3 in m.ups:
            P["ups"].append((self._pack_block(b1, None), self._pack_attn(a1),
                             self._pack_conv(up.weight, up.bias, transposed=True),
                             self._pack_block(b2, None), self._pack_attn(a2), self._pack_block(b3, None), self._pack_attn(a3)))
        P["final_block"] = self._pack_block(m.final_conv[0], None)
        fc = m.final_conv[1]
        P["final"] = self._pack_conv(fc.weight, fc.bias, small_out=True)
        self.P = P
        # conditioning matrices
        if m.time_mlp is not None:
            half = cfg["down_dims"][0] // 2
            import math
            self.freqs = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1))).to(self.dev)
            self.tm1 = (self._f32(m.time_mlp[1].weight), self._f32(m.time_mlp[1].bias))
            self.tm3 = (self._f32(m.time_mlp[3].weight), self._f32(m.time_mlp[3].bias))
            self.tb_W = torch.cat(self._tb_w, 0).contiguous() if self._tb_w else None
            self.tb_b = torch.cat(self._tb_b, 0).contiguous() if self._tb_b else None
        emb = m.label_embedding.embedding
        self.emb_is_linear = isinstance(emb, torch.nn.Linear)
        self.emb_w = self._f32(emb.weight)
        self.emb_b = self._f32(emb.bias) if self.emb_is_linear else None
        self.lab_W = torch.cat(self._lab_w, 0).contiguous()
        self.lab_b = torch.cat(self._lab_b, 0).contiguous()
        self.label_dim = cfg["label_emb_dim"]

    # ================================================================== plan
    def _plan(self, B, H, W, has_cond, paired=False):
        key = (B, H, W, has_cond) if not paired else (B, H, W, has_cond, "paired")
        return self._cached_plan(key, lambda: _PlanBuilder(self, B, H, W, has_cond, paired))

    def forward(self, x, time, condition, paired=False):
        """paired: the caller guarantees x[:B/2] == x[B/2:] and time[:B/2] == time[B/2:] (the doubled batch of classifier-free guidance,
        DiffSynthSampler.py:311-320): everything in front of the first operator that reads `condition` is computed once."""
        cfg = self.cfg
        assert x.dim() == 4 and x.shape[1] == cfg["in_dim"], "x must be (B, in_dim, H, W)"
        B, _, H, W = x.shape
        x = x.to(torch.float32).contiguous()
        time = time.to(device=x.device, dtype=torch.int64).contiguous()
        cond = None
        if condition is not None:
            if self.emb_is_linear:
                cond = condition.to(device=x.device, dtype=torch.float32).contiguous()
            else:
                cond = self.emb_w[condition.to(x.device)].contiguous()     # nn.Embedding lookup (components:161)
        out = torch.empty((B, cfg["out_dim"], H, W), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            paired = bool(paired) and B % 2 == 0 and cond is not None and self.use_cfg_pair and cfg["use_convnext"]
            plan = self._plan(B, H, W, cond is not None, paired)
            if getattr(self, "hip_graph", False) and plan.prof is None and not L.lib_path().endswith("_bounds.so"):
                plan.run_graphed(x, time, cond, out)
            else:
                plan.run(x, time, cond, out)
        return out


class _PlanBuilder:
    def __init__(self, eng, B, H, W, has_cond, paired=False):
        self.e, self.B, self.H, self.W, self.has_cond = eng, B, H, W, has_cond
        self.alloc_B = 0         # > B only while a paired plan's shared prefix runs at half the batch (act(): tensors carved at full size)
        self.Btile = B           # the batch every split-K decision looks at: the FULL batch, also while the shared prefix of a paired (CFG)
        #                          plan runs at half of it — the prefix then adds its partial sums in the plain plan's order (same bits)
        self.paired = paired
        self.arena = _Arena()
        self.ops = []
        self.ws = None
        self.lib = L.load()
        self.conv_meta = {}      # op index -> (tile id, algorithmic FLOPs) for every ds_conv_igemm launch
        self.prof = None         # set to a list to collect (op index, start event, end event) per conv launch
        self.prof_every = 1      # ... on every prof_every-th run() only (the event pairs serialise the queue: ~6 % of a step)
        self.calls = 0

    # ---------------------------------------------------------------- arena helpers
    def act(self, Cc, H, W):
        # (alloc_B > B only while the shared prefix of a paired plan runs at half the batch: its tensors are carved at FULL size, so the
        # prefix's results are the first half of the full-batch tensors and dup() writes the second half only)
        off, n = self.arena.alloc(max(self.B, self.alloc_B) * H * W * Cc * self.e.es)
        return _Act(self.base + off, n, Cc, H, W)

    def raw(self, nbytes):
        off, n = self.arena.alloc(nbytes)
        return (self.base + off, n)

    def free(self, a):
        if isinstance(a, _Act):
            if a.nbytes:
                self.arena.release(a.off - self.base, a.nbytes)
            if a.stats is not None:
                self.free_raw(a.stats[0])
                a.stats = None
            if a.planes is not None:
                self.free(a.planes)
                a.planes = None
        else:
            self.free_raw(a)

    def free_raw(self, r):
        self.arena.release(r[0] - self.base, r[1])

    def op(self, name, *args):
        self.ops.append((getattr(self.lib, name), args, name))

    # ---------------------------------------------------------------- kernels
    def halo_ksplit(self, cw, H, W, Cin, ncc=None):
        """Split-K factor of a 3x3 halo launch: > 1 only when (patch x channel-tile x sample) blocks cannot fill the 256 CUs.
        One of the tiling decisions that look at the batch (the others: the split-K of Down / Upsample and conv1x1_x3, the attention
        segments), 16-bit tiers only; fp32 never splits (batch-invariant bit for bit).  The batch looked at is the plan's FULL batch
        (self.Btile), not the half batch of a paired plan's shared prefix."""
        B = self.Btile
        twl = 3
        while (1 << twl) < W and twl < 5:
            twl += 1
        tw_, th_ = 1 << twl, 256 >> twl
        pn = (-(-H // th_)) * (-(-W // tw_)) * (cw.cout_pad // 96)
        split = ncc is not None                          # split-precision launches: K slices = whole source chunks = 27 steps each
        ncc = Cin // 32 if ncc is None else ncc
        # the smallest factor that fills the chip, else the largest possible (r04: 3 and 6 — every channel count is a multiple of 96, so chunk
        # counts of 3, 9, 18 had no power-of-two slice: a 96 -> 192 layer at 256 x 64, batch 1, ran as 128 blocks of 81 steps)
        ok = [c for c in (2, 3, 4, 6, 8) if ncc % c == 0 and ncc // c >= (1 if split else 2)]
        if not split:      # (the bf16 tier gains nothing from the 3s: same-box A/B, batch 1 and 16)
            ok = [c for c in ok if c in (2, 4, 8)]
        ks = 1
        for c in ok:
            ks = c
            if pn * B * c >= KSPLIT_FILL:
                break
        if pn * B >= KSPLIT_FILL:
            ks = 1
        return ks

    def conv(self, cw, src0, src1=None, off1=(0, 0), stride=1, pad=0, gn_ab=None, act=L.ACT_NONE, res=None,
             want_stats=False, out=None, out_nchw_ptr=False, gn_src=None, res_fuse=None, out_split=False):
        """gn_src = (partials ptr, parts, count, eps): the consumer reduces the producer's statistics itself.
        res_fuse = (x0, x1, off1): run the block's 1x1 res_conv over pad_and_concat(x0, x1) inside this launch (HALO3 tile,
        weights packed with the res tiles appended; the caller checked halo_ksplit() == 1)."""
        if gn_src is not None:
            gn_ab = True
        e, B = self.e, self.B
        H, W = src0.H, src0.W
        if cw.transposed:
            Ho, Wo, oh, ow = H, W, 2 * H, 2 * W
        else:
            Ho = (H + 2 * pad - cw.KH) // stride + 1
            Wo = (W + 2 * pad - cw.KW) // stride + 1
            oh, ow = Ho, Wo
        C1 = src1.C if src1 is not None else 0
        assert src0.C + C1 == cw.cin_pad, (src0.C, C1, cw.cin_pad)
        if out is None:
            out = self.act(_up(cw.Cout, e.vec), oh, ow)
        # tile: BN family fixed by packing; BM halves on the small-spatial levels so the grid still fills the chip.
        # The TILE depends on the layer shape only, never on B.  In the fp32 tier nothing else looks at B either: a sample's result (incl.
        # its GroupNorm partial sums) does not change with the batch it is computed in (shard == unsharded, bit for bit).  The bf16 and
        # bf16x3 tiers additionally pick split-K (halo_ksplit and the quad / conv1x1_x3 / generic-kernel choices below, all from
        # self.Btile) and the attention kernel generation / segment count by B (ds_attn_fused_segments, ds_attn_x3_segments): there a
        # sample's result depends on its batch to the rounding of fp32 partial sums.
        if cw.k_order == 1:
            # chunk-major weights = a single-source 3x3 stride-1 pad-1 layer packed for the LDS-halo kernel (conv3x3_halo3.hip)
            assert src1 is None and stride == 1 and pad == 1 and src0.C % 32 == 0, "chunk-major weights reached a layer the halo kernel cannot run"
            tile = L.TILE_HALO3_256x96
        elif cw.bn == 192:
            tile = L.TILE_64x192 if Ho * Wo <= 1024 else L.TILE_128x192
        elif cw.bn == 96:
            tile = L.TILE_256x96
        else:
            tile = L.TILE_128x32
        if (cw.w_f32n4 is not None and src1 is None and stride == 1 and pad == 1 and res is None and gn_ab is None and not want_stats
                and not out_nchw_ptr and not src0.split and out.C == 4 and act == L.ACT_NONE and res_fuse is None):
            self.op("ds_conv3x3_f32_n4", src0.off, B, H, W, src0.C, cw.w_f32n4.data_ptr(), out.off)
            return out
        split = (cw.w_split is not None and src1 is None and stride == 1 and pad == 1 and not out_nchw_ptr and src0.split)
        quad = (cw.w_quad is not None and src1 is None and res is None and gn_ab is None and not out_nchw_ptr and (not src0.split or e.split3) and
                (cw.transposed or (stride == 2 and pad == 1 and H % 2 == 0 and W % 2 == 0)))
        p = L.ConvParams(src0=src0.off, src1=(src1.off if src1 is not None else None), C0=src0.C, C1=C1, H=H, W=W,
                         H1=(src1.H if src1 is not None else 0), W1=(src1.W if src1 is not None else 0),
                         off_h1=off1[0], off_w1=off1[1], wpk=cw.w.data_ptr(), Cout=cw.Cout, cout_pad=cw.cout_pad,
                         KH=cw.KH, KW=cw.KW, stride=stride, pad_h=pad, pad_w=pad, Ho=Ho, Wo=Wo,
                         transposed=1 if cw.transposed else 0, out=out.off,
                         out_C=out.C, out_c0=0, out_nchw_f32=0,
                         bias=L.ptr(cw.bias), gn_ab=(gn_ab if gn_src is None else None), fold_t1=L.ptr(cw.t1) if gn_ab else None,
                         fold_t2=L.ptr(cw.t2) if gn_ab else None, ncls=cw.ncls if gn_ab else 1, act=act,
                         res=(res.off if res is not None else None), stats_part=None, B=B, dtype=e.dt, tile=tile, wk_order=cw.k_order)
        if split:
            # split-precision 3x3: input = hi / lo bf16 planes (2C channels), output = planes again (conv1: feeds conv2) or fp32 (conv2)
            p.tile = tile = L.TILE_HALO3_256x96
            p.dtype, p.wpk, p.wk_order, p.C0 = L.DS_BF16, cw.w_split.data_ptr(), 1, 2 * src0.C
            p.flags = 1 | (2 if out_split else 4)
            p.out_C = 2 * out.C if out_split else out.C
            out.split = bool(out_split)
        if (cw.w_n16 is not None and src1 is None and stride == 1 and pad == 1 and res is None and gn_ab is None and not want_stats
                and not out_nchw_ptr and not src0.split):
            p.tile = tile = L.TILE_HALO3_N16
            p.wpk, p.cout_pad, p.wk_order = cw.w_n16.data_ptr(), 16, 1
        xsplit = None
        if quad:
            p.tile = tile = L.TILE_QUAD_HALO3
            p.wpk, p.cout_pad, p.wk_order = cw.w_quad.data_ptr(), cw.quad_cout_pad, 2
            if e.split3:
                # split-precision tier: the kernel reads hi / lo bf16 planes and writes fp32.  The planes come from the producer where it
                # wrote them (the attention block in front of a Down / Upsample, r04) — otherwise one streaming pass re-stores the fp32 input
                given = src0 if src0.split else getattr(src0, "planes", None)
                if given is None:
                    xsplit = self.act(src0.C, H, W)
                    self.op("ds_split_planes", src0.off, xsplit.off, B * H * W, src0.C)
                    given = xsplit
                elif not src0.split:
                    xsplit, src0.planes = given, None                      # (released after this launch)
                p.src0, p.C0, p.dtype, p.flags = given.off, 2 * src0.C, L.DS_BF16, 1 | 4
        if gn_src is not None:
            p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = gn_src[0], gn_src[1], float(gn_src[2]), gn_src[3]
        if res_fuse is not None:
            x0, x1, xoff = res_fuse
            assert tile == L.TILE_HALO3_256x96 and cw.res_steps == (x0.C + (x1.C if x1 is not None else 0)) // 32 and res is None
            p.res_src0, p.res_C0, p.res_steps, p.res_bias, p.wpk = x0.off, x0.C, cw.res_steps, L.ptr(cw.res_bias), cw.w_fused.data_ptr()
            if x1 is not None:
                p.res_src1, p.res_C1, p.res_H1, p.res_W1, p.res_off_h1, p.res_off_w1 = x1.off, x1.C, x1.H, x1.W, xoff[0], xoff[1]
        slab = None
        if tile == L.TILE_HALO3_256x96 and res_fuse is None:
            # (split-precision launches too since r04: three times the K steps per block — a 32 x 8-level layer at batch 1 was 8 blocks of
            # 648 serial steps; like the bf16 tier's, this decision looks at B: partial sums are added in a different order, nothing else)
            ks = self.halo_ksplit(cw, H, W, src0.C, src0.C // 32 if split else None)      # (K slices = whole source chunks = triples of virtual chunks)
            if ks > 1:
                slab = self.raw(ks * B * Ho * Wo * _up(cw.Cout, 8) * 4)
                p.ksplit, p.slab = ks, slab[0]
        elif tile == L.TILE_QUAD_HALO3:
            # Down / Upsample on the halo pipeline (r04): K slices of whole groups of six chunks (the kernel's loop period)
            twl = 3
            while (1 << twl) < Wo and twl < 5:
                twl += 1
            nblk = (-(-Ho // (256 >> twl))) * (-(-Wo // (1 << twl))) * (cw.quad_cout_pad // 96) * self.Btile
            nch = (1 if cw.transposed else 4) * ((3 * src0.C // 32) if e.split3 else src0.C // 32)
            ks = 1
            if nblk < KSPLIT_FILL:
                for c in ((2, 3, 4, 6, 8) if e.split3 else (2, 4, 8)):
                    if nch % c == 0 and (nch // c) % 6 == 0:
                        ks = c
                        if nblk * c >= KSPLIT_FILL:
                            break
            if ks > 1:
                slab = self.raw(ks * B * oh * ow * _up(cw.Cout, 8) * 4)
                p.ksplit, p.slab = ks, slab[0]
        elif e.dt == L.DS_BF16 and tile in (L.TILE_64x192, L.TILE_128x192, L.TILE_256x96):
            # same idea for the generic kernel (4x4 stride-2, transposed and 1x1 layers of the small-spatial levels):
            # their K loops are long (up to 192 steps) and their grids small
            bm_, bn_ = {L.TILE_64x192: (64, 192), L.TILE_128x192: (128, 192), L.TILE_256x96: (256, 96)}[tile]
            nblk = (-(-(Ho * Wo) // bm_)) * (cw.cout_pad // bn_) * self.Btile * (4 if cw.transposed else 1)
            nq = -(-((4 if cw.transposed else cw.KH * cw.KW) * (src0.C + C1)) // 32)
            ks = 1
            while ks < 8 and nblk * ks < 384 and nq // (ks * 2) >= 6:
                ks *= 2
            while ks > 1 and (ks - 1) * (-(-nq // ks)) >= nq:      # never an empty last slice (ceil(nq / ks) steps per slice)
                ks //= 2
            if ks > 1:
                slab = self.raw(ks * B * oh * ow * _up(cw.Cout, 8) * 4)
                p.ksplit, p.slab = ks, slab[0]
        if (cw.w_x3 is not None and stride == 1 and pad == 0 and not out_nchw_ptr and not src0.split and gn_src is None and act == L.ACT_NONE
                and src0.C % 32 == 0 and C1 % 32 == 0 and res_fuse is None and slab is None):
            # split-precision tier: 1x1 convolution of fp32 tensors as three bf16 MFMA products (conv1x1_x3.hip)
            p.dtype, p.flags, p.wpk, p.cout_pad, p.wk_order, p.tile = L.DS_BF16, 8 | 4, cw.w_x3.data_ptr(), cw.x3_cout_pad, 0, 0
            # K slices at small batches (r04): res_conv of a 64 x 16-level block at batch 1 was 16 blocks of 24 - 36 serial chunks
            nblk, nq, ks = (-(-(Ho * Wo) // 256)) * (cw.x3_cout_pad // 96) * self.Btile, (src0.C + C1) // 32, 1
            if nblk < KSPLIT_FILL:
                for c in (2, 3, 4, 6, 8):
                    if nq // c >= 3 and (c - 1) * (-(-nq // c)) < nq:
                        ks = c
                        if nblk * c >= KSPLIT_FILL:
                            break
            if ks > 1:
                slab = self.raw(ks * B * Ho * Wo * _up(cw.Cout, 8) * 4)
                p.ksplit, p.slab = ks, slab[0]
            if want_stats:
                parts = self.lib.ds_conv1x1_x3_stats_parts(C.byref(p))
                st = self.raw(B * parts * 2 * 4)
                p.stats_part = st[0]
                out.stats = (st, parts)
            self.op("ds_conv1x1_x3", p)
            if slab is not None:
                self.op("ds_conv_splitk_reduce", p)
                self.free_raw(slab)
            return out
        if want_stats:
            parts = self.lib.ds_conv_stats_parts(C.byref(p))
            st = self.raw(B * parts * 2 * 4)
            p.stats_part = st[0]
            out.stats = (st, parts)
        # algorithmic work of this launch: real taps x real channels (padding excluded)
        taps = 16 if cw.transposed else cw.KH * cw.KW
        cin_real = min(src0.C + C1, getattr(cw, "cin_real", src0.C + C1))
        flops = 2.0 * B * Ho * Wo * cw.Cout * taps * cin_real
        if res_fuse is not None:
            flops += 2.0 * B * Ho * Wo * cw.Cout * 32 * cw.res_steps
        self.conv_meta[len(self.ops)] = (tile, flops, f"{cw.KH}x{cw.KW}{'T' if cw.transposed else ''} {src0.C + C1}->{cw.Cout} @{Ho}x{Wo}"
                                         + (f" +1x1 {32 * cw.res_steps}" if res_fuse is not None else ""))
        self.op("ds_conv_igemm", p)
        if xsplit is not None:
            self.free(xsplit)
        if slab is not None:
            self.op("ds_conv_splitk_reduce", p)
            self.free_raw(slab)
        return out

    def dup(self, a):
        """Both halves of a full-batch activation = the half-batch activation ``a`` (incl. its GroupNorm partials); self.B is the full batch."""
        nb = (self.B // 2) * a.H * a.W * a.C * self.e.es
        # r05: `a` was carved at full size (act() while alloc_B is set) and holds the prefix in its first half: one read + one write
        assert a.nbytes >= 2 * nb, "dup() of a tensor not carved at the full batch"
        out = _Act(a.off, a.nbytes, a.C, a.H, a.W)
        out.split = getattr(a, "split", False)
        self.op("ds_dup_batch", a.off, a.off, nb)
        a.nbytes = 0                                  # (ownership of the bytes moved to `out`: free(a) releases nothing)
        if a.stats is not None:
            st, parts = a.stats
            ns = self.raw(self.B * parts * 2 * 4)
            self.op("ds_dup_batch", st[0], ns[0], (self.B // 2) * parts * 2 * 4)
            out.stats = (ns, parts)
        return out

    def finalize(self, a, count, eps=1e-5):
        """partials of activation ``a`` -> (rstd, rstd*mean) per sample; returns raw buffer."""
        st, parts = a.stats
        ab = self.raw(self.B * 2 * 4)
        self.op("ds_gn_finalize", st[0], self.B, parts, float(count), eps, ab[0])
        self.free_raw(st)
        a.stats = None
        return ab

    def stats_src(self, a, count, eps=1e-5):
        """Hand activation ``a``'s raw partials to the consumer: returns (gn_src tuple, raw buffer to free after use)."""
        st, parts = a.stats
        a.stats = None
        return (st[0], parts, count, eps), st

    def srcs(self, x):
        """x is an _Act or (enc, dec) pair to be read as pad_and_concat(enc, dec) (components:210-249)."""
        if isinstance(x, _Act):
            return x, None, (0, 0)
        enc, dec = x
        return enc, dec, ((enc.H - dec.H) // 2, (enc.W - dec.W) // 2)

    def convnext(self, d, x, want_stats):
        """components:107-139."""
        e, B = self.e, self.B
        s0, s1, off1 = self.srcs(x)
        H, W = s0.H, s0.W
        dim, dim_out = d["dim"], d["dim_out"]
        h = self.act(dim, H, W)
        p = L.DwconvParams(src0=s0.off, src1=(s1.off if s1 else None), C0=s0.C, C1=(s1.C if s1 else 0), H=H, W=W,
                           H1=(s1.H if s1 else 0), W1=(s1.W if s1 else 0), off_h1=off1[0], off_w1=off1[1],
                           wt=d["dw"].data_ptr(), bias=d["dw_bias"].data_ptr(),
                           tbias=(self.tb_all[0] + 4 * d["tb_off"]) if (d["tb_off"] is not None and self.tb_all) else None,
                           tb_stride=e._tb_total, out=h.off, stats_part=None, B=B, dtype=e.dt,
                           wexp=(d["dw_exp"].data_ptr() if d.get("dw_exp") is not None else None))
        # split-precision tier: the two tensors only 3x3 convolutions read (h, g) are stored as hi / lo bf16 planes
        sp = (d["conv1"].w_split is not None and d["conv2"].w_split is not None and s0.C % 16 == 0 and (s1 is None or s1.C % 16 == 0))
        if sp:
            p.out_split, h.split = 1, True
        parts = self.lib.ds_dwconv_stats_parts(C.byref(p))
        st = self.raw(B * parts * 2 * 4)
        p.stats_part = st[0]
        h.stats = (st, parts)
        self.op("ds_dwconv7", p)
        src1_, st1 = self.stats_src(h, dim * H * W)
        g = self.conv(d["conv1"], h, pad=1, gn_src=src1_, act=L.ACT_GELU, want_stats=True, out_split=sp)
        self.free(h)
        self.free_raw(st1)
        src2_, st2 = self.stats_src(g, d["conv1"].Cout * H * W)
        c2 = d["conv2"]
        if (d["res"] is not None and c2.res_steps and
                self.halo_ksplit(c2, H, W, g.C) == 1):
            out = self.conv(c2, g, pad=1, gn_src=src2_, want_stats=want_stats, res_fuse=(s0, s1, off1))
            self.free(g)
            self.free_raw(st2)
            return out
        if d["res"] is not None:
            out = self.conv(d["res"], s0, s1, off1)           # 1x1 res_conv straight into the output buffer
            res = out
        else:
            out, res = None, s0
        out = self.conv(d["conv2"], g, pad=1, gn_src=src2_, res=res, want_stats=want_stats, out=out)
        self.free(g)
        self.free_raw(st2)
        return out

    def resnet(self, d, x, want_stats):
        """components:59-104 (groups > 1: explicit statistics + apply passes)."""
        e, B = self.e, self.B
        s0, s1, off1 = self.srcs(x)
        H, W = s0.H, s0.W
        G = e.cfg["resnet_block_groups"]
        co = d["dim_out"]
        y = self.conv(d["conv1"], s0, s1, off1, pad=1)
        h = self._gn_explicit(y, d["n1"], G, L.ACT_SILU, cbias=d["tb_off"])
        self.free(y)
        y = self.conv(d["conv2"], h, pad=1)
        self.free(h)
        if d["res"] is not None:
            r = self.conv(d["res"], s0, s1, off1)
        else:
            r = s0
        out = self._gn_explicit(y, d["n2"], G, L.ACT_SILU, res=r)
        self.free(y)
        if d["res"] is not None:
            self.free(r)
        if want_stats:
            self._direct_stats(out)
        return out

    def _direct_stats(self, a):
        ab = self.raw(self.B * 2 * 4)
        self._stats_op(a, 1, 1e-5, ab)
        a.stats = ("direct", ab)

    def _stats_op(self, a, G, eps, ab):
        """(rstd, rstd*mean) per (sample, group) of activation ``a`` by the streaming pass (workspace from the arena)."""
        e, B = self.e, self.B
        if isinstance(a.stats, tuple) and len(a.stats) == 3 and a.stats[2] == "chan_ws":
            # the producer left per-channel partial sums of this tensor (the 80-channel decoder kernels): no pass over it
            ws, slots, _ = a.stats
            self.op("ds_gn_stats_finish", ws[0], B, slots, a.C, G, a.H * a.W, eps, ab[0])
            self.free_raw(ws)
            a.stats = None
            return
        if a.C % e.vec == 0 and a.C // e.vec <= 256:
            ws = self.raw(self.lib.ds_gn_stats_ws_floats(B, a.H * a.W, a.C) * 4)
            self.op("ds_gn_stats_stream", a.off, e.dt, B, a.H * a.W, a.C, G, eps, ws[0], ab[0])
            self.free_raw(ws)
        else:
            self.op("ds_gn_stats", a.off, e.dt, B, a.H * a.W, a.C, G, eps, ab[0])

    def _gn_explicit(self, y, nrm, G, act, cbias=None, res=None, eps=1e-5):
        e, B = self.e, self.B
        ab = self.raw(B * G * 2 * 4)
        self._stats_op(y, G, eps, ab)
        out = self.act(y.C, y.H, y.W)
        p = L.GnApplyParams(x=y.off, res=(res.off if res is not None else None), out=out.off, gn_ab=ab[0],
                            gamma=nrm[0].data_ptr(), beta=nrm[1].data_ptr(),
                            cbias=(self.tb_all[0] + 4 * cbias) if (cbias is not None and self.tb_all) else None,
                            cb_stride=e._tb_total, B=B, HW=y.H * y.W, C=y.C, G=G, act=act, dtype=e.dt)
        self.op("ds_gn_apply", p)
        self.free_raw(ab)
        return out

    def _quad_takes(self, cw, x, stride=1):
        """Will conv(cw, an activation shaped like x) run on the four-tap halo kernel of the split-precision tier (which reads planes)?"""
        e = self.e
        return bool(e.split3 and cw.w_quad is not None and (cw.transposed or (stride == 2 and x.H % 2 == 0 and x.W % 2 == 0)))

    def block(self, d, x, want_stats=False):
        return self.convnext(d, x, want_stats) if self.e.cfg["use_convnext"] else self.resnet(d, x, want_stats)

    def attention(self, d, x, planes=None):
        """Residual(PreNorm(LinearCrossAttention[Add])) — components:22-29,142-152,171-207,252-293.
        planes (split-precision tier): "both" = the output additionally as hi / lo planes (out.planes), "only" = as planes alone
        (returned activation has .split set) — what the Down / Upsample that follows reads; ignored elsewhere."""
        e, B = self.e, self.B
        N, Cc = x.H * x.W, x.C
        lazy = (d["fused"] is not None or d.get("x3") is not None) and x.stats[0] != "direct"
        if lazy:
            xsrc, xst = self.stats_src(x, Cc * N)
            abx = (None, 0)
        elif x.stats[0] == "direct":
            abx = x.stats[1]
            x.stats = None
        else:
            abx = self.finalize(x, Cc * N)
        heads = 4
        nseg = max(1, min(N // 1024, 16))          # function of N only (batch-invariant results)
        if d.get("x3") is not None:
            return self._attention_x3(d, x, abx, lazy, xsrc if lazy else None, xst if lazy else None, planes)
        if d["fused"] is not None:
            # one input stream: k/v projection + softmax_n + k.v^T, then q projection + softmax_d + ctx^T.q + to_out
            # segments of partials: the library's choice for this shape and batch — N / 128 <= 32 for the first-generation context pass, one
            # round of blocks (one segment per wave) for the second generation, which it runs from U-Net batch 96 on (the bf16 tier's second
            # tiling decision that looks at B, after halo_ksplit)
            nseg = self.lib.ds_attn_fused_segments(B, N, Cc)
            part = self.raw(self.lib.ds_linattn_part_floats(B, heads, nseg) * 4)
            ctx = self.raw(B * heads * 1024 * 4)
            y = self.act(Cc, x.H, x.W)
            lab = self.lab_all[0] if self.lab_all else None
            fp = L.AttnFusedParams(x=x.off, B=B, N=N, C=Cc, nseg=nseg, wqkv=d["fused"][0].data_ptr(), t1=d["qkv"].t1.data_ptr(),
                                   t2=d["qkv"].t2.data_ptr(), gn_ab=abx[0], label_q=(lab + 4 * d["l_off"]) if lab else None,
                                   lq_stride=e._lab_total, scale=32 ** -0.5, part=part[0], ctx=ctx[0],
                                   wout_perm=d["fused"][1].data_ptr(), bias_out=d["out"].bias.data_ptr(), y=y.off, stats_part=None)
            if lazy:
                fp.gn_ab, fp.gn_part, fp.gn_parts, fp.gn_count, fp.gn_eps = None, xsrc[0], xsrc[1], float(xsrc[2]), xsrc[3]
            mfold = self.raw(B * Cc * 128 * 2) if Cc in (96, 192) else None      # to_out folded into the context (attn_out2.hpp)
            fp.mfold = mfold[0] if mfold is not None else None
            parts = self.lib.ds_attn_fused_stats_parts(C.byref(fp))
            st = self.raw(B * parts * 2 * 4)
            fp.stats_part = st[0]
            y.stats = (st, parts)
            self.op("ds_attn_fused_context", fp)
            self.op("ds_attn_fused_output", fp)
            if lazy:
                self.free_raw(xst)
            else:
                self.free_raw(abx)
            self.free_raw(part)
            self.free_raw(ctx)
            if mfold is not None:
                self.free_raw(mfold)
            out = self.act(Cc, x.H, x.W)
            g = L.GnApplyParams(x=y.off, res=x.off, out=out.off, gn_ab=None, gamma=d["on"][0].data_ptr(),
                                beta=d["on"][1].data_ptr(), cbias=None, cb_stride=0, B=B, HW=N, C=Cc, G=1, act=L.ACT_NONE, dtype=e.dt)
            ysrc, yst = self.stats_src(y, Cc * N)        # the apply pass reduces the output pass' partials itself
            g.gn_part, g.gn_parts, g.gn_count, g.gn_eps = ysrc[0], ysrc[1], float(ysrc[2]), ysrc[3]
            self.op("ds_gn_apply", g)
            self.free_raw(yst)
            self.free(y)
            return out
        qkv = self.conv(d["qkv"], x, gn_ab=abx[0])
        self.free_raw(abx)
        part = self.raw(self.lib.ds_linattn_part_floats(B, heads, nseg) * 4)
        ctx = self.raw(B * heads * 1024 * 4)
        ao = self.act(heads * 32, x.H, x.W)
        add = e.cfg["attn_type"] == "linear_add"
        lab = self.lab_all[0] if self.lab_all else None
        ls = e._lab_total
        p = L.AttnParams(qkv=qkv.off, B=B, N=N, heads=heads, dtype=e.dt, nseg=nseg, part=part[0], ctx=ctx[0],
                         label_q=(lab + 4 * d["l_off"]) if (lab and add) else None,
                         label_k=(lab + 4 * d["l_off"]) if (lab and not add) else None,
                         label_v=(lab + 4 * (d["l_off"] + heads * 32)) if (lab and not add) else None,
                         lq_stride=ls, lk_stride=ls, lv_stride=ls, q_softmax=1, scale=32 ** -0.5, out=ao.off)
        self.op("ds_linattn_context", p)
        self.op("ds_linattn_output", p)
        self.free(qkv)
        self.free_raw(part)
        self.free_raw(ctx)
        y = self.conv(d["out"], ao, want_stats=True)
        self.free(ao)
        aby = self.finalize(y, Cc * N)
        out = self.act(Cc, x.H, x.W)
        g = L.GnApplyParams(x=y.off, res=x.off, out=out.off, gn_ab=aby[0], gamma=d["on"][0].data_ptr(),
                            beta=d["on"][1].data_ptr(), cbias=None, cb_stride=0, B=B, HW=N, C=Cc, G=1, act=L.ACT_NONE, dtype=e.dt)
        self.op("ds_gn_apply", g)
        self.free(y)
        self.free_raw(aby)
        return out

    def _attention_x3(self, d, x, abx, lazy, xsrc, xst, planes=None):
        """The block in the split-precision tier (attn_x3.hip): x (fp32) is the only activation stream — k / v / q projections, both
        softmaxes, ctx and to_out as three-term bf16 MFMA products, and the output GroupNorm + residual applied while y is computed a
        second time (ds_attn_x3_output form B: no y tensor, no apply pass; +1.15 % on the step against form A + ds_gn_apply, same box —
        after the statistics-only pass lost the 644 bytes of scratch that made it slower than the pass that writes y)."""
        e, B = self.e, self.B
        N, Cc = x.H * x.W, x.C
        lib = self.lib
        nseg = lib.ds_attn_x3_segments(B, N, Cc)
        part = self.raw(lib.ds_linattn_part_floats(B, 4, nseg) * 4)
        ctx = self.raw(B * 4 * 1024 * 4)
        qpl = self.raw(lib.ds_attn_x3_qplane_bytes(B, N)) if Cc != 96 else None      # (C = 96: q is projected inside the fused pass 2)
        mf = self.raw(lib.ds_attn_x3_mfold_bytes(B, Cc))
        out = self.act(Cc, x.H, x.W) if planes != "only" else None
        pl = self.act(Cc, x.H, x.W) if planes else None            # (2C bf16 per pixel = the bytes of C fp32)
        if pl is not None:
            pl.split = True
        lab = self.lab_all[0] if self.lab_all else None
        fp = L.AttnX3Params(x=x.off, B=B, N=N, C=Cc, nseg=nseg, wqkv_hl=d["x3"][0].data_ptr(), t1=d["qkv"].t1.data_ptr(),
                            t2=d["qkv"].t2.data_ptr(), gn_ab=abx[0], label_q=(lab + 4 * d["l_off"]) if lab else None,
                            lq_stride=e._lab_total, scale=32 ** -0.5, part=part[0], ctx=ctx[0], qplanes=(qpl[0] if qpl else None), mfold=mf[0],
                            wout=d["x3"][1].data_ptr(), bias_out=d["out"].bias.data_ptr(), y=None, stats_part=None,
                            out=(out.off if out is not None else None), on_gamma=d["on"][0].data_ptr(), on_beta=d["on"][1].data_ptr(), on_eps=1e-5,
                            out_planes=(pl.off if pl is not None else None))
        if lazy:
            fp.gn_ab, fp.gn_part, fp.gn_parts, fp.gn_count, fp.gn_eps = None, xsrc[0], xsrc[1], float(xsrc[2]), xsrc[3]
        parts = lib.ds_attn_x3_stats_parts(C.byref(fp))
        st = self.raw(B * parts * 2 * 4)
        fp.stats_part = st[0]
        self.op("ds_attn_x3_context", fp)
        self.op("ds_attn_x3_output", fp)
        if lazy:
            self.free_raw(xst)
        else:
            self.free_raw(abx)
        for r in (part, ctx, qpl, mf):
            if r is not None:
                self.free_raw(r)
        self.free_raw(st)
        if planes == "only":
            return pl
        if pl is not None:
            out.planes = pl
        return out

    # ---------------------------------------------------------------- whole graph
    def build(self, base):
        self.base = base
        e, cfg, B, H, W = self.e, self.e.cfg, self.B, self.H, self.W
        P = e.P
        # --- conditioning (diffusion.py:200-203,212; components:42-56,112-116,155-168,267-268)
        self.tb_all = None
        self.lab_all = None
        self.sin = self.h1 = self.temb = None
        if e.m.time_mlp is not None:
            half = cfg["down_dims"][0] // 2
            td = cfg["time_dim"]
            self.sin = self.raw(B * 2 * half * 4)
            self.h1 = self.raw(B * td * 4)
            self.temb = self.raw(B * td * 4)
            # op args containing the per-call time pointer are patched in run(): marked with "T"
            self.ops.append(("sinusoid", half))
            self.op("ds_linear", self.sin[0], 2 * half, e.tm1[0].data_ptr(), e.tm1[1].data_ptr(), B, 2 * half, td, L.ACT_NONE, self.h1[0], td)
            # the activations in front of the two wide linears are applied once, in place (ds_linear's act_in evaluates them once per 16 outputs:
            # 80 + 85 us of exact-erf GELUs per step at U-Net batch 128); h1 and temb have no other reader
            self.op("ds_activation", self.h1[0], B * td, L.ACT_GELU, self.h1[0])
            self.op("ds_linear", self.h1[0], td, e.tm3[0].data_ptr(), e.tm3[1].data_ptr(), B, td, td, L.ACT_NONE, self.temb[0], td)
            if e.tb_W is not None:
                self.tb_all = self.raw(B * e._tb_total * 4)
                self.op("ds_activation", self.temb[0], B * td, L.ACT_GELU if cfg["use_convnext"] else L.ACT_SILU, self.temb[0])
                self.op("ds_linear", self.temb[0], td, e.tb_W.data_ptr(), e.tb_b.data_ptr(), B, td, e._tb_total, L.ACT_NONE, self.tb_all[0], e._tb_total)
        if self.has_cond:
            ld = e.label_dim
            if e.emb_is_linear:
                self.cemb = self.raw(B * ld * 4)
                self.ops.append(("cond_embed", ld))
                cptr = self.cemb[0]
            else:
                self.cemb = None
                cptr = "COND"
            self.lab_all = self.raw(B * e._lab_total * 4)
            self.ops.append(("labels", cptr, ld))

        # --- trunk
        self.n_cond = len(self.ops)                    # ops [0, n_cond) read (time, condition) only: the conditioning GEMVs
        # classifier-free guidance evaluates cat([x, x]) with cat([uncond, cond]): the two halves are the same computation until the first
        # attention block adds the label query — the init convolution and the first block run ONCE, at half the batch, and their two results
        # (the skip tensor and the block output with its GroupNorm partials) are duplicated (ds_dup_batch).  Bit-identical to the plain plan:
        # the split-K decisions of these layers are taken from the full batch (self.Btile), everything else depends on the layer shape only.
        Bfull = self.B
        half = self.paired and len(P["downs"]) > 0
        if half:
            self.B = B = Bfull // 2
            self.alloc_B = Bfull
        xin = self.act(e.cin0, H, W)
        self.ops.append(("input", xin.off, self.B))
        if getattr(P["init"], "w_init7", None) is not None:
            cw = P["init"]
            x = self.act(96, H, W)
            self.conv_meta[len(self.ops)] = (L.TILE_INIT7, 2.0 * B * H * W * 96 * 49 * cw.cin_real, f"7x7 {cw.cin_real}->96 @{H}x{W}")
            self.op("ds_conv7x7_c4", xin.off, B, H, W, e.cin0, cw.w_init7.data_ptr(), L.ptr(cw.bias), x.off)
        elif getattr(P["init"], "w_init7x3", None) is not None:
            cw = P["init"]
            x = self.act(96, H, W)
            self.op("ds_conv7x7_c4_x3", xin.off, B, H, W, cw.w_init7x3.data_ptr(), L.ptr(cw.bias), x.off)
        else:
            x = self.conv(P["init"], xin, pad=3)
        self.free(xin)
        self.n_cond_join = len(self.ops)               # first op that may consume a conditioning output
        skips = [x]
        for b1, a1, b2, a2, down in P["downs"]:
            y = self.block(b1, x, True)
            if half:
                half = False
                self.B = B = Bfull
                self.alloc_B = 0
                xf, yf = self.dup(x), self.dup(y)
                self.free(x)
                self.free(y)
                x, y = xf, yf
                skips[-1] = x
            if x is not skips[-1]:
                self.free(x)
            x = self.attention(a1, y)
            self.free(y)
            skips.append(x)
            y = self.block(b2, x, True)
            x = self.attention(a2, y, planes="both" if self._quad_takes(down, y, stride=2) else None)
            self.free(y)
            skips.append(x)
            x = self.conv(down, x, stride=2, pad=1)
            skips.append(x)
        for b in P["mid_left"]:
            x = self.block(b, x)
            skips.append(x)
        b1, a, b2 = P["mid_mid"]
        y = self.block(b1, x, True)
        x = self.attention(a, y)
        self.free(y)
        y = self.block(b2, x)
        self.free(x)
        x = y
        for b in P["mid_right"]:
            sk = skips.pop()
            y = self.block(b, (sk, x))
            self.free(sk)
            self.free(x)
            x = y
        for b1, a1, up, b2, a2, b3, a3 in P["ups"]:
            for blk, at, do_up in ((b1, a1, True), (b2, a2, False), (b3, a3, False)):
                sk = skips.pop()
                y = self.block(blk, (sk, x), True)
                self.free(sk)
                self.free(x)
                x = self.attention(at, y, planes="only" if (do_up and self._quad_takes(up, y)) else None)
                self.free(y)
                if do_up:
                    y = self.conv(up, x)
                    self.free(x)
                    x = y
        sk = skips.pop()
        assert not skips
        y = self.block(P["final_block"], (sk, x))
        self.free(sk)
        self.free(x)
        z = self.conv(P["final"], y, pad=1)                  # NHWC, out_dim rounded up to the vector width
        self.free(y)
        self.ops.append(("output", z.off, z.C))
        self.free(z)

    # ---------------------------------------------------------------- execution
    def run_graphed(self, x, time, cond, out):
        """run() captured once as a HIP graph over static input / output buffers, then replayed (ConditionedUnet.use_hip_graph)."""
        g = getattr(self, "_graph", None)
        if g is None:
            self._gx, self._gt, self._go = torch.empty_like(x), torch.empty_like(time), torch.empty_like(out)
            self._gc = torch.empty_like(cond) if cond is not None else None
            self._gx.copy_(x)
            self._gt.copy_(time)
            if cond is not None:
                self._gc.copy_(cond)
            self.run(self._gx, self._gt, self._gc, self._go)       # eager once: per-kernel attributes, the side stream, lazy allocations
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.run(self._gx, self._gt, self._gc, self._go)
            self._graph = g
        self._gx.copy_(x, non_blocking=True)
        self._gt.copy_(time, non_blocking=True)
        if cond is not None:
            self._gc.copy_(cond, non_blocking=True)
        g.replay()
        out.copy_(self._go, non_blocking=True)

    def run(self, x, time, cond, out):
        e, B = self.e, self.B
        st = L.current_stream()
        lib = self.lib
        prof = self.prof
        if prof is not None:
            if self.calls % self.prof_every:
                prof = None
            self.calls += 1
        # The conditioning GEMVs (0.36 ms at U-Net batch 128: five latency-bound launches) depend on (time, condition) only: at
        # large batches they run on a side stream under the layout change + init convolution of the trunk.
        side = None
        if self.n_cond > 0 and B * self.H * self.W >= 65536:
            if e.side_stream is None:
                e.side_stream = torch.cuda.Stream()
            side = e.side_stream
        main_st = st
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
            st = side.cuda_stream
        for k, item in enumerate(self.ops):
            tag = item[0]
            if side is not None:
                if k == self.n_cond:
                    st = main_st
                elif k == self.n_cond_join:
                    torch.cuda.current_stream().wait_stream(side)
            if prof is not None and k in self.conv_meta:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                rc = item[0](C.byref(item[1][0]), st) if isinstance(item[1][0], C.Structure) else item[0](*item[1], st)
                ev1.record()
                prof.append((k, ev0, ev1))
                if rc != 0:
                    L.check(rc, item[2])
                continue
            if tag == "sinusoid":
                rc = lib.ds_sinusoid(time.data_ptr(), e.freqs.data_ptr(), B, item[1], self.sin[0], st)
                name = "ds_sinusoid"
            elif tag == "cond_embed":
                ld = item[1]
                rc = lib.ds_linear(cond.data_ptr(), ld, e.emb_w.data_ptr(), e.emb_b.data_ptr(), B, ld, ld, L.ACT_NONE, self.cemb[0], ld, st)
                name = "ds_linear(cond)"
            elif tag == "labels":
                src = cond.data_ptr() if item[1] == "COND" else item[1]
                rc = lib.ds_linear(src, item[2], e.lab_W.data_ptr(), e.lab_b.data_ptr(), B, item[2], e._lab_total, L.ACT_NONE,
                                   self.lab_all[0], e._lab_total, st)
                name = "ds_linear(labels)"
            elif tag == "input":
                rc = lib.ds_nchw_to_nhwc(x.data_ptr(), item[2], x.shape[1], self.H, self.W, item[1], e.cin0, e.dt, st)
                name = "ds_nchw_to_nhwc"
            elif tag == "output":
                rc = lib.ds_nhwc_to_nchw(item[1], e.dt, B, out.shape[1], item[2], self.H, self.W, out.data_ptr(), st)
                name = "ds_nhwc_to_nchw"
            else:
                fn, args, name = item
                a0 = args[0]
                if isinstance(a0, C.Structure):
                    rc = fn(C.byref(a0), st)
                else:
                    rc = fn(*args, st)
            if rc != 0:
                L.check(rc, name)
