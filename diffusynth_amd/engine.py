"""Host-side execution plan of the U-Net forward pass (Python over the C ABI).

``UnetEngine`` packs the module's parameters once (GroupNorm gains folded into the packed
convolution weights, border-class shift tables, stacked conditioning matrices) and, per input
shape, builds a *plan*: a flat list of pre-bound C-ABI calls whose activation buffers are
carved at plan time from one arena (first-fit with explicit lifetimes, so the working set
stays small and hot in L2 / Infinity Cache).  Running a plan is a loop of ctypes calls on the
caller's current HIP stream — no allocation, no synchronisation, HIP-graph capturable.

Graph: model/diffusion.py:187-258.  Blocks: model/diffusion_components.py (cited per method).
"""
import collections
import ctypes as C
import math
import os
from typing import NamedTuple

import torch

from . import _lib as L
from . import conv_policy as policy
from .conv_policy import up as _up

_ESIZE = {L.DS_F32: 4, L.DS_BF16: 2}
_TDT = {L.DS_F32: torch.float32, L.DS_BF16: torch.bfloat16}
_X, _TIME, _COND, _OUT = range(4)        # _Op.late of the U-Net plan: which tensor of run(x, time, cond, out)


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


class _Partials(NamedTuple):
    """GroupNorm statistics a producer left as partial sums: ``buf`` = [B][parts][2] floats; a consumer or ds_gn_finalize reduces them."""
    buf: tuple
    parts: int


class _Finished(NamedTuple):
    """GroupNorm statistics already finished: ``buf`` = (rstd, rstd * mean) per sample."""
    buf: tuple


class _ChanSums(NamedTuple):
    """Per-channel partial sums (the 80-channel decoder kernels): ``buf`` = [B][slots][C][2] floats; ds_gn_stats_finish reduces them."""
    buf: tuple
    slots: int


class _Op(NamedTuple):
    """One launch of a plan: ``fn(*args, stream)``, parameter structs already wrapped in C.byref (``args[0]._obj`` is the struct).
    ``late`` = ((argument position, index into the tensors run() was called with), ...): pointers only known per call; None for most."""
    name: str
    fn: object
    args: tuple
    late: tuple = None


class _Act:
    """Channels-last activation [B][H][W][C] living at arena offset ``off``."""
    __slots__ = ("off", "nbytes", "C", "H", "W", "stats", "split", "planes")

    def __init__(self, off, nbytes, Cc, H, W):
        self.off, self.nbytes, self.C, self.H, self.W = off, nbytes, Cc, H, W
        self.stats = None        # GroupNorm statistics of this tensor, left by its producer: _Partials, _Finished or _ChanSums (raw buffer in .buf)
        self.split = False       # split-precision tier: the buffer holds 2C bf16 channels per pixel (hi plane, lo plane), not C fp32
        self.planes = None       # ... or a second activation holding this tensor in that form (written by the producer for a Down / Upsample)


class _ConvW:
    """Packed convolution: the generic kernel's weights (+ GroupNorm fold tables) and every other form the layer's shape and tier
    qualify for (conv_policy.*_fits; None where not).  conv() picks one of them per launch."""
    __slots__ = ("w", "bias", "t1", "t2", "ncls", "Cout", "cout_pad", "cin_pad", "cin_real", "KH", "KW", "bn", "transposed", "k_order",
                 "w_f32n4", "w_x3", "x3_cout_pad", "w_n16", "w_split", "w_quad", "quad_cout_pad", "w_init7", "w_init7x3",
                 "w_fused", "res_steps", "res_bias")

    def __init__(self, s):
        self.Cout, self.cin_pad, self.cin_real, self.transposed = s.Cout, s.cin_pad, s.Cin, s.transposed
        self.KH, self.KW = (2, 2) if s.transposed else s.k
        self.bn, self.cout_pad, self.k_order = s.bn, s.cout_pad, s.k_order
        self.w = self.bias = self.t1 = self.t2 = None
        self.w_f32n4 = self.w_x3 = self.w_n16 = self.w_split = self.w_quad = self.w_init7 = self.w_init7x3 = None
        self.ncls, self.x3_cout_pad, self.quad_cout_pad = 1, 0, 0
        self.w_fused, self.res_steps, self.res_bias = None, 0, None       # the block's 1x1 res_conv in front (UnetEngine._pack_block)


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


def max_plans():
    """Plans an engine keeps (least recently used evicted): DS_MAX_PLANS, default 8."""
    return max(1, int(os.environ.get("DS_MAX_PLANS", "8")))


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
        self.plans = collections.OrderedDict()       # _cached_plan: least recently used first
        self._max_plans = max_plans()
        self._arena, self._arena_base, self._arena_bytes = None, 0, 0
        self.hip_graph = False   # UnetEngine.forward: replay plans as captured HIP graphs (ConditionedUnet.use_hip_graph)
        self.plan_builds = 0     # plans built so far (cache misses of _cached_plan)
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
        plan = self.plans.get(key)
        if plan is not None:
            self.plans.move_to_end(key)
            return plan
        self.plan_builds += 1
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

    def _pack_weight(self, w, gamma, dtype, Cout, Cin, cin_pad, KH, KW, cout_pad, transposed=False, k_order=1):
        """ds_pack_conv_weight into a new tensor (k_order 1: chunk-major tiles of the halo kernels)."""
        dst = torch.empty(L.load().ds_pack_conv_elems(cin_pad, KH, KW, cout_pad, int(transposed)), dtype=_TDT[dtype], device=self.dev)
        pp = L.PackConvParams(w=w.data_ptr(), gamma=L.ptr(gamma), dst=dst.data_ptr(), dtype=dtype, Cout=Cout, Cin=Cin, cin_pad=cin_pad,
                              KH=KH, KW=KW, cout_pad=cout_pad, transposed=int(transposed), k_order=k_order)
        L.call("ds_pack_conv_weight", C.byref(pp), L.current_stream())
        return dst

    def _pack_init7(self, w, fn, planes):
        dst = torch.empty(planes * L.load().ds_conv7x7_c4_weight_elems(), dtype=torch.bfloat16, device=self.dev)
        L.call(fn, w.data_ptr(), 96, int(w.shape[1]), dst.data_ptr(), L.current_stream())
        return dst

    def _pack_conv(self, weight, bias, cin_pad=None, gamma=None, beta=None, transposed=False, small_out=False, halo=False):
        """halo=True: the layer is a single-source 3x3 stride-1 convolution of a block, i.e. it runs on an LDS-halo kernel where its tier
        has one (bf16: chunk-major weights, k_order 1; bf16x3: the split-precision weights)."""
        w = self._f32(weight)
        Cin, Cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
        s = policy.ConvLayer(Cout, Cin, Cin if cin_pad is None else cin_pad, tuple(w.shape[2:]), transposed, gamma is not None, halo,
                             small_out, self.dt == L.DS_BF16, self.split3)
        cw = _ConvW(s)
        g = self._f32(gamma) if gamma is not None else None
        cw.w = self._pack_weight(w, g, self.dt, Cout, Cin, s.cin_pad, cw.KH, cw.KW, cw.cout_pad, transposed, cw.k_order)
        cw.bias = self._f32(bias) if bias is not None else None
        if s.f32n4_fits:
            cw.w_f32n4 = torch.empty(L.load().ds_conv3x3_f32_n4_weight_floats(Cin), dtype=torch.float32, device=self.dev)
            L.call("ds_pack_conv3x3_f32_n4", w.data_ptr(), L.ptr(cw.bias), Cout, Cin, cw.w_f32n4.data_ptr(), L.current_stream())
        if s.x3_1x1_fits:
            cw.w_x3, cw.x3_cout_pad = pack_x3_1x1(weight.to(self.dev), gamma.to(self.dev) if gamma is not None else None)
        if s.n16_fits:
            cw.w_n16 = self._pack_weight(w, None, L.DS_BF16, Cout, Cin, Cin, 3, 3, 16)
        if s.split3_fits:
            ws = split3_weight(weight, gamma)                                     # [Cout][3 Cin][3][3] fp32: per chunk W_hi | W_lo | W_hi (gain folded)
            cw.w_split = self._pack_weight(ws, None, L.DS_BF16, Cout, 3 * Cin, 3 * Cin, 3, 3, cw.cout_pad)
            self._pack_tmp.append(ws)
        if s.quad_fits:
            # in the split-precision tier as [W_hi | W_hi | W_lo] over 3 Cin input channels (the kernel then reads hi / lo planes)
            wq = weight
            if self.split3:
                w32 = weight.detach().float()
                hi = w32.bfloat16().float()
                wq = torch.cat([hi, hi, w32 - hi], 0 if transposed else 1)
            cw.w_quad, cw.quad_cout_pad = pack_quad_weights(wq, transposed)
        if s.init7_fits:
            cw.w_init7 = self._pack_init7(w, "ds_pack_conv7x7_c4", 1)
        if s.init7x3_fits:
            cw.w_init7x3 = self._pack_init7(w, "ds_pack_conv7x7_c4_x3", 2)
        if gamma is not None:
            cw.ncls = 9 if cw.KH == 3 else 1
            cw.t1 = torch.empty(cw.ncls * Cout, dtype=torch.float32, device=self.dev)
            cw.t2 = torch.empty(cw.ncls * Cout, dtype=torch.float32, device=self.dev)
            b = self._f32(beta)
            L.call("ds_conv_fold_tables", w.data_ptr(), L.ptr(cw.bias), g.data_ptr(), b.data_ptr(), Cout, Cin, cw.KH, cw.KW,
                   cw.t1.data_ptr(), cw.t2.data_ptr(), L.current_stream())
            self._keep += [g, b]
        self._pack_tmp += [w, g]
        return cw


class _PlanBase:
    """What the U-Net and the VQGAN plans share: the arena, the op list and its launch loop, convolutions and GroupNorm statistics."""
    prof_all = False             # profile every op (True) or the ops in conv_meta only

    def __init__(self, eng, B, H, W):
        self.e, self.B, self.H, self.W = eng, B, H, W
        self.alloc_B = 0         # > B only while a paired plan's shared prefix runs at half the batch (act(): tensors carved at full size)
        self.Btile = getattr(eng, "launch_batch", None) or B
        #                          the batch every batch-dependent launch decision looks at (split-K factors; through the structs' batch_hint the
        #                          depthwise family / row ranges / chunks, the halo kernel's pair tile, the attention generations and blocks per
        #                          sample; the attention segment counts): the FULL batch, also while the shared prefix of a paired (CFG) plan runs
        #                          at half of it — the prefix then adds its partial sums in the plain plan's order (same bits) — or the engine's
        #                          pin (UnetEngine.launch_batch), and then never B: workspaces alone are sized from the actual batch
        self.tb_all = self.lab_all = None      # the U-Net's conditioning outputs (time biases, label projections) where its build() makes them
        self.arena = _Arena()
        self.ops = []            # _Op records, in launch order
        self.ws = None
        self.lib = L.load()
        self.conv_meta = {}      # op index -> (tile id, algorithmic FLOPs, description) for every ds_conv_igemm launch
        self.prof = None         # set to a list to collect (op index, start event, end event) per profiled launch
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
                self.free_raw(a.stats.buf)       # (every form owns one raw buffer)
                a.stats = None
            if a.planes is not None:
                self.free(a.planes)
                a.planes = None
        else:
            self.free_raw(a)

    def free_raw(self, r):
        self.arena.release(r[0] - self.base, r[1])

    def op(self, name, *args, late=None):
        """Record a launch (a parameter struct is passed as its C.byref, bound here once); ``late`` as in _Op, those positions hold None."""
        self.ops.append(_Op(name, getattr(self.lib, name), args, late))

    # ---------------------------------------------------------------- execution
    def _prof_now(self):
        """The list this call's event pairs go to, or None (no profiling, or not a prof_every-th call)."""
        prof = self.prof
        if prof is not None:
            if self.calls % self.prof_every:
                prof = None
            self.calls += 1
        return prof

    def launch(self, lo, hi, st, tensors, prof):
        """Run ops [lo, hi) on stream ``st`` — the one loop that calls plan ops.  tensors: what the _Op.late positions index."""
        meta = None if self.prof_all else self.conv_meta
        for k, (name, fn, args, late) in enumerate(self.ops[lo:hi], lo):
            if late is not None:
                args = list(args)
                for pos, t in late:
                    args[pos] = tensors[t].data_ptr()
            if prof is not None and (meta is None or k in meta):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                rc = fn(*args, st)
                ev1.record()
                prof.append((k, ev0, ev1))
            else:
                rc = fn(*args, st)
            if rc != 0:
                L.check(rc, name)

    # ---------------------------------------------------------------- kernels
    def _halo3_ksplit(self, cw, x, split):
        """Split-K factor of a 3x3 halo launch over x (split: split precision), from the plan's FULL batch (self.Btile)."""
        return policy.halo3_ksplit(self.Btile, x.H, x.W, cw.cout_pad, x.C // 32, split)

    def _split_takes(self, cw, src1=None, stride=1, pad=1, out_nchw_ptr=False):
        """Does conv(cw, ...) run the split-precision halo kernel when its input holds hi / lo planes (DS_CONV_F_SPLIT_IN)?"""
        return cw.w_split is not None and src1 is None and stride == 1 and pad == 1 and not out_nchw_ptr

    def _quad_takes(self, cw, x, stride=1, pad=0, src1=None, res=None, gn_ab=None, out_nchw_ptr=False):
        """Does conv(cw, x, ...) run on the four-tap halo kernel (conv_quad_halo3.hip; in the split-precision tier it reads planes)?"""
        return (cw.w_quad is not None and src1 is None and res is None and gn_ab is None and not out_nchw_ptr and (not x.split or self.e.split3)
                and (cw.transposed or (stride == 2 and pad == 1 and x.H % 2 == 0 and x.W % 2 == 0)))

    def _conv_route(self, cw, src0, src1, stride, pad, gn_ab, act, res, want_stats, out, out_nchw_ptr, gn_src, res_fuse):
        """The kernel a launch runs on: the first packed form the call allows (the special forms exclude each other by shape or tier)."""
        plain = src1 is None and stride == 1 and pad == 1 and not out_nchw_ptr and res is None and gn_ab is None and not want_stats
        if cw.w_f32n4 is not None and plain and not src0.split and out.C == 4 and act == L.ACT_NONE and res_fuse is None:
            return "f32n4"
        if (cw.w_x3 is not None and stride == 1 and pad == 0 and not out_nchw_ptr and not src0.split and gn_src is None and act == L.ACT_NONE
                and src0.C % 32 == 0 and (src1.C if src1 is not None else 0) % 32 == 0):
            return "x3"
        if cw.w_n16 is not None and plain and not src0.split:
            return "n16"
        if self._split_takes(cw, src1, stride, pad, out_nchw_ptr) and src0.split:
            return "split"
        if self._quad_takes(cw, src0, stride, pad, src1, res, gn_ab, out_nchw_ptr):
            return "quad"
        if cw.k_order == 1:
            # chunk-major weights = a single-source 3x3 stride-1 pad-1 layer packed for the LDS-halo kernel (conv3x3_halo3.hip)
            assert src1 is None and stride == 1 and pad == 1 and src0.C % 32 == 0, "chunk-major weights reached a layer the halo kernel cannot run"
            return "halo3"
        return "igemm"

    def conv(self, cw, src0, src1=None, off1=(0, 0), stride=1, pad=0, gn_ab=None, act=L.ACT_NONE, res=None,
             want_stats=False, out=None, out_nchw_ptr=False, gn_src=None, res_fuse=None, out_split=False):
        """gn_src = (partials ptr, parts, count, eps): the consumer reduces the producer's statistics itself.
        res_fuse = (x0, x1, off1): run the block's 1x1 res_conv over pad_and_concat(x0, x1) inside this launch (HALO3 tile,
        weights packed with the res tiles appended; the caller checked that the launch does not split K).
        The route (kernel + packed form) is picked first, then its ConvParams filled once; split-K, statistics partials and conv_meta follow."""
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
        route = self._conv_route(cw, src0, src1, stride, pad, gn_ab, act, res, want_stats, out, out_nchw_ptr, gn_src, res_fuse)
        if route == "f32n4":
            self.op("ds_conv3x3_f32_n4", src0.off, B, H, W, src0.C, cw.w_f32n4.data_ptr(), out.off)
            return out
        # The tile depends on the layer shape only.  fp32 never splits K: a sample's result (incl. its GroupNorm partials) does not change
        # with the batch it is computed in.  The 16-bit tiers split K by self.Btile (and pick attention segments by B): to the rounding of fp32 sums.
        tile, dtype, src, C0, flags, wpk, cout_pad, korder, out_C = None, e.dt, src0, src0.C, 0, cw.w, cw.cout_pad, cw.k_order, out.C
        xsplit = None
        if route == "x3":
            # split-precision tier: 1x1 convolution of fp32 tensors as three bf16 MFMA products (conv1x1_x3.hip)
            tile, dtype, flags, wpk, cout_pad, korder = 0, L.DS_BF16, 8 | 4, cw.w_x3, cw.x3_cout_pad, 0
        elif route == "n16":
            tile, wpk, cout_pad, korder = L.TILE_HALO3_N16, cw.w_n16, 16, 1
        elif route == "split":
            # split-precision 3x3: input = hi / lo bf16 planes (2C channels), output = planes again (conv1: feeds conv2) or fp32 (conv2)
            tile, dtype, C0, flags, wpk, korder = L.TILE_HALO3_256x96, L.DS_BF16, 2 * src0.C, 1 | (2 if out_split else 4), cw.w_split, 1
            out_C = 2 * out.C if out_split else out.C
            out.split = bool(out_split)
        elif route == "quad":
            tile, wpk, cout_pad, korder = L.TILE_QUAD_HALO3, cw.w_quad, cw.quad_cout_pad, 2
            if e.split3:
                # split-precision tier: the kernel reads hi / lo bf16 planes and writes fp32.  The planes come from the producer where it
                # wrote them (the attention block in front of a Down / Upsample, r04) — otherwise one streaming pass re-stores the fp32 input
                src = src0 if src0.split else src0.planes
                if src is None:
                    src = xsplit = self.act(src0.C, H, W)
                    self.op("ds_split_planes", src0.off, xsplit.off, B * H * W, src0.C)
                elif not src0.split:
                    xsplit, src0.planes = src, None                      # (released after this launch)
                dtype, C0, flags = L.DS_BF16, 2 * src0.C, 1 | 4
        else:
            tile = policy.igemm_tile(cw.bn, Ho * Wo, cw.k_order)
        extra = {}
        if gn_src is not None:
            extra.update(gn_part=gn_src[0], gn_parts=gn_src[1], gn_count=float(gn_src[2]), gn_eps=gn_src[3])
        if res_fuse is not None:
            x0, x1, xoff = res_fuse
            assert tile == L.TILE_HALO3_256x96 and cw.res_steps == (x0.C + (x1.C if x1 is not None else 0)) // 32 and res is None
            wpk = cw.w_fused
            extra.update(res_src0=x0.off, res_C0=x0.C, res_steps=cw.res_steps, res_bias=L.ptr(cw.res_bias))
            if x1 is not None:
                extra.update(res_src1=x1.off, res_C1=x1.C, res_H1=x1.H, res_W1=x1.W, res_off_h1=xoff[0], res_off_w1=xoff[1])
        # K slices at small batches: the grid of (tile x channel-tile x sample) blocks cannot fill the 256 CUs (conv_policy)
        ks = 1
        if route in ("halo3", "split") and res_fuse is None:
            ks = self._halo3_ksplit(cw, src0, route == "split")
        elif route == "quad":
            ks = policy.quad_ksplit(self.Btile, Ho, Wo, cw.quad_cout_pad, (1 if cw.transposed else 4) * (3 if e.split3 else 1) * src0.C // 32, e.split3)
        elif route == "igemm" and e.dt == L.DS_BF16:
            nq = -(-((4 if cw.transposed else cw.KH * cw.KW) * (src0.C + C1)) // 32)
            ks = policy.igemm_ksplit(self.Btile, tile, Ho, Wo, cw.cout_pad, nq, 4 if cw.transposed else 1)
        elif route == "x3":
            ks = policy.x3_1x1_ksplit(self.Btile, Ho, Wo, cw.x3_cout_pad, (src0.C + C1) // 32)
        slab = None
        if ks > 1:
            slab = self.raw(ks * B * oh * ow * _up(cw.Cout, 8) * 4)
            extra.update(ksplit=ks, slab=slab[0])
        if src1 is not None:
            extra.update(src1=src1.off, H1=src1.H, W1=src1.W)
        p = L.ConvParams(src0=src.off, C0=C0, C1=C1, H=H, W=W, off_h1=off1[0], off_w1=off1[1], wpk=wpk.data_ptr(), Cout=cw.Cout,
                         cout_pad=cout_pad, KH=cw.KH, KW=cw.KW, stride=stride, pad_h=pad, pad_w=pad, Ho=Ho, Wo=Wo,
                         transposed=int(cw.transposed), out=out.off, out_C=out_C, out_c0=0, out_nchw_f32=0,
                         bias=L.ptr(cw.bias), gn_ab=(gn_ab if gn_src is None else None), fold_t1=L.ptr(cw.t1) if gn_ab else None,
                         fold_t2=L.ptr(cw.t2) if gn_ab else None, ncls=cw.ncls if gn_ab else 1, act=act,
                         res=(res.off if res is not None else None), stats_part=None, B=B, dtype=dtype, tile=tile, wk_order=korder,
                         flags=flags, batch_hint=self.Btile, **extra)
        if want_stats:
            parts = (self.lib.ds_conv1x1_x3_stats_parts if route == "x3" else self.lib.ds_conv_stats_parts)(C.byref(p))
            st = self.raw(B * parts * 2 * 4)
            p.stats_part = st[0]
            out.stats = _Partials(st, parts)
        if route == "x3":
            self.op("ds_conv1x1_x3", C.byref(p))
        else:
            self.conv_meta[len(self.ops)] = policy.conv_meta(tile, B, Ho, Wo, cw.Cout, cw.KH, cw.KW, cw.transposed, src0.C + C1, cw.cin_real,
                                                             32 * cw.res_steps if res_fuse is not None else 0)
            self.op("ds_conv_igemm", C.byref(p))
        if xsplit is not None:
            self.free(xsplit)
        if slab is not None:
            self.op("ds_conv_splitk_reduce", C.byref(p))
            self.free_raw(slab)
        return out

    @staticmethod
    def _partials(a, who):
        assert isinstance(a.stats, _Partials), f"{who}() reads a producer's partial sums, not {type(a.stats).__name__}"
        return a.stats

    def finalize(self, a, count, eps=1e-5):
        """partials of activation ``a`` -> (rstd, rstd*mean) per sample; returns raw buffer."""
        st, parts = self._partials(a, "finalize")
        ab = self.raw(self.B * 2 * 4)
        self.op("ds_gn_finalize", st[0], self.B, parts, float(count), eps, ab[0])
        self.free_raw(st)
        a.stats = None
        return ab

    def stats_src(self, a, count, eps=1e-5):
        """Hand activation ``a``'s raw partials to the consumer: returns (gn_src tuple, raw buffer to free after use)."""
        st, parts = self._partials(a, "stats_src")
        a.stats = None
        return (st[0], parts, count, eps), st

    def srcs(self, x):
        """x is an _Act or (enc, dec) pair to be read as pad_and_concat(enc, dec) (components:210-249)."""
        if isinstance(x, _Act):
            return x, None, (0, 0)
        enc, dec = x
        return enc, dec, ((enc.H - dec.H) // 2, (enc.W - dec.W) // 2)

    def _stats_op(self, a, G, eps, ab):
        """(rstd, rstd*mean) per (sample, group) of activation ``a`` by the streaming pass (workspace from the arena)."""
        e, B = self.e, self.B
        if isinstance(a.stats, _ChanSums):
            # the producer left per-channel partial sums of this tensor (the 80-channel decoder kernels): no pass over it
            ws, slots = a.stats
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
        self.op("ds_gn_apply", C.byref(p))
        self.free_raw(ab)
        return out


class UnetEngine(_EngineBase):
    use_cfg_pair = True      # shared prefix of a classifier-free-guidance batch computed once (tests switch it off to compare)

    def __init__(self, module, compute_dtype="fp32"):
        self._init_common(module, compute_dtype)
        self.cfg = module.config
        # None: every plan decides from its own batch.  P >= 1 (ConditionedUnet.pin_launch_batch; U-Net rows, a CFG batch counts double): every
        # batch-dependent launch decision of every plan is taken as if the batch were P (_PlanBase.Btile), so a sample's partial sums are
        # grouped — and its result rounded — the same way in whatever batch it travels.  Part of the plan cache key.
        self.launch_batch = None
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
            c2, cx = d["conv2"], blk.res_conv.weight.shape[1]
            if c2.k_order == 1 and cx % 96 == 0:      # (the fused steps come in threes: the weight ring's phase)
                # components:128,139 fused into conv2's launch: the 1x1 tiles ([cx/32][cout_pad][32]) precede the 3x3 tiles
                # (a second copy: the unfused fallback — split-K at small batch — keeps reading cw.w)
                w = self._f32(blk.res_conv.weight)
                c2.w_fused = torch.cat([self._pack_weight(w, None, self.dt, c2.Cout, cx, cx, 1, 1, c2.cout_pad), c2.w])
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
        P["init"] = self._pack_conv(m.init_conv.weight, m.init_conv.bias, cin_pad=self.cin0)      # (+ the 7x7 kernel's forms: init7_fits)
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
        if self.launch_batch is not None:
            key += ("pin", self.launch_batch)          # (a plan records the decisions of the pin it was built under)
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
            if self.hip_graph and plan.prof is None and not L.lib_path().endswith("_bounds.so"):
                plan.run_graphed(x, time, cond, out)
            else:
                plan.run(x, time, cond, out)
        return out


class _PlanBuilder(_PlanBase):
    """The U-Net graph (model/diffusion.py:187-258) as a plan."""

    def __init__(self, eng, B, H, W, has_cond, paired=False):
        super().__init__(eng, B, H, W)
        self.has_cond, self.paired = has_cond, paired
        self._graph = None       # run_graphed(): the captured HIP graph

    # ---------------------------------------------------------------- inspection
    def launch_signature(self):
        """What the recorded launches DECIDED, for tests that ask which batches take the same code paths: (categorical, counts).
        categorical: one tuple per op, never addresses or sizes that merely scale with the batch —
          convolutions: (name, tile, K slices, flags, res_steps, two samples per block [the halo kernel's pair predicate, restated]);
          ds_dwconv7: (name, kernel family, row ranges / chunks per image, a chunk covers several samples) from ds_dwconv_launch_choice;
          attention: (name, generations of the two passes [ds_attn_fused_generations; 0 elsewhere]) on the context op;
          anything else: (name,).
        counts: per attention block (segments of the context pass, GroupNorm partials per sample of the output pass) in op order — budgets
        divided by the batch, kept apart because they change at almost every batch.  Read-only; works on a dry build."""
        cat, counts = [], []
        lib = self.lib
        for op in self.ops:
            name = op.name
            ref = op.args[0]                                   # (of the ops looked into below: the C.byref of the parameter struct)
            if name in ("ds_conv_igemm", "ds_conv1x1_x3"):
                p = ref._obj
                ks = max(1, p.ksplit)
                # conv3x3_halo3.hip, ds_conv_igemm's halo3 dispatch: the 8 x 32 tile holds two images of at most 16 x 8
                pair = bool(name == "ds_conv_igemm" and p.tile == L.TILE_HALO3_256x96 and p.flags != 0 and p.W <= 8 and 2 * p.H <= 32
                            and ks == 1 and not p.res_steps and (p.batch_hint or p.B) >= 2)
                cat.append((name, p.tile, ks, p.flags, p.res_steps, pair))
            elif name == "ds_dwconv7":
                fam, ranges, spc = C.c_int32(), C.c_int32(), C.c_int32()
                L.call("ds_dwconv_launch_choice", ref, C.byref(fam), C.byref(ranges), C.byref(spc))
                cat.append((name, L.DW_FAMILY[fam.value], ranges.value, spc.value > 1))
            elif name == "ds_attn_fused_context":
                counts.append((ref._obj.nseg, lib.ds_attn_fused_stats_parts(ref)))
                cat.append((name, lib.ds_attn_fused_generations(ref)))
            elif name == "ds_attn_x3_context":
                counts.append((ref._obj.nseg, lib.ds_attn_x3_stats_parts(ref)))
                cat.append((name, 0))
            elif name == "ds_linattn_context":
                counts.append((ref._obj.nseg, 0))
                cat.append((name, 0))
            else:
                cat.append((name,))
        return tuple(cat), tuple(counts)

    # ---------------------------------------------------------------- blocks
    def dup(self, a):
        """Both halves of a full-batch activation = the half-batch activation ``a`` (incl. its GroupNorm partials); self.B is the full batch."""
        nb = (self.B // 2) * a.H * a.W * a.C * self.e.es
        # r05: `a` was carved at full size (act() while alloc_B is set) and holds the prefix in its first half: one read + one write
        assert a.nbytes >= 2 * nb, "dup() of a tensor not carved at the full batch"
        out = _Act(a.off, a.nbytes, a.C, a.H, a.W)
        out.split = a.split
        self.op("ds_dup_batch", a.off, a.off, nb)
        a.nbytes = 0                                  # (ownership of the bytes moved to `out`: free(a) releases nothing)
        if a.stats is not None:
            st, parts = self._partials(a, "dup")
            ns = self.raw(self.B * parts * 2 * 4)
            self.op("ds_dup_batch", st[0], ns[0], (self.B // 2) * parts * 2 * 4)
            out.stats = _Partials(ns, parts)
        return out

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
                           wexp=L.ptr(d["dw_exp"]),
                           batch_hint=self.Btile)      # (kernel family and row ranges / chunks per image: by the FULL batch, like split-K)
        # split-precision tier: the two tensors only 3x3 convolutions read (h, g) are stored as hi / lo bf16 planes
        sp = (self._split_takes(d["conv1"]) and self._split_takes(d["conv2"]) and s0.C % 16 == 0 and (s1 is None or s1.C % 16 == 0))
        if sp:
            p.out_split, h.split = 1, True
        parts = self.lib.ds_dwconv_stats_parts(C.byref(p))
        st = self.raw(B * parts * 2 * 4)
        p.stats_part = st[0]
        h.stats = _Partials(st, parts)
        self.op("ds_dwconv7", C.byref(p))
        src1_, st1 = self.stats_src(h, dim * H * W)
        g = self.conv(d["conv1"], h, pad=1, gn_src=src1_, act=L.ACT_GELU, want_stats=True, out_split=sp)
        self.free(h)
        self.free_raw(st1)
        src2_, st2 = self.stats_src(g, d["conv1"].Cout * H * W)
        c2 = d["conv2"]
        if c2.res_steps and self._halo3_ksplit(c2, g, g.split) == 1:          # (res_steps: the block's res_conv is packed in front)
            out = self.conv(c2, g, pad=1, gn_src=src2_, want_stats=want_stats, res_fuse=(s0, s1, off1))
        else:
            out = self.conv(d["res"], s0, s1, off1) if d["res"] is not None else None      # 1x1 res_conv straight into the output buffer
            out = self.conv(c2, g, pad=1, gn_src=src2_, res=s0 if out is None else out, want_stats=want_stats, out=out)
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
        a.stats = _Finished(ab)

    def block(self, d, x, want_stats=False):
        return self.convnext(d, x, want_stats) if self.e.cfg["use_convnext"] else self.resnet(d, x, want_stats)

    def attention(self, d, x, planes=None):
        """Residual(PreNorm(LinearCrossAttention[Add])) — components:22-29,142-152,171-207,252-293.
        planes (split-precision tier): "both" = the output additionally as hi / lo planes (out.planes), "only" = as planes alone
        (returned activation has .split set) — what the Down / Upsample that follows reads; ignored elsewhere."""
        e, B = self.e, self.B
        N, Cc = x.H * x.W, x.C
        xsrc, xst, abx = None, None, (None, 0)       # the PreNorm statistics of x: partials the attention kernel reduces itself, or finished (abx)
        if isinstance(x.stats, _Finished):           # (a ResNet block in front: _direct_stats)
            abx, x.stats = x.stats.buf, None
        elif d["fused"] is not None or d["x3"] is not None:
            xsrc, xst = self.stats_src(x, Cc * N)
        else:
            abx = self.finalize(x, Cc * N)
        lazy = xsrc is not None
        heads = 4
        nseg = max(1, min(N // 1024, 16))          # function of N only (batch-invariant results)
        if d["x3"] is not None:
            return self._attention_x3(d, x, abx, xsrc, xst, planes)
        if d["fused"] is not None:
            # one input stream: k/v projection + softmax_n + k.v^T, then q projection + softmax_d + ctx^T.q + to_out
            # segments of partials: the library's choice for this shape and batch — N / 128 <= 32 for the first-generation context pass, one
            # round of blocks (one segment per wave) for the second generation, which it runs from U-Net batch 96 on (the bf16 tier's second
            # tiling decision that looks at B, after split-K)
            nseg = self.lib.ds_attn_fused_segments(self.Btile, N, Cc)
            part = self.raw(self.lib.ds_linattn_part_floats(B, heads, nseg) * 4)
            ctx = self.raw(B * heads * 1024 * 4)
            y = self.act(Cc, x.H, x.W)
            lab = self.lab_all[0] if self.lab_all else None
            fp = L.AttnFusedParams(x=x.off, B=B, N=N, C=Cc, nseg=nseg, wqkv=d["fused"][0].data_ptr(), t1=d["qkv"].t1.data_ptr(),
                                   t2=d["qkv"].t2.data_ptr(), gn_ab=abx[0], label_q=(lab + 4 * d["l_off"]) if lab else None,
                                   lq_stride=e._lab_total, scale=32 ** -0.5, part=part[0], ctx=ctx[0],
                                   wout_perm=d["fused"][1].data_ptr(), bias_out=d["out"].bias.data_ptr(), y=y.off, stats_part=None,
                                   batch_hint=self.Btile)
            if lazy:
                fp.gn_ab, fp.gn_part, fp.gn_parts, fp.gn_count, fp.gn_eps = None, xsrc[0], xsrc[1], float(xsrc[2]), xsrc[3]
            mfold = self.raw(B * Cc * 128 * 2) if Cc in (96, 192) else None      # to_out folded into the context (attn_out2.hpp)
            fp.mfold = mfold[0] if mfold is not None else None
            parts = self.lib.ds_attn_fused_stats_parts(C.byref(fp))
            st = self.raw(B * parts * 2 * 4)
            fp.stats_part = st[0]
            y.stats = _Partials(st, parts)
            self.op("ds_attn_fused_context", C.byref(fp))
            self.op("ds_attn_fused_output", C.byref(fp))
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
            self.op("ds_gn_apply", C.byref(g))
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
        self.op("ds_linattn_context", C.byref(p))
        self.op("ds_linattn_output", C.byref(p))
        self.free(qkv)
        self.free_raw(part)
        self.free_raw(ctx)
        y = self.conv(d["out"], ao, want_stats=True)
        self.free(ao)
        aby = self.finalize(y, Cc * N)
        out = self.act(Cc, x.H, x.W)
        g = L.GnApplyParams(x=y.off, res=x.off, out=out.off, gn_ab=aby[0], gamma=d["on"][0].data_ptr(),
                            beta=d["on"][1].data_ptr(), cbias=None, cb_stride=0, B=B, HW=N, C=Cc, G=1, act=L.ACT_NONE, dtype=e.dt)
        self.op("ds_gn_apply", C.byref(g))
        self.free(y)
        self.free_raw(aby)
        return out

    def _attention_x3(self, d, x, abx, xsrc, xst, planes=None):
        """The block in the split-precision tier (attn_x3.hip): x (fp32) is the only activation stream — k / v / q projections, both
        softmaxes, ctx and to_out as three-term bf16 MFMA products, and the output GroupNorm + residual applied while y is computed a
        second time (ds_attn_x3_output form B: no y tensor, no apply pass; +1.15 % on the step against form A + ds_gn_apply, same box —
        after the statistics-only pass lost the 644 bytes of scratch that made it slower than the pass that writes y)."""
        e, B = self.e, self.B
        N, Cc = x.H * x.W, x.C
        lib, lazy = self.lib, xsrc is not None
        nseg = lib.ds_attn_x3_segments(self.Btile, N, Cc)          # (segments and blocks per sample by the decision batch; buffers by B)
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
                            out_planes=(pl.off if pl is not None else None), batch_hint=self.Btile)
        if lazy:
            fp.gn_ab, fp.gn_part, fp.gn_parts, fp.gn_count, fp.gn_eps = None, xsrc[0], xsrc[1], float(xsrc[2]), xsrc[3]
        parts = lib.ds_attn_x3_stats_parts(C.byref(fp))
        st = self.raw(B * parts * 2 * 4)
        fp.stats_part = st[0]
        self.op("ds_attn_x3_context", C.byref(fp))
        self.op("ds_attn_x3_output", C.byref(fp))
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
        self.sin = self.h1 = self.temb = None
        if e.m.time_mlp is not None:
            half = cfg["down_dims"][0] // 2
            td = cfg["time_dim"]
            self.sin = self.raw(B * 2 * half * 4)
            self.h1 = self.raw(B * td * 4)
            self.temb = self.raw(B * td * 4)
            self.op("ds_sinusoid", None, e.freqs.data_ptr(), B, half, self.sin[0], late=((0, _TIME),))
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
            self.cemb = None                           # (nn.Embedding: forward() looked the rows up, the labels GEMV reads `cond` itself)
            if e.emb_is_linear:
                self.cemb = self.raw(B * ld * 4)
                self.op("ds_linear", None, ld, e.emb_w.data_ptr(), e.emb_b.data_ptr(), B, ld, ld, L.ACT_NONE, self.cemb[0], ld, late=((0, _COND),))
            self.lab_all = self.raw(B * e._lab_total * 4)
            self.op("ds_linear", self.cemb[0] if self.cemb else None, ld, e.lab_W.data_ptr(), e.lab_b.data_ptr(), B, ld, e._lab_total, L.ACT_NONE,
                    self.lab_all[0], e._lab_total, late=None if self.cemb else ((0, _COND),))

        # --- trunk
        self.n_cond = len(self.ops)                    # ops [0, n_cond) read (time, condition) only: the conditioning GEMVs
        # classifier-free guidance evaluates cat([x, x]) with cat([uncond, cond]): the two halves are the same computation until the first
        # attention block adds the label query — the init convolution and the first block run ONCE, at half the batch, and their two results
        # (the skip tensor and the block output with its GroupNorm partials) are duplicated (ds_dup_batch).  Bit-identical to the plain plan:
        # every decision of these layers that looks at the batch is taken from the full batch (self.Btile) — the split-K factors, and the
        # depthwise launch's kernel family and row ranges / chunks per image (ds_dwconv_params.batch_hint) — so the prefix groups its partial
        # sums as the plain plan does; everything else depends on the layer shape only (tests/test_hip_batch_ladder.py compares the two
        # plans' launch_signature() at every even batch up to 256 and their output bits on a ladder of batches).
        Bfull = self.B
        half = self.paired and len(P["downs"]) > 0
        if half:
            self.B = B = Bfull // 2
            self.alloc_B = Bfull
        xin = self.act(e.cin0, H, W)
        self.op("ds_nchw_to_nhwc", None, self.B, cfg["in_dim"], H, W, xin.off, e.cin0, e.dt, late=((0, _X),))
        cw = P["init"]
        if cw.w_init7 is not None:
            x = self.act(96, H, W)
            self.conv_meta[len(self.ops)] = policy.conv_meta(L.TILE_INIT7, B, H, W, 96, 7, 7, False, cw.cin_real, cw.cin_real)
            self.op("ds_conv7x7_c4", xin.off, B, H, W, e.cin0, cw.w_init7.data_ptr(), L.ptr(cw.bias), x.off)
        elif cw.w_init7x3 is not None:
            x = self.act(96, H, W)
            self.op("ds_conv7x7_c4_x3", xin.off, B, H, W, cw.w_init7x3.data_ptr(), L.ptr(cw.bias), x.off)
        else:
            x = self.conv(cw, xin, pad=3)
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
            x = self.attention(a2, y, planes="both" if (e.split3 and self._quad_takes(down, y, stride=2, pad=1)) else None)
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
                x = self.attention(at, y, planes="only" if (do_up and e.split3 and self._quad_takes(up, y)) else None)
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
        self.op("ds_nhwc_to_nchw", z.off, e.dt, B, cfg["out_dim"], z.C, H, W, None, late=((7, _OUT),))
        self.free(z)

    # ---------------------------------------------------------------- execution
    def run_graphed(self, x, time, cond, out):
        """run() captured once as a HIP graph over static input / output buffers, then replayed (ConditionedUnet.use_hip_graph)."""
        g = self._graph
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
        st = L.current_stream()
        tensors, prof = (x, time, cond, out), self._prof_now()
        # The conditioning GEMVs (0.36 ms at U-Net batch 128: five latency-bound launches) depend on (time, condition) only: at
        # large batches they run on a side stream under the layout change + init convolution of the trunk.
        e, side, cond_st = self.e, None, st
        if self.n_cond > 0 and self.B * self.H * self.W >= 65536:
            if e.side_stream is None:
                e.side_stream = torch.cuda.Stream()
            side = e.side_stream
            side.wait_stream(torch.cuda.current_stream())
            cond_st = side.cuda_stream
        self.launch(0, self.n_cond, cond_st, tensors, prof)
        self.launch(self.n_cond, self.n_cond_join, st, tensors, prof)
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        self.launch(self.n_cond_join, len(self.ops), st, tensors, prof)
