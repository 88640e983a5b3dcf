"""SamplingBatcher — concurrent sampler calls sharing U-Net steps.

Every caller of the reference builds its own DiffSynthSampler and runs one call to completion (text2sound, sound2sound,
inpainting, one batch-1 ``inpaint_sample`` per note of the MIDI arranger).  A batch-1 step leaves most of the card idle
(DESIGN.md §5), so this module runs many such calls together: each call is submitted with the sampler it would have been
run on, and every tick advances every active call by one step with ONE U-Net forward per bucket and ONE ``ds_step_rows``
launch per bucket that applies each row's own guidance scale, coefficients, inpaint blend and step noise.  Requests of the
"dpmpp_2m" sampler share buckets and U-Net batches with the others: their rows are stepped by one ``ds_dpm_step_rows`` launch per
bucket, each request on history rows of its own that stay where they are for the request's lifetime.  Requests whose sampler has
a guidance rescale (``activate_classifier_free_guidance(..., guidance_rescale=phi)``) get their combined eps from one
``ds_cfg_rescale_rows`` launch per bucket in front of the step launches, written over their unconditional eps rows.  Requests whose
sampler has a condition mix (``set_condition_mix``: K prompts per sample) occupy ``B * (1 + K)`` U-Net rows and get theirs from one
``ds_cfg_compose_rows`` launch per bucket beside it (a request is in exactly one of the two); one ``ds_copy_rows`` launch per bucket
then writes the copies of their state rows that the step kernel's one duplicate does not cover.  An ``"edit_sample"`` request
(``submit(dss, "edit_sample", inv, condition=c)``) is a "ddpm" request whose step noise is given: its rows read ``inv.z[k]`` as a raw
draw of its own width through an identity column table, and it reserves no counters and draws nothing.  On a windowed model
(``diffusynth_amd.windowed.WindowedUnet``: a wide state is evaluated as ``rows_per_sample(width)`` windows per row) nothing of this
changes but the accounting: a request's rows count that many times against ``max_rows``.

    b = SamplingBatcher(unet, max_rows=128)
    h = b.submit(dss, "inpaint_sample", shape, 0.7, guide, mask, condition=c, sampler="ddpm", use_dynamic_mask=True, seed=7)
    b.run()
    imgs, initial_noise = h.result()

A call's arguments and return values are those of ``getattr(dss, method)(unet, ...)``.  The call's prologue (initial noise,
guide, q_sample, masks, step list, coefficient tables) is the sampler's own (``DiffSynthSampler._loop_prologue``); its draws
come from a private ``torch.Generator`` (or the sampler's Philox stream), so a request's noise does not depend on the other
requests.  In the fp32 tier no tiling choice of the U-Net depends on the batch, so a request's result is the same bits as the
call run alone — and so it is in the bf16x3 / bf16 tiers on a model pinned with ``unet.pin_launch_batch(max_rows)`` (every launch
decision then looks at the pin, not at the batch; the batcher needs no argument for it).  Unpinned, in the bf16x3 / bf16 tiers
split-K factors and attention segment counts follow the U-Net batch, so a result
depends on its batch mates within the tier's error contract (a batcher that holds one request is the standalone call).

Buckets: one per (height, width, has_condition).  A tick runs every non-empty bucket: the U-Net batch is every request's rows
plus, for classifier-free guidance (CFG), one unconditional row per row.  When every request of a bucket uses CFG the batch is
laid out as the standalone call lays it out, ``[x; x]`` with ``paired_halves=True``; otherwise each CFG request contributes
``[x (unconditional); x (conditional)]`` next to the plain rows of the others.  The step kernel writes the next U-Net input
(duplicate rows included) directly; the batch is re-laid only when requests join or leave.
"""
import ctypes as C
import inspect
import time as _time
from collections import deque

import numpy as np
import torch

from . import _lib as L
from .sampler import LOOP_PROGRAM

METHODS = ("sample", "img_guided_sample", "inpaint_sample", "interpolate", "edit_sample")
_NOISE_NONE, _NOISE_DRAW, _NOISE_PHILOX = 0, 1, 2


def _seed_from_global():
    """One draw of torch's global generator: the seed of a request submitted with seed=None (not reproducible, as in the reference)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def request_program(dss, method, *args, **kwargs):
    """(LoopProgram, bound arguments) of ``getattr(dss, method)(model, *args, **kwargs)``: what the call computes before its first
    model call (DiffSynthSampler._loop_prologue), with the draws on the sampler's current generator.  Runs on CPU samplers too."""
    if method not in METHODS:
        raise ValueError("method must be one of %s, got %r" % (", ".join(METHODS), method))
    fn = getattr(dss, method)
    bound = inspect.signature(fn).bind(LOOP_PROGRAM, *args, **kwargs)
    bound.apply_defaults()
    return fn(LOOP_PROGRAM, *args, **kwargs), bound.arguments


class SamplingHandle:
    """One submitted call.  ``result()`` returns what the call returns (running the batcher until this call is done)."""

    def __init__(self, batcher, req):
        self._batcher, self._req = batcher, req

    def done(self):
        return self._req.out is not None

    def result(self):
        while self._req.out is None:
            self._batcher.step()
        return self._req.out


class _Request:
    def __init__(self, dss, method, prog, args, unet_dev, rows_per_sample=1):
        self.dss, self.method, self.prog = dss, method, prog
        self.B, self.C, self.H, self.W = prog.shape
        self.mix = dss._mix                         # condition mix (set_condition_mix): (K,) or (K, W) float32, or None
        self.cfg = dss.CFG != 1.0 or self.mix is not None       # the request has unconditional rows
        self.K = (1 if self.mix is None else self.mix.shape[0]) if self.cfg else 0      # its conditional row groups
        self.scale = float(dss.CFG)
        self.phi = float(dss.guidance_rescale) if self.cfg else 0.0     # guidance rescale (applied under CFG only, as in the sampler)
        self.batch_rows = self.B * (1 + self.K)     # its rows in the bucket's batch
        self.unet_rows = self.batch_rows * rows_per_sample          # what the U-Net runs for them (a windowed model: a row per window)
        self.sampler = prog.sampler
        self.given = prog.step_noise is not None    # "edit_sample": the step noise is prog.step_noise[k], nothing is drawn
        cond = args["condition"]
        self.cond = None if cond is None else cond.to(unet_dev)
        self.uncond = None
        if self.cfg:
            u = dss.unconditional_condition
            self.uncond = u.unsqueeze(0).repeat(*([self.B] + [1] * len(u.shape))).to(unet_dev)     # (DiffSynthSampler._predict)
        self.key = (self.H, self.W, self.cond is not None)
        self.k = 0                      # next step
        self.state = prog.img.contiguous().float()
        self.imgs = [prog.img]
        self.out = None
        if self.sampler == "ddpm":
            self.draw_w, self.cols = (self.W, list(range(self.W))) if self.given else dss._step_noise_layout(self.W)
        self.solver = self.sampler == "dpmpp_2m"
        # the solver's history (the previous step's x0 prediction): the request's own rows, never part of the bucket's re-laid tensors
        self.hist = torch.empty(prog.shape, dtype=torch.float32, device=self.state.device) if self.solver else None
        self.mapped = [int(dss.timestep_map[i]) for i in prog.steps]


class _Bucket:
    def __init__(self, key):
        self.key = key
        self.reqs = []
        self.dirty = True               # the request set changed: the U-Net input is re-laid at the next tick
        self.x = None                   # the U-Net input of the next tick (written by the previous tick's ds_step_rows)


class _Tables:
    """The one upload of a bucket tick, each part at a 16-byte boundary: the U-Net timesteps, the DS_SR_* tables of the R step rows
    (rows [0, R1): ds_step_rows, [R1, R): ds_dpm_step_rows), the history addresses of the solver rows, the column tables of the DDPM
    requests (one per distinct layout), the DS_CR_* tables of the Rg rows of the ds_cfg_rescale_rows launch (guidance rescale), the
    DS_CC_* tables and the weights of the Rm rows of the ds_cfg_compose_rows launch (condition mixes: one weight table per request)
    and the Rp (src, dst) pairs of the ds_copy_rows launch (the copies of a state row beyond the step kernel's one duplicate)."""

    def __init__(self, reqs, Bu):
        self.R = R = sum(r.B for r in reqs)
        self.R1 = R1 = sum(r.B for r in reqs if not r.solver)
        self.Rg = Rg = sum(r.B for r in reqs if r.phi > 0.0 and r.mix is None)
        self.Rm = Rm = sum(r.B for r in reqs if r.mix is not None)
        self.Rp = Rp = sum(r.B * (r.K - 1) for r in reqs if r.mix is not None)
        self.n_wt = n_wt = sum(r.mix.size for r in reqs if r.mix is not None)
        self.col_tabs, self.n_cols = {}, 0          # layout -> offset of its columns in cols
        for r in reqs:
            if r.sampler == "ddpm" and tuple(r.cols) not in self.col_tabs:
                self.col_tabs[tuple(r.cols)] = self.n_cols
                self.n_cols += len(r.cols)
        self.parts = {"tim": (np.int64, (Bu,), 0), "irow": (np.int32, (R, L.SR["DS_SR_NI"]), 0),        # name: (type, shape, floor)
                      "frow": (np.float32, (R, L.SR["DS_SR_NF"]), 0), "prow": (np.uint64, (R, L.SR["DS_SR_NP"]), 0),
                      "hrow": (np.uint64, (R - R1,), 1), "cols": (np.int32, (max(self.n_cols, 1),), 1),
                      "girow": (np.int32, (Rg, L.CR["DS_CR_NI"]), 0), "gfrow": (np.float32, (Rg, L.CR["DS_CR_NF"]), 0),
                      "mirow": (np.int32, (Rm, L.CC["DS_CC_NI"]), 0), "mfrow": (np.float32, (Rm, L.CC["DS_CC_NF"]), 0),
                      "mwt": (np.float32, (n_wt,), 0), "pairs": (np.int32, (Rp, 2), 0)}
        self.off, o = {}, 0                                             # part -> its byte offset in the upload
        for name, (dt, shape, floor) in self.parts.items():             # (floor: the least number of elements the part reserves)
            self.off[name] = o
            o += (np.dtype(dt).itemsize * max(int(np.prod(shape)), floor) + 15) & ~15
        self.nbytes = o

    def bind(self, hb):
        """Numpy views of the parts in the staged bytes ``hb`` (attributes tim, irow, ..., pairs); writes the column tables."""
        for name, (dt, shape, _) in self.parts.items():
            o = self.off[name]
            setattr(self, name, hb[o:o + np.dtype(dt).itemsize * int(np.prod(shape))].view(dt).reshape(shape))
        for key, off in self.col_tabs.items():
            self.cols[off:off + len(key)] = key

    def at(self, dev, name, row=0):                 # device address of row ``row`` of a part in the uploaded bytes ``dev``
        dt, shape, _ = self.parts[name]
        return dev.data_ptr() + self.off[name] + row * np.dtype(dt).itemsize * int(np.prod(shape[1:]))


class SamplingBatcher:
    """See the module docstring.  ``max_rows`` bounds the U-Net rows (CFG rows counted twice, rows of a K-prompt mix 1 + K times, and on a
    windowed model — diffusynth_amd.windowed.WindowedUnet — every row ``unet.rows_per_sample(width)`` times: a row per window) of all requests in flight and
    ``max_buckets`` (default: the number of plans the U-Net's engine keeps, DS_MAX_PLANS) the buckets live at once; requests are
    admitted first in, first out at the start of a tick, and a request that does not fit waits (and holds back the ones after it).
    Not thread-safe; the U-Net is run on the current stream."""

    def __init__(self, unet, max_rows=128, max_buckets=None):
        from .engine import max_plans
        self.unet = unet
        self.max_rows = int(max_rows)
        if self.max_rows < 1:
            raise ValueError("max_rows must be >= 1")
        # a tick visits every live bucket, one U-Net plan each: more live buckets than the engine keeps plans would rebuild every
        # plan on every tick (LRU round robin), so admission holds a request of a new bucket while this many are live
        self.max_buckets = max_plans() if max_buckets is None else int(max_buckets)
        if self.max_buckets < 1:
            raise ValueError("max_buckets must be >= 1")
        self.dev = next(unet.parameters()).device
        self._pending = deque()
        self._buckets = {}
        self._inflight = set()
        self._geometry = None           # (height, channels) shared by every request in flight
        self._stage = [None, None]      # double-buffered pinned staging of the per-tick upload: (host tensor, event)
        self._flip = 0
        self.ticks = 0
        self.plan_builds = 0
        self.host_seconds = 0.0
        self.unet_batches = set()       # distinct (U-Net rows, H, W, has condition, paired) the ticks have run

    # ------------------------------------------------------------------ submission
    def submit(self, dss, method, /, *args, **kwargs):
        """Queue ``getattr(dss, method)(unet, *args, **kwargs)``; returns a SamplingHandle.  Rejected here: an unknown method, a
        sampler already in flight, a sharded sampler, more U-Net rows than max_rows, and a height / channel count that differs from
        the requests in flight.  The call's prologue (its noise draws included) runs now."""
        if method not in METHODS:
            raise ValueError("method must be one of %s, got %r" % (", ".join(METHODS), method))
        if id(dss) in self._inflight:
            raise RuntimeError("this DiffSynthSampler already has a call in flight; build one sampler per concurrent call")
        if dss.shard is not None:
            raise ValueError("sharded samplers (shard=) are served by diffusynth_amd.dist, not by the batcher")
        bound = inspect.signature(getattr(dss, method)).bind(LOOP_PROGRAM, *args, **kwargs)
        bound.apply_defaults()
        a = bound.arguments
        shape = tuple(int(v) for v in (a["inv"].shape if method == "edit_sample" else a["shape"]))
        if self._geometry is not None:
            assert shape[1] == self._geometry[1] and dss.channels == self._geometry[1], "shape[1] != self.channels"
            assert shape[2] == self._geometry[0] and dss.height == self._geometry[0], "shape[2] != self.height"
        cfg = dss.CFG != 1.0
        rps = self._rows_per_sample(shape[3])
        rows = shape[0] * ((2 if cfg else 1) if dss._mix is None else 1 + dss._mix.shape[0]) * rps
        if rows > self.max_rows:
            raise ValueError("the request needs %d U-Net rows, more than max_rows=%d" % (rows, self.max_rows))
        if cfg and a["condition"] is None:
            raise ValueError("classifier-free guidance (CFG != 1) needs a condition")
        # every batched call gets a private generator: the entry point's _seed(seed) then seeds it instead of torch's global
        # generators.  A Philox call draws nothing from it (its noise is the sampler's counter stream), so it lives on the CPU.
        if dss.noise_device == "philox":
            dss._generator = torch.Generator()
        else:
            dss._generator = torch.Generator(device=dss.device if dss.noise_device is None else dss.noise_device)
            if a.get("seed") is None and method != "edit_sample":        # (an edit draws nothing: it takes no seed)
                dss._generator.manual_seed(_seed_from_global())
        try:
            prog = getattr(dss, method)(LOOP_PROGRAM, *args, **kwargs)
            req = _Request(dss, method, prog, a, self.dev, rps)
        except BaseException:
            dss._generator = None
            raise
        self._inflight.add(id(dss))
        self._geometry = (req.H, req.C)
        h = SamplingHandle(self, req)
        if not prog.steps:                          # nothing to run (start == end): the call's result is its prologue
            self._retire(req)
        else:
            self._pending.append(req)
        return h

    def _rows_per_sample(self, W):
        """U-Net rows per batch row at width W: 1, or the number of windows of a windowed model (diffusynth_amd.windowed)."""
        rps = getattr(self.unet, "rows_per_sample", None)
        return 1 if rps is None else int(rps(W))

    def _retire(self, req):
        req.out = (req.imgs, req.prog.initial_noise)
        req.dss._generator = None
        self._inflight.discard(id(req.dss))
        if not self._inflight:
            self._geometry = None

    # ------------------------------------------------------------------ ticks
    def active(self):
        return sum(len(b.reqs) for b in self._buckets.values()) + len(self._pending)

    def run(self):
        while self.active():
            self.step()

    @torch.no_grad()
    def step(self):
        """One tick: admit waiting requests, then advance every active request by one step."""
        t0 = _time.perf_counter()
        used = sum(r.unet_rows for b in self._buckets.values() for r in b.reqs)
        while self._pending and used + self._pending[0].unet_rows <= self.max_rows:
            if self._pending[0].key not in self._buckets and len(self._buckets) >= self.max_buckets:
                break
            r = self._pending.popleft()
            b = self._buckets.get(r.key)
            if b is None:
                b = self._buckets[r.key] = _Bucket(r.key)
            b.reqs.append(r)
            b.dirty = True
            used += r.unet_rows
        eng = self.unet._engine
        builds0 = getattr(eng, "plan_builds", 0) if eng is not None else 0
        for key in list(self._buckets):
            b = self._buckets[key]
            if b.reqs:
                self._tick(b)
            if not b.reqs:
                del self._buckets[key]
        eng2 = self.unet._engine
        if eng2 is not None:
            self.plan_builds += eng2.plan_builds - (builds0 if eng2 is eng else 0)
        self.ticks += 1
        self.host_seconds += _time.perf_counter() - t0

    def _layout(self, b):
        """Row layout of the bucket's U-Net batch: per request (x row of its first state row, eps row, conditional eps row or -1,
        duplicate row or -1), the U-Net batch size and whether it is the paired [x; x] form.  A condition mix of K prompts lies
        as [u rows; c_1 rows; ...; c_K rows]: its further conditional groups follow the first at a distance of B rows each, and a
        bucket that holds one with K >= 2 is not paired."""
        paired = all(r.K == 1 for r in b.reqs)
        lay, base = [], 0
        if paired:
            n = sum(r.B for r in b.reqs)
            for r in b.reqs:
                lay.append((base, base, n + base, n + base))
                base += r.B
            return lay, 2 * n, True
        for r in b.reqs:
            if r.cfg:
                lay.append((base, base, base + r.B, base + r.B))
            else:
                lay.append((base, base, -1, -1))
            base += r.batch_rows
        return lay, base, False

    def _relayout(self, b):
        b.lay, b.Bu, b.paired = self._layout(b)
        xs, conds = [], []
        if b.paired:
            xs = [r.state for r in b.reqs] * 2
            if b.key[2]:
                conds = [r.uncond for r in b.reqs] + [r.cond if r.mix is None else r.cond[:, 0] for r in b.reqs]
        else:
            for r in b.reqs:
                xs += [r.state] * (1 + r.K)
                if b.key[2]:
                    if r.mix is not None:
                        conds += [r.uncond] + [r.cond[:, k] for k in range(r.K)]
                    else:
                        conds += [r.uncond, r.cond] if r.cfg else [r.cond]
        b.x = torch.cat(xs, 0).contiguous()
        b.cond = torch.cat(conds, 0).contiguous() if conds else None
        b.dirty = False

    def _staging(self, nbytes):
        """A pinned host buffer of >= nbytes whose previous upload has completed (two alternate)."""
        i = self._flip
        self._flip ^= 1
        st = self._stage[i]
        if st is None or st[0].numel() < nbytes:
            st = self._stage[i] = (torch.empty(max(nbytes, 1 << 16) * 2, dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
        else:
            st[1].synchronize()
        return st

    def _fill_rows(self, b, tb):
        """The table rows of every request of the bucket, in layout order.  Returns the tensors the launches must keep alive."""
        S, CR, CC, (H, W), Cc = L.SR, L.CR, L.CC, b.key[:2], b.reqs[0].C
        CHW = Cc * H * W
        keep = []
        nxt = [0, tb.R1]                # next table row of a ds_step_rows request, of a solver request
        gnxt = 0                        # next row of the rescale tables
        mnxt = wnxt = pnxt = 0          # next row of the compose tables, next weight, next copy pair
        for r, (x0, e0, ec0, d0) in zip(b.reqs, b.lay):
            k, B, prog = r.k, r.B, r.prog
            row = nxt[r.solver]
            nxt[r.solver] += B
            sl = slice(row, row + B)
            ar = np.arange(B, dtype=np.int32)
            ar64 = ar.astype(np.uint64)
            tb.tim[x0:x0 + B] = r.mapped[k]
            if r.cfg:
                tb.tim[ec0:ec0 + B * r.K] = r.mapped[k]
            irow, frow, prow = tb.irow[sl], tb.frow[sl], tb.prow[sl]
            irow[:] = 0
            irow[:, S["DS_SR_X"]] = x0 + ar
            irow[:, S["DS_SR_EPS"]] = e0 + ar
            if r.mix is not None:       # the compose launch combines into the unconditional eps rows: the step sees a plain eps
                msl = slice(mnxt, mnxt + B)
                mnxt += B
                tb.mirow[msl, CC["DS_CC_U"]] = tb.mirow[msl, CC["DS_CC_OUT"]] = e0 + ar
                tb.mirow[msl, CC["DS_CC_K"]], tb.mirow[msl, CC["DS_CC_C0"]], tb.mirow[msl, CC["DS_CC_CSTRIDE"]] = r.K, ec0 + ar, B
                tb.mirow[msl, CC["DS_CC_WT"]], tb.mirow[msl, CC["DS_CC_WTW"]] = wnxt, r.mix.size // r.K
                tb.mfrow[msl, CC["DS_CC_SCALE"]], tb.mfrow[msl, CC["DS_CC_PHI"]] = r.scale, r.phi
                tb.mwt[wnxt:wnxt + r.mix.size] = r.mix.ravel()
                wnxt += r.mix.size
                for j in range(1, r.K):     # the step launch writes the state row and one duplicate; ds_copy_rows the other K - 1
                    tb.pairs[pnxt:pnxt + B, 0], tb.pairs[pnxt:pnxt + B, 1] = x0 + ar, d0 + j * B + ar
                    pnxt += B
                irow[:, S["DS_SR_EPSC"]] = -1
            elif r.phi > 0.0:           # the rescale launch combines into the unconditional eps rows: the step sees a plain eps
                gsl = slice(gnxt, gnxt + B)
                gnxt += B
                tb.girow[gsl, CR["DS_CR_U"]] = tb.girow[gsl, CR["DS_CR_OUT"]] = e0 + ar
                tb.girow[gsl, CR["DS_CR_C"]] = ec0 + ar
                tb.gfrow[gsl, CR["DS_CR_SCALE"]], tb.gfrow[gsl, CR["DS_CR_PHI"]] = r.scale, r.phi
                irow[:, S["DS_SR_EPSC"]] = -1
            else:
                irow[:, S["DS_SR_EPSC"]] = (ec0 + ar) if ec0 >= 0 else -1
            irow[:, S["DS_SR_OUT"]] = x0 + ar
            irow[:, S["DS_SR_DUP"]] = (d0 + ar) if d0 >= 0 else -1
            frow[:] = 0
            frow[:, S["DS_SR_COEF"]:S["DS_SR_COEF"] + 5] = prog.coef_cpu[k].numpy()
            frow[:, S["DS_SR_CFG"]] = r.scale
            prow[:] = 0
            if prog.inpaint:
                mode, m = prog.blends[k]
                irow[:, S["DS_SR_BLEND"]] = mode
                chw = 0 if m.shape[1] == 1 else 1
                irow[:, S["DS_SR_MASK_CHW"]] = chw
                if mode == 1:
                    frow[:, S["DS_SR_Q0"]:S["DS_SR_Q1"] + 1] = prog.q_cpu[k].numpy()
                    prow[:, S["DS_SR_INIT"]] = np.uint64(prog.init.data_ptr()) + np.uint64(4 * CHW) * ar64
                prow[:, S["DS_SR_GUIDE"]] = np.uint64(prog.guide.data_ptr()) + np.uint64(4 * CHW) * ar64
                prow[:, S["DS_SR_MASKP"]] = np.uint64(m.data_ptr()) + np.uint64(4 * (CHW if chw else H * W)) * ar64
            if r.solver:
                tb.hrow[row - tb.R1:row - tb.R1 + B] = np.uint64(r.hist.data_ptr()) + np.uint64(4 * CHW) * ar64
            if r.sampler == "ddpm":
                dss = r.dss
                draw_shape = (dss.max_batchsize, Cc, H, r.draw_w)
                irow[:, S["DS_SR_SAMPLE"]] = ar
                irow[:, S["DS_SR_DRAW_ROWS"]] = dss.max_batchsize
                irow[:, S["DS_SR_DRAW_W"]] = r.draw_w
                irow[:, S["DS_SR_COLS"]] = tb.col_tabs[tuple(r.cols)]
                if r.given:                             # the request's own z[k], read as a draw of B rows of its width
                    irow[:, S["DS_SR_DRAW_ROWS"]] = B
                    irow[:, S["DS_SR_NOISE"]] = _NOISE_DRAW
                    prow[:, S["DS_SR_DRAW"]] = prog.step_noise[k].data_ptr()
                elif dss.noise_device == "philox":        # the kernel computes the draw: only its counters are reserved
                    irow[:, S["DS_SR_NOISE"]] = _NOISE_PHILOX
                    prow[:, S["DS_SR_SEED"]] = dss._philox_seed
                    prow[:, S["DS_SR_OFFSET"]] = dss._philox_take(int(np.prod(draw_shape)))
                else:                                   # the standalone call's draw, on the request's own generator
                    raw = dss._randn(draw_shape, B).contiguous()
                    keep.append(raw)
                    irow[:, S["DS_SR_NOISE"]] = _NOISE_DRAW
                    prow[:, S["DS_SR_DRAW"]] = raw.data_ptr()
        return keep

    def _tick(self, b):
        if b.dirty:
            self._relayout(b)
        reqs, Bu, H, W, Cc = b.reqs, b.Bu, b.key[0], b.key[1], b.reqs[0].C
        tb = _Tables(reqs, Bu)
        host, ev = self._staging(tb.nbytes)
        tb.bind(host.numpy())
        keep = self._fill_rows(b, tb)
        dev = torch.empty(tb.nbytes, dtype=torch.uint8, device=self.dev)
        dev.copy_(host[:tb.nbytes], non_blocking=True)
        ev.record()
        t_dev = dev[tb.off["tim"]:tb.off["tim"] + 8 * Bu].view(torch.int64)
        paired = b.paired and getattr(self.unet, "cfg_paired_halves", False)
        self.unet_batches.add((Bu * self._rows_per_sample(W), H, W, b.key[2], paired))
        eps = self.unet(b.x, t_dev, b.cond, paired_halves=True) if paired else self.unet(b.x, t_dev, b.cond)
        out = torch.empty_like(b.x)
        if tb.Rg:
            g = L.CfgRescaleRowsParams(eps=eps.data_ptr(), irow=tb.at(dev, "girow"), frow=tb.at(dev, "gfrow"), gain=None,
                                       R=tb.Rg, CHW=Cc * H * W, Beps=eps.shape[0])
            L.call("ds_cfg_rescale_rows", C.byref(g), L.current_stream())
        if tb.Rm:
            m = L.CfgComposeRowsParams(eps=eps.data_ptr(), irow=tb.at(dev, "mirow"), frow=tb.at(dev, "mfrow"), wt=tb.at(dev, "mwt"), gain=None,
                                       R=tb.Rm, CHW=Cc * H * W, W=W, Beps=eps.shape[0], n_wt=tb.n_wt)
            L.call("ds_cfg_compose_rows", C.byref(m), L.current_stream())
        for name, first, n, hrow in (("ds_step_rows", 0, tb.R1, ()), ("ds_dpm_step_rows", tb.R1, tb.R - tb.R1, (tb.at(dev, "hrow"),))):
            if n == 0:
                continue
            p = L.StepRowsParams(x=b.x.data_ptr(), eps=eps.data_ptr(), out=out.data_ptr(), irow=tb.at(dev, "irow", first),
                                 frow=tb.at(dev, "frow", first), prow=tb.at(dev, "prow", first), cols=tb.at(dev, "cols") if tb.n_cols else None,
                                 R=n, C=Cc, H=H, W=W, Bx=Bu, Beps=eps.shape[0], Bout=Bu, n_cols=tb.n_cols)
            L.call(name, C.byref(p), *hrow, L.current_stream())
        if tb.Rp:
            L.call("ds_copy_rows", out.data_ptr(), tb.at(dev, "pairs"), tb.Rp, Cc * H * W, Bu, L.current_stream())
        del keep
        b.x = out
        done = []
        for r, (x0, _, _, _) in zip(reqs, b.lay):
            r.state = out[x0:x0 + r.B]
            # (a trajectory entry owns its rows: a view would keep the whole bucket's output alive for as long as the entry lives)
            r.imgs.append(r.state.clone() if r.prog.return_tensor else r.state.cpu().numpy())
            r.k += 1
            if r.k == len(r.prog.steps):
                done.append(r)
        for r in done:
            b.reqs.remove(r)
            self._retire(r)
            b.dirty = True
