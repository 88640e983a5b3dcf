"""SamplingBatcher on the GPU: ds_step_rows against the single-call step kernels, and concurrent sampler calls against the same calls
run alone (bit for bit in the fp32 tier, whatever shares the batch and whenever it was submitted)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err, rel_errs
from diffusynth_amd import _lib as L
from diffusynth_amd.batching import SamplingBatcher
from diffusynth_amd.sampler import DiffSynthSampler
from diffusynth_amd.synth import synth_input

pytestmark = pytest.mark.gpu

H = 32


@pytest.fixture(scope="module")
def unet(unet_sd):
    from diffusynth_amd.unet import ConditionedUnet, PRODUCTION_CONFIG
    m = ConditionedUnet(**PRODUCTION_CONFIG)
    m.load_state_dict(unet_sd)
    return m.to("cuda")


# ------------------------------------------------------------------------------------------------ kernel
def _ddim_step(x, eps, eps_c, scale, noise, coef, blend=None):
    """ds_ddim_step on one row (the kernel of the standalone sampler)."""
    out = torch.empty_like(x)
    p = L.StepParams(x=x.data_ptr(), eps=eps.data_ptr(), eps_cond=eps_c.data_ptr() if eps_c is not None else None, noise=noise.data_ptr(),
                     out=out.data_ptr(), coef=coef.data_ptr(), cfg_scale=scale, blend_mode=0, guide=None, init_noise=None, mask=None,
                     qcoef=None, B=1, CHW=x.numel(), HW=x.shape[-2] * x.shape[-1])
    if blend is not None:
        mode, guide, init, mask, q = blend
        p.blend_mode, p.guide, p.mask, p.mask_chw = mode, guide.data_ptr(), mask.data_ptr(), 0 if mask.shape[1] == 1 else 1
        if mode == 1:
            p.init_noise, p.qcoef = init.data_ptr(), q.data_ptr()
    L.call("ds_ddim_step", ctypes.byref(p), L.current_stream())
    return out


def _gather(src, cols):
    idx = torch.tensor(cols, dtype=torch.int32, device="cuda")
    out = torch.empty(src.shape[:-1] + (len(cols),), device="cuda")
    L.call("ds_gather_cols", src.data_ptr(), src.numel() // src.shape[-1], src.shape[-1], idx.data_ptr(), len(cols), out.data_ptr(),
           L.current_stream())
    return out


@pytest.mark.parametrize("W,strategy", [(20, "repeat"), (27, "repeat"), (64, "repeat"), (100, "repeat"), (144, "repeat"),
                                        (27, "non-repeat"), (64, "non-repeat")])
def test_step_rows_equals_ddim_step_row_by_row(W, strategy):
    S = L.SR
    Cc, MB = 4, 3
    g = torch.Generator(device="cuda").manual_seed(W)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)                              # noqa: E731
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=MB, noise_strategy=strategy)
    s.respace(list(np.linspace(0, 999, 10, dtype=np.int32)))
    draw_w, cols = s._step_noise_layout(W)
    x, eps = rnd(4, Cc, H, W), rnd(7, Cc, H, W)
    guide, init = rnd(MB, Cc, H, W), rnd(MB, Cc, H, W)
    mask1 = (torch.rand(MB, 1, H, W, device="cuda", generator=g) > 0.5).float()
    maskc = (torch.rand(MB, Cc, H, W, device="cuda", generator=g) > 0.5).float()
    draw = rnd(MB, Cc, H, draw_w)
    seed, offset = 1234 + W, 77
    q = torch.tensor([[0.8, 0.6]], device="cuda")
    # rows: (x row, eps row, cond eps row, cfg scale, eta, t, blend mode, mask, noise mode, sample index, dup row)
    rows = [(0, 0, -1, 1.0, 0.0, 9, 0, None, 0, 0, -1),
            (1, 1, 2, 3.0, 1.0, 5, 1, mask1, 1, 1, -1),
            (2, 3, 4, 6.0, 1.0, 2, 2, maskc, 2, 2, 5),
            (3, 5, 6, 1.5, 1.0, 0, 1, maskc, 2, 0, 6),
            (3, 6, -1, 1.0, 0.0, 7, 2, mask1, 1, 2, -1)]
    R = len(rows)
    irow = torch.zeros(R, S["DS_SR_NI"], dtype=torch.int32)
    frow = torch.zeros(R, S["DS_SR_NF"], dtype=torch.float32)
    prow = torch.zeros(R, S["DS_SR_NP"], dtype=torch.int64)
    want = {}
    for r, (xr, er, ecr, scale, eta, t, mode, mask, nmode, b, dup) in enumerate(rows):
        coef = s._step_coefficients(torch.tensor([t]), eta)
        irow[r, S["DS_SR_X"]], irow[r, S["DS_SR_EPS"]], irow[r, S["DS_SR_EPSC"]] = xr, er, ecr
        irow[r, S["DS_SR_OUT"]], irow[r, S["DS_SR_DUP"]] = r, dup
        irow[r, S["DS_SR_BLEND"]], irow[r, S["DS_SR_NOISE"]] = mode, nmode
        irow[r, S["DS_SR_SAMPLE"]], irow[r, S["DS_SR_DRAW_ROWS"]], irow[r, S["DS_SR_DRAW_W"]] = b, MB, draw_w
        frow[r, :5], frow[r, S["DS_SR_CFG"]] = coef[0], scale
        frow[r, S["DS_SR_Q0"]], frow[r, S["DS_SR_Q1"]] = q[0, 0].item(), q[0, 1].item()
        blend = None
        if mode:
            m = mask[b:b + 1]
            irow[r, S["DS_SR_MASK_CHW"]] = 0 if m.shape[1] == 1 else 1
            prow[r, S["DS_SR_GUIDE"]], prow[r, S["DS_SR_INIT"]], prow[r, S["DS_SR_MASKP"]] = \
                guide[b:b + 1].data_ptr(), init[b:b + 1].data_ptr(), m.data_ptr()
            blend = (mode, guide[b:b + 1], init[b:b + 1], m, q)
        if nmode == 1:
            prow[r, S["DS_SR_DRAW"]] = draw.data_ptr()
            noise = _gather(draw[b:b + 1].contiguous(), cols)
        elif nmode == 2:
            prow[r, S["DS_SR_SEED"]], prow[r, S["DS_SR_OFFSET"]] = seed, offset
            full = torch.empty(MB, Cc, H, draw_w, device="cuda")
            L.call("ds_philox_normal", full.data_ptr(), full.numel(), seed, offset, L.current_stream())
            noise = _gather(full[b:b + 1].contiguous(), cols)
        else:
            noise = torch.zeros(1, Cc, H, W, device="cuda")
        want[r] = _ddim_step(x[xr:xr + 1], eps[er:er + 1], eps[ecr:ecr + 1] if ecr >= 0 else None, scale, noise, coef.cuda(), blend)
        if dup >= 0:
            want[dup] = want[r]
    colt = torch.tensor(cols, dtype=torch.int32, device="cuda")
    out = torch.full((7, Cc, H, W), float("nan"), device="cuda")
    it, ft, pt = irow.cuda(), frow.cuda(), prow.cuda()
    p = L.StepRowsParams(x=x.data_ptr(), eps=eps.data_ptr(), out=out.data_ptr(), irow=it.data_ptr(), frow=ft.data_ptr(), prow=pt.data_ptr(),
                         cols=colt.data_ptr(), R=R, C=Cc, H=H, W=W, Bx=x.shape[0], Beps=eps.shape[0], Bout=out.shape[0], n_cols=len(cols))
    L.call("ds_step_rows", ctypes.byref(p), L.current_stream())
    for r, w in want.items():
        assert torch.equal(out[r:r + 1], w), r


# ------------------------------------------------------------------------------------------------ end to end
def _dss(K, B, noise_device, cfg=1.0, uncond=None):
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=max(B, 2), noise_device=noise_device)
    s.respace(list(np.linspace(0, 999, K, dtype=np.int32)))
    if cfg != 1.0:
        s.activate_classifier_free_guidance(cfg, uncond)
    return s


def _mix(noise_device):
    """(tick of submission, sampler factory, method, args, kwargs) of the mixed workload: CFG-6 DDPM text, CFG-1 DDIM text, a
    null-condition request, sound2sound at strength 0.6, an arranger note, interpolate, and two late requests; widths 27 and 64."""
    cond = lambda tag, B: synth_input("bt_" + tag, (B, 512)).cuda()                          # noqa: E731
    un = synth_input("bt_uncond", (512,)).cuda()
    guide1 = synth_input("bt_guide1", (1, 4, H, 64)).cuda()
    guide2 = synth_input("bt_guide2", (1, 4, H, 64)).cuda()
    nd = noise_device
    return [
        (0, lambda: _dss(3, 2, nd, 6.0, un), "sample", ((2, 4, H, 27),), dict(return_tensor=True, condition=cond("a", 2), sampler="ddpm", seed=1)),
        (0, lambda: _dss(5, 1, nd), "sample", ((1, 4, H, 27),), dict(return_tensor=True, condition=cond("b", 1), sampler="ddim", seed=2)),
        (0, lambda: _dss(3, 1, nd), "sample", ((1, 4, H, 27),), dict(return_tensor=True, condition=None, sampler="ddim", seed=3)),
        (0, lambda: _dss(8, 1, nd), "img_guided_sample", ((1, 4, H, 64), 0.6, guide1),
         dict(return_tensor=True, condition=cond("d", 1), sampler="ddpm", seed=4)),
        (0, lambda: _dss(8, 1, nd), "inpaint_sample", ((1, 4, H, 27), 0.7, guide2, None),
         dict(return_tensor=True, condition=cond("e", 1), sampler="ddpm", use_dynamic_mask=True, end_noise_level_ratio=0.0,
              mask_flexivity=1.0, seed=5)),
        (0, lambda: _dss(3, 3, nd), "interpolate", ((3, 4, H, 64), 1.0), dict(return_tensor=True, condition=cond("f", 3), sampler="ddim", seed=6)),
        (2, lambda: _dss(5, 1, nd, 6.0, un), "sample", ((1, 4, H, 64),), dict(return_tensor=True, condition=cond("g", 1), sampler="ddpm", seed=7)),
        (3, lambda: _dss(3, 1, nd), "sample", ((1, 4, H, 27),), dict(return_tensor=True, condition=cond("h", 1), sampler="ddpm", seed=8)),
    ]


def _run_batched(unet, mix, max_rows=128):
    b = SamplingBatcher(unet, max_rows=max_rows)
    samplers, handles = [None] * len(mix), [None] * len(mix)
    tick = 0
    while any(h is None for h in handles) or b.active():
        for i, (at, mk, method, args, kw) in enumerate(mix):
            if handles[i] is None and at <= tick:
                samplers[i] = mk()
                handles[i] = b.submit(samplers[i], method, *args, **kw)
        b.step()
        tick += 1
    return b, samplers, [h.result() for h in handles]


def _run_alone(unet, mix):
    samplers, outs = [], []
    for at, mk, method, args, kw in mix:
        s = mk()
        outs.append(getattr(s, method)(unet, *args, **kw))
        samplers.append(s)
    return samplers, outs


@pytest.mark.parametrize("noise_device", ["cpu", "philox", None])
def test_concurrent_calls_equal_standalone_calls_fp32(unet, noise_device):
    unet.set_compute_dtype("fp32")
    mix = _mix(noise_device)
    b, sb, got = _run_batched(unet, mix)
    sa, want = _run_alone(unet, mix)
    for i, ((gi, gn), (wi, wn)) in enumerate(zip(got, want)):
        assert torch.equal(gn, wn), i
        assert len(gi) == len(wi), i
        for k, (x, y) in enumerate(zip(gi, wi)):
            assert torch.equal(x, y), (i, k)
        assert sb[i]._philox_offset == sa[i]._philox_offset and sb[i]._philox_seed == sa[i]._philox_seed, i
        assert sb[i]._generator is None
    assert len(unet._engine.plans) <= 8
    print(f"[batching] noise_device={noise_device}: {b.ticks} ticks, {b.plan_builds} plan builds, "
          f"host {1e3 * b.host_seconds / max(b.ticks, 1):.2f} ms per tick")


@pytest.mark.parametrize("tier", ["fp32", "bf16x3", "bf16"])
def test_single_request_is_the_standalone_call_in_every_tier(unet, tier):
    un = synth_input("bt_uncond", (512,)).cuda()
    c = synth_input("bt_single", (2, 512)).cuda()
    unet.set_compute_dtype(tier)
    try:
        args, kw = ((2, 4, H, 40),), dict(return_tensor=True, condition=c, sampler="ddpm", seed=9)
        b = SamplingBatcher(unet)
        h = b.submit(_dss(4, 2, "cpu", 6.0, un), "sample", *args, **kw)
        b.run()
        got, _ = h.result()
        want, _ = _dss(4, 2, "cpu", 6.0, un).sample(unet, *args, **kw)
        for x, y in zip(got, want):
            assert torch.equal(x, y)
    finally:
        unet.set_compute_dtype("fp32")


def test_mixed_batch_bf16x3_meets_the_tier_contract(unet):
    mix = _mix("cpu")
    unet.set_compute_dtype("fp32")
    _, ref = _run_alone(unet, mix)
    unet.set_compute_dtype("bf16x3")
    try:
        _, _, got = _run_batched(unet, mix)
        _, alone = _run_alone(unet, mix)
    finally:
        unet.set_compute_dtype("fp32")
    for i, ((g, _), (r, _), (a, _)) in enumerate(zip(got, ref, alone)):
        assert rel_err(g[-1].cpu(), r[-1].cpu()) < 1e-3, i
        mx, rms = rel_errs(g[-1].cpu(), a[-1].cpu())
        print(f"[batching] request {i}: bf16x3 batched vs bf16x3 alone: max-norm rel {mx:.2e}, rms rel {rms:.2e}")


def test_plan_churn_stays_bounded_and_exact(unet):
    """Requests come and go over many ticks at a small row budget (many distinct U-Net batches): no plan is built twice — the
    plans built are at most the distinct U-Net batches the ticks ran — and every result is still the standalone call's."""
    unet.set_compute_dtype("fp32")
    unet(synth_input("bt_arena", (8, 4, H, 64)).cuda(), torch.full((8,), 500, device="cuda"), synth_input("bt_arena_c", (8, 512)).cuda())
    mix = _mix("philox")                # (the arena now holds the largest plan below: no growth, which would drop the cached plans)
    b, _, got = _run_batched(unet, mix, max_rows=4)
    _, want = _run_alone(unet, mix)
    assert 0 < b.plan_builds <= len(b.unet_batches), (b.plan_builds, sorted(b.unet_batches))
    for (gi, _), (wi, _) in zip(got, want):
        assert torch.equal(gi[-1], wi[-1])
    print(f"[batching] max_rows=4: {b.ticks} ticks, {b.plan_builds} plan builds, {len(b.unet_batches)} distinct U-Net batches")


WIDTHS = (144, 128, 112, 100, 88, 76, 64, 52, 40, 27)     # more widths than the engine keeps plans (DS_MAX_PLANS = 8)


def test_more_buckets_than_plans_build_each_plan_once(unet):
    """Ten widths at once: admission keeps at most max_buckets (the engine's plan count) buckets live, so the round robin of a tick
    never evicts a plan it needs again — each width's plan is built once (widths in descending order: the first plan sizes the
    arena) — and every result is the call alone."""
    unet.set_compute_dtype("fp32")
    c = synth_input("bt_widths", (len(WIDTHS), 512)).cuda()
    mix = [(0, lambda: _dss(3, 1, "philox"), "sample", ((1, 4, H, w),), dict(return_tensor=True, condition=c[i:i + 1], sampler="ddpm", seed=40 + i))
           for i, w in enumerate(WIDTHS)]
    b, _, got = _run_batched(unet, mix)
    assert b.max_buckets == 8
    assert b.plan_builds <= len(WIDTHS), b.plan_builds
    _, want = _run_alone(unet, mix)
    for (gi, _), (wi, _) in zip(got, want):
        assert torch.equal(gi[-1], wi[-1])


def test_mixed_widths_serving_builds_one_plan_per_width(unet):
    """sample_mixed_widths over ten widths runs one width group after another: one plan per width, not one per width and step."""
    from diffusynth_amd.serving import sample_mixed_widths
    unet.set_compute_dtype("fp32")
    reqs = [{"width": w, "condition": synth_input("bt_mw%d" % i, (512,)), "seed": 60 + i} for i, w in enumerate(sorted(WIDTHS) * 2)]
    unet(synth_input("bt_mw_x", (1, 4, H, 20)).cuda(), torch.full((1,), 10, device="cuda"), None)     # (engine exists)
    before = unet._engine.plan_builds
    got = sample_mixed_widths(unet, reqs, 4, height=H, noise_device="cpu")
    assert unet._engine.plan_builds - before <= len(WIDTHS)
    assert [g.shape[-1] for g in got] == [r["width"] for r in reqs]


@pytest.mark.parametrize("noise_device", ["philox", "cpu", None])
def test_seeded_submit_leaves_the_global_generators_alone(unet, noise_device):
    un = synth_input("bt_uncond", (512,)).cuda()
    torch.manual_seed(123)
    cpu0, gpu0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    b = SamplingBatcher(unet)
    h = b.submit(_dss(3, 1, noise_device, 6.0, un), "sample", (1, 4, H, 27), return_tensor=True,
                 condition=synth_input("bt_rng", (1, 512)).cuda(), sampler="ddpm", seed=5)
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), gpu0)
    h.result()
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), gpu0)


def test_instrument_family_labels_fp32_exact():
    """Label conditions (nn.Embedding, condition_type="instrument_family"): CFG requests repeat the unconditional label, and a mixed
    bucket concatenates label vectors — still the calls alone, bit for bit."""
    from diffusynth_amd.unet import ConditionedUnet, PRODUCTION_CONFIG
    torch.manual_seed(0)
    net = ConditionedUnet(**dict(PRODUCTION_CONFIG, condition_type="instrument_family")).cuda()
    un = torch.tensor(11, device="cuda")
    lab = lambda *v: torch.tensor(v, device="cuda")                                           # noqa: E731
    mix = [(0, lambda: _dss(3, 2, "cpu", 3.0, un), "sample", ((2, 4, H, 27),), dict(return_tensor=True, condition=lab(3, 7), sampler="ddpm", seed=1)),
           (0, lambda: _dss(4, 1, "cpu"), "sample", ((1, 4, H, 27),), dict(return_tensor=True, condition=lab(5), sampler="ddim", seed=2)),
           (1, lambda: _dss(3, 1, "philox", 3.0, un), "sample", ((1, 4, H, 27),), dict(return_tensor=True, condition=lab(0), sampler="ddpm", seed=3)),
           (0, lambda: _dss(3, 2, "cpu", 3.0, un), "sample", ((2, 4, H, 64),), dict(return_tensor=True, condition=lab(1, 2), sampler="ddim", seed=4))]
    _, _, got = _run_batched(net, mix)
    _, want = _run_alone(net, mix)
    for i, ((gi, _), (wi, _)) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(gi, wi)):
            assert torch.equal(x, y), (i, k)


def test_malformed_row_reads_nothing_and_writes_nan():
    S = L.SR
    Cc, W = 4, 27
    x = torch.randn(2, Cc, H, W, device="cuda")
    eps = torch.randn(2, Cc, H, W, device="cuda")
    coef = DiffSynthSampler(1000, mute=True, device="cuda", height=H)._step_coefficients(torch.tensor([500]), 0.0)
    irow = torch.zeros(2, S["DS_SR_NI"], dtype=torch.int32)
    frow = torch.zeros(2, S["DS_SR_NF"], dtype=torch.float32)
    frow[:, :5] = coef[0]
    irow[:, S["DS_SR_EPSC"]] = -1
    irow[0, S["DS_SR_DUP"]] = -1
    irow[1, S["DS_SR_X"]], irow[1, S["DS_SR_EPS"]], irow[1, S["DS_SR_OUT"]], irow[1, S["DS_SR_DUP"]] = 1, 9, 1, 2   # eps row 9 of 2
    prow = torch.zeros(2, S["DS_SR_NP"], dtype=torch.int64)
    out = torch.zeros(3, Cc, H, W, device="cuda")
    it, ft, pt = irow.cuda(), frow.cuda(), prow.cuda()
    p = L.StepRowsParams(x=x.data_ptr(), eps=eps.data_ptr(), out=out.data_ptr(), irow=it.data_ptr(), frow=ft.data_ptr(), prow=pt.data_ptr(),
                         cols=None, R=2, C=Cc, H=H, W=W, Bx=2, Beps=2, Bout=3, n_cols=0)
    L.call("ds_step_rows", ctypes.byref(p), L.current_stream())
    assert torch.isfinite(out[0]).all()
    assert torch.isnan(out[1]).all() and torch.isnan(out[2]).all()
