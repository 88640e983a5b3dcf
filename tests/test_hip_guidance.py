"""Guidance rescale on the GPU: ds_cfg_rescale against the float64 restatement (tests/guidance_ref.py), its bit guarantees (a row alone,
in a batch and in ds_cfg_rescale_rows), the edge rows, and the plumbing through the sampler, the batcher and the serving entry point,
bit for bit against the same arithmetic done by hand around a sampler that has no guidance.

The kernel's bound, 2e-6 of the float64 restatement (gain: 1e-6), is eleven times what an fp32 two-pass twin needs on this data
(1.8e-7) and twenty-five times below the least a single-pass fp32 variance loses at off = 100 (5.3e-5); test_guidance_cpu.py measures
both.  Measured on the MI355X: 1.0e-7 at worst for the output, 5.9e-8 for the gain, 1.9e-7 for the std at phi = 1."""
import ctypes

import numpy as np
import pytest
import torch

import guidance_ref as G
from conftest import rel_err
from diffusynth_amd import _lib as L
from diffusynth_amd.batching import SamplingBatcher
from diffusynth_amd.sampler import DiffSynthSampler
from diffusynth_amd.synth import synth_input

pytestmark = pytest.mark.gpu

CHWS = (160, 1728, 32768)           # 4 x 8 x 5 (fewer pieces than threads), 4 x 16 x 27 (odd width), 32 pieces per thread
SCALES = (0.5, 6.0, 20.0)
NAN = float("nan")


def _buf(rows, chw, shift=0):
    """[rows][chw] fp32 on the device whose address is 16-byte aligned (shift 0) or one float past it (the scalar path)."""
    t = torch.empty(rows * chw + 4, device="cuda")[shift:shift + rows * chw].view(rows, chw)
    assert t.data_ptr() % 16 == 4 * shift
    return t


def _put(a, shift=0):
    t = _buf(a.shape[0], a.shape[1], shift)
    t.copy_(torch.from_numpy(a))
    return t


def _rescale(u, c, s, phi, out=None):
    """ds_cfg_rescale on the rows of u / c: (out, gain)."""
    out = torch.empty_like(u) if out is None else out
    gain = torch.full((u.shape[0],), NAN, device="cuda")
    p = L.CfgRescaleParams(eps_u=u.data_ptr(), eps_c=c.data_ptr(), out=out.data_ptr(), gain=gain.data_ptr(), cfg_scale=s, phi=phi,
                           B=u.shape[0], CHW=u[0].numel())
    L.call("ds_cfg_rescale", ctypes.byref(p), L.current_stream())
    return out, gain


def _rescale_rows(eps, irow, frow, gain=True):
    it, ft = torch.tensor(irow, dtype=torch.int32).cuda(), torch.tensor(frow, dtype=torch.float32).cuda()
    g = torch.full((len(irow),), 7.0, device="cuda") if gain else None
    p = L.CfgRescaleRowsParams(eps=eps.data_ptr(), irow=it.data_ptr(), frow=ft.data_ptr(), gain=g.data_ptr() if gain else None,
                               R=len(irow), CHW=eps.shape[1], Beps=eps.shape[0])
    L.call("ds_cfg_rescale_rows", ctypes.byref(p), L.current_stream())
    torch.cuda.synchronize()
    return g


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("off", [0.0, 100.0])
@pytest.mark.parametrize("chw", CHWS)
def test_kernel_against_float64(chw, off):
    worst = [0.0, 0.0, 0.0]
    for B in (1, 3):
        u_np, c_np = G.case_inputs(B, chw, off)
        for shift in (0, 1):
            u, c = _put(u_np, shift), _put(c_np, shift)
            for s in SCALES:
                for phi in (0.7, 1.0):
                    ref, gref = G.rescale(u_np, c_np, s, phi, np.float32)
                    for inplace in (False, True):
                        uu = _put(u_np, shift) if inplace else u
                        out, gain = _rescale(uu, c, s, phi, out=uu if inplace else _buf(B, chw, shift))
                        assert out.data_ptr() % 16 == 4 * shift
                        err = rel_err(out.cpu(), torch.from_numpy(ref))
                        gerr = float(np.abs(gain.cpu().numpy().astype(np.float64) / gref - 1.0).max())
                        worst[0], worst[1] = max(worst[0], err), max(worst[1], gerr)
                        assert err < 2e-6 and gerr < 1e-6, (B, shift, s, phi, inplace, err, gerr)
                        if phi == 1.0:          # std of every output row, evaluated in float64, is the conditional eps's
                            serr = float(np.abs(G.row_std(out.cpu().numpy()) / G.row_std(c_np) - 1.0).max())
                            worst[2] = max(worst[2], serr)
                            assert serr < 1e-6, (B, shift, s, inplace, serr)
                    assert torch.equal(u, torch.from_numpy(u_np).cuda()) and torch.equal(c, torch.from_numpy(c_np).cuda())
    print(f"[guidance] CHW={chw} off={off}: worst rel_err {worst[0]:.2e}, gain {worst[1]:.2e}, std at phi = 1 {worst[2]:.2e}")


@pytest.mark.parametrize("chw", CHWS)
def test_a_row_is_the_same_bits_alone_in_a_batch_and_at_any_address(chw):
    u_np, c_np = G.case_inputs(3, chw, 100.0, seed=1)
    u, c = _put(u_np), _put(c_np)
    whole, gw = _rescale(u, c, 6.0, 0.7)
    assert torch.isfinite(whole).all() and not torch.equal(whole[0], whole[1])
    for i in range(3):
        alone, ga = _rescale(u[i:i + 1], c[i:i + 1], 6.0, 0.7)
        assert torch.equal(_bits(alone[0]), _bits(whole[i])) and torch.equal(ga[0], gw[i]), i
        moved, gm = _rescale(_put(u_np[i:i + 1], 1), _put(c_np[i:i + 1], 1), 6.0, 0.7, out=_buf(1, chw, 1))
        assert torch.equal(_bits(moved[0]), _bits(whole[i])) and torch.equal(gm[0], gw[i]), i


SENTINEL = 0x7FC12345               # a NaN with a payload: any write to a row shows


@pytest.mark.parametrize("chw", CHWS)
def test_rows_form_is_the_call_form(chw):
    """Five requests' rows permuted inside a buffer of 14, two of them written in place, three to rows of their own; the rows the table
    does not name keep the sentinel and the conditional rows their contents, byte for byte."""
    u_np, c_np = G.case_inputs(5, chw, 100.0, seed=2)
    eps = _buf(14, chw)
    _bits(eps).fill_(SENTINEL)
    # (u row, c row, out row, scale, phi)
    rows = [(9, 2, 9, 6.0, 0.7), (0, 11, 5, 20.0, 1.0), (4, 3, 4, 0.5, 0.3), (12, 7, 13, 6.0, 0.0), (6, 1, 10, 3.0, 1.0)]
    want, want_g = {}, []
    for k, (ur, cr, orow, s, phi) in enumerate(rows):
        eps[ur].copy_(torch.from_numpy(u_np[k]))
        eps[cr].copy_(torch.from_numpy(c_np[k]))
    before = eps.clone()
    for k, (ur, cr, orow, s, phi) in enumerate(rows):
        if phi == 0.0:              # the call form takes phi = 0 too (it is the combine): the rows form must agree with it and with numpy
            want[orow] = torch.from_numpy(G.combine(u_np[k:k + 1], c_np[k:k + 1], s, np.float32)).cuda()
            want_g.append(1.0)
            o, g = _rescale(before[ur:ur + 1], before[cr:cr + 1], s, phi)
            assert torch.equal(_bits(o), _bits(want[orow])) and g.item() == 1.0
        else:
            o, g = _rescale(before[ur:ur + 1], before[cr:cr + 1], s, phi)
            want[orow] = o
            want_g.append(g.item())
    order = [3, 0, 4, 2, 1]
    gain = _rescale_rows(eps, [list(rows[k][:3]) for k in order], [list(rows[k][3:]) for k in order])
    assert gain.cpu().tolist() == [want_g[k] for k in order]
    for r in range(14):
        if r in want:
            assert torch.isfinite(want[r]).all() and torch.equal(_bits(eps[r]), _bits(want[r][0])), r
        else:
            assert torch.equal(_bits(eps[r]), _bits(before[r])), r
    assert all((_bits(eps[r]) == SENTINEL).all() for r in (8,))            # the one row nobody names
    # without a gain array
    eps2 = before.clone()
    _rescale_rows(eps2, [list(rows[k][:3]) for k in order], [list(rows[k][3:]) for k in order], gain=False)
    assert torch.equal(_bits(eps2), _bits(eps))


def test_edge_rows():
    chw = 1728
    u_np, c_np = G.case_inputs(2, chw, 0.0, seed=3)
    u_np[1] = c_np[1] = 0.0
    out, gain = _rescale(_put(u_np), _put(c_np), 6.0, 0.7)
    assert torch.isfinite(out).all() and (out[1] == 0).all() and gain[1].item() == 1.0 and 0.0 < gain[0].item() < 1.0
    # malformed rows: 1 names an unconditional row outside the buffer, 2 a conditional one, 3 a phi outside [0, 1], 4 an output row outside
    eps = _buf(8, chw)
    eps.copy_(torch.from_numpy(np.concatenate([u_np[:1], c_np[:1]] * 4)))
    before = eps.clone()
    irow = [[0, 1, 0], [9, 1, 2], [0, -1, 3], [0, 1, 4], [0, 1, 8]]
    frow = [[6.0, 0.7], [6.0, 0.7], [6.0, 0.7], [6.0, 1.5], [6.0, 0.7]]
    gain = _rescale_rows(eps, irow, frow)
    good, gg = _rescale(before[0:1], before[1:2], 6.0, 0.7)
    assert torch.equal(eps[0], good[0]) and gain[0].item() == gg.item()
    assert torch.isnan(eps[2:5]).all() and torch.isnan(gain[1:]).all()
    assert torch.equal(eps[1], before[1]) and torch.equal(eps[5:], before[5:])


# ------------------------------------------------------------------------------------------------ sampler
H5, K5, CFG, PHI = 16, 5, 6.0, 0.7


class _Stub:
    """A cheap model whose eps depends on x, t and the condition, in elementwise IEEE operations only (a row's result does not depend on
    the batch it is in)."""

    def __init__(self):
        self.k = torch.linspace(0.2, 0.9, 1000, device="cuda")
        self.calls = 0

    def __call__(self, x, t, c):
        self.calls += 1
        k = self.k[t].view(-1, 1, 1, 1)
        return k * x + c[:, 0].view(-1, 1, 1, 1) + (0.05 * c[:, 1]).view(-1, 1, 1, 1) * (x * x)


class _ByHand:
    """What a sampler with guidance rescale computes per step, as a model for a sampler without guidance."""

    def __init__(self, model, uncond, scale, phi):
        self.model, self.uncond, self.scale, self.phi = model, uncond, scale, phi

    def __call__(self, x, t, c):
        un = self.uncond.unsqueeze(0).repeat(x.shape[0], 1)
        eu, ec = self.model(x, t, un).contiguous(), self.model(x, t, c).contiguous()
        return _rescale(eu.flatten(1), ec.flatten(1), self.scale, self.phi)[0].view_as(x)


def _dss5(B, W, **guidance):
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H5, max_batchsize=B, train_width=W, noise_device="cpu")
    s.respace(list(np.linspace(0, 999, K5, dtype=np.int32)))
    if guidance:
        s.activate_classifier_free_guidance(CFG, guidance.pop("uncond"), **guidance)
    return s


def _call(s, model, method, shape, cond, sampler):
    B, _, _, W = shape
    kw = dict(return_tensor=True, condition=cond, sampler=sampler, seed=13)
    guide = synth_input("gd_guide", (B, 4, H5, W)).cuda()
    if method == "sample":
        return s.sample(model, shape, **kw)
    if method == "img_guided":
        return s.img_guided_sample(model, shape, 0.6, guide, **kw)
    dyn = method == "inpaint_dynamic"
    mask = None if dyn else (synth_input("gd_mask", (B, 1, H5, W)) > 0).float().cuda()
    return s.inpaint_sample(model, shape, 0.7, guide, mask, use_dynamic_mask=dyn, mask_flexivity=1.0, **kw)


def _same(a, b):
    return len(a[0]) == len(b[0]) > 1 and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))


@pytest.mark.parametrize("shape", [(2, 4, H5, 20), (1, 4, H5, 27)])
@pytest.mark.parametrize("method", ["sample", "img_guided", "inpaint_static", "inpaint_dynamic"])
@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "dpmpp_2m"])
def test_sampler_applies_the_rescale_at_every_step(sampler, method, shape):
    B, W = shape[0], shape[3]
    model = _Stub()
    cond = synth_input("gd_cond", (B, 8)).cuda()
    un = synth_input("gd_uncond", (8,)).cuda()
    got = _call(_dss5(B, W, uncond=un, guidance_rescale=PHI), model, method, shape, cond, sampler)
    want = _call(_dss5(B, W), _ByHand(model, un, CFG, PHI), method, shape, cond, sampler)
    assert all(torch.isfinite(x).all() for x in want[0])
    assert _same(got, want)
    # phi = 0 given explicitly is the sampler that never got the keyword, and the rescale does move the trajectory
    plain = _call(_dss5(B, W, uncond=un), model, method, shape, cond, sampler)
    assert _same(_call(_dss5(B, W, uncond=un, guidance_rescale=0.0), model, method, shape, cond, sampler), plain)
    assert not torch.equal(plain[0][-1], got[0][-1])


def test_single_steps_and_interpolate_take_the_rescale():
    model = _Stub()
    un = synth_input("gd_uncond", (8,)).cuda()
    cond = synth_input("gd_cond", (2, 8)).cuda()
    x = synth_input("gd_state", (2, 4, H5, 20)).cuda()
    t = torch.tensor([3, 1], device="cuda")
    for sampler in ("ddim", "dpmpp_2m"):
        got = _dss5(2, 20, uncond=un, guidance_rescale=PHI).p_sample(model, x, t, condition=cond, sampler=sampler)
        want = _dss5(2, 20).p_sample(_ByHand(model, un, CFG, PHI), x, t, condition=cond, sampler=sampler)
        assert torch.isfinite(want).all() and torch.equal(got, want), sampler
    kw = dict(return_tensor=True, condition=synth_input("gd_cond3", (3, 8)).cuda(), sampler="ddim", seed=5)
    got = _dss5(3, 20, uncond=un, guidance_rescale=PHI).interpolate(model, (3, 4, H5, 20), 1.0, **kw)
    assert _same(got, _dss5(3, 20).interpolate(_ByHand(model, un, CFG, PHI), (3, 4, H5, 20), 1.0, **kw))
    # CFG == 1: phi is kept and not applied (one model call per step, the plain trajectory)
    s = _dss5(2, 20)
    s.activate_classifier_free_guidance(1.0, None, PHI)
    n0 = model.calls
    a = s.sample(model, (2, 4, H5, 20), return_tensor=True, condition=cond, seed=2)
    assert model.calls - n0 == K5 and s.guidance_rescale == PHI
    assert _same(a, _dss5(2, 20).sample(model, (2, 4, H5, 20), return_tensor=True, condition=cond, seed=2))


# ------------------------------------------------------------------------------------------------ batcher and serving, on the U-Net
H = 32


@pytest.fixture(scope="module")
def unet(unet_sd):
    from diffusynth_amd.unet import ConditionedUnet, PRODUCTION_CONFIG
    m = ConditionedUnet(**PRODUCTION_CONFIG)
    m.load_state_dict(unet_sd)
    return m.to("cuda")


def _dss(B, noise_device, cfg=1.0, uncond=None, phi=None):
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=max(B, 2), noise_device=noise_device)
    s.respace(list(np.linspace(0, 999, K5, dtype=np.int32)))
    if cfg != 1.0:
        if phi is None:
            s.activate_classifier_free_guidance(cfg, uncond)
        else:
            s.activate_classifier_free_guidance(cfg, uncond, guidance_rescale=phi)
    return s


def _mix(W, with_phi=True):
    """One bucket: CFG 6 / phi 0.7 / ddim, CFG 6 / phi 0 / dpmpp_2m, no CFG / ddpm, CFG 3 / phi 0.3 / inpaint with dynamic masks (on the
    solver, so that both step launches take rescaled rows).  with_phi=False: the same mix with every phi 0."""
    cond = lambda tag, B: synth_input("gd_" + tag, (B, 512)).cuda()                          # noqa: E731
    un = synth_input("gd_un512", (512,)).cuda()
    guide = synth_input("gd_guide64", (1, 4, H, 64)).cuda()
    f = (lambda v: v) if with_phi else (lambda v: 0.0)                                       # noqa: E731
    return [
        (lambda: _dss(2, "cpu", 6.0, un, f(0.7)), "sample", ((2, 4, H, W),), dict(return_tensor=True, condition=cond("a", 2), sampler="ddim", seed=1)),
        (lambda: _dss(1, "cpu", 6.0, un, f(0.0)), "sample", ((1, 4, H, W),), dict(return_tensor=True, condition=cond("b", 1), sampler="dpmpp_2m", seed=2)),
        (lambda: _dss(1, "philox"), "sample", ((1, 4, H, W),), dict(return_tensor=True, condition=cond("c", 1), sampler="ddpm", seed=3)),
        (lambda: _dss(1, "philox", 3.0, un, f(0.3)), "inpaint_sample", ((1, 4, H, W), 0.7, guide, None),
         dict(return_tensor=True, condition=cond("d", 1), sampler="dpmpp_2m", use_dynamic_mask=True, end_noise_level_ratio=0.0, mask_flexivity=1.0,
              seed=4)),
    ]


def _run_batched(unet, mix, max_rows):
    b = SamplingBatcher(unet, max_rows=max_rows)
    handles = [b.submit(mk(), method, *args, **kw) for mk, method, args, kw in mix]
    b.run()
    return b, [h.result() for h in handles]


@pytest.mark.parametrize("W", [20, 27])
@pytest.mark.parametrize("tier", ["fp32", "bf16x3"])
def test_batched_requests_with_phi_equal_the_calls_alone(unet, tier, W):
    """INTEGRATION.md §1 with phi: in the fp32 tier, and in bf16x3 on a model pinned at the batcher's max_rows, every h.result() is the
    call alone, whatever shares the bucket; the rescale changes no U-Net batch."""
    max_rows = 16
    unet.set_compute_dtype(tier).pin_launch_batch(None if tier == "fp32" else max_rows)
    try:
        b, got = _run_batched(unet, _mix(W), max_rows)
        b0, got0 = _run_batched(unet, _mix(W, with_phi=False), max_rows)
        assert b.unet_batches == b0.unet_batches and {k[0] for k in b.unet_batches} == {9, 7}      # 2 x 2 + 2 + 1 + 2 rows, then without the inpaint
        for i, (mk, method, args, kw) in enumerate(_mix(W)):
            want, want_noise = getattr(mk(), method)(unet, *args, **kw)
            assert torch.equal(got[i][1], want_noise), i
            assert len(got[i][0]) == len(want) > 1, i
            for k, (x, y) in enumerate(zip(got[i][0], want)):
                assert torch.isfinite(y).all() and torch.equal(x, y), (i, k)
        # phi does something to the requests that have it, and nothing to their bucket mates
        moved = [not torch.equal(a[0][-1], c[0][-1]) for a, c in zip(got, got0)]
        assert moved == [True, False, False, True]
    finally:
        unet.set_compute_dtype("fp32").pin_launch_batch(None)


def test_mixed_widths_serving_passes_phi_to_every_sampler(unet):
    from diffusynth_amd.serving import sample_mixed_widths
    unet.set_compute_dtype("fp32")
    un = synth_input("gd_un512", (512,)).cuda()
    reqs = [{"width": w, "condition": synth_input("gd_mw%d" % i, (512,)), "seed": 40 + i} for i, w in enumerate((20, 27, 20))]
    got = sample_mixed_widths(unet, reqs, K5, height=H, cfg_scale=6, unconditional_condition=un, noise_device="cpu", guidance_rescale=0.7)
    plain = sample_mixed_widths(unet, reqs, K5, height=H, cfg_scale=6, unconditional_condition=un, noise_device="cpu")
    for r, g, p in zip(reqs, got, plain):
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=1, noise_device="cpu")
        s.respace(list(np.linspace(0, 999, K5, dtype=np.int32)))
        s.activate_classifier_free_guidance(6, un, guidance_rescale=0.7)
        want, _ = s.sample(unet, (1, 4, H, r["width"]), return_tensor=True, condition=r["condition"].cuda().float()[None], seed=r["seed"])
        assert len(want) == K5 + 1 and torch.isfinite(want[-1]).all()
        assert torch.equal(g, want[-1][0]) and not torch.equal(g, p), r["width"]
    with pytest.raises(ValueError, match="guidance_rescale"):
        sample_mixed_widths(unet, reqs, K5, height=H, cfg_scale=6, unconditional_condition=un, guidance_rescale=1.5)
