"""Weighted multi-prompt guidance on the GPU: ds_cfg_compose against the restatement (tests/compose_ref.py), its bit identities (the
plain combine, constant envelopes, half-and-half, column selection, a row alone / in a batch / shifted / in ds_cfg_compose_rows), the
edge rows, ds_copy_rows, and the plumbing through the sampler, the batcher and the serving entry point, bit for bit against the same
arithmetic done by hand around a sampler that has no guidance.

The kernel's bounds are test_hip_guidance.py's: 2e-6 of the restatement for the output, 1e-6 for the gain.  Behind the fp32 combine,
which the restatement reproduces, the kernel's arithmetic is the same float64 two-pass.  An fp32 two-pass twin needs 1.8e-7 / 1.4e-7 on
this data (test_compose_cpu.py): 10.9 and 7.3 times inside the bounds.  Measured on the MI355X: 1.07e-7 at worst for the output,
6.5e-8 for the gain."""
import ctypes

import numpy as np
import pytest
import torch

import compose_ref as R
from conftest import rel_err
from diffusynth_amd import _lib as L
from diffusynth_amd.batching import SamplingBatcher
from diffusynth_amd.sampler import DiffSynthSampler
from diffusynth_amd.synth import synth_input

pytestmark = pytest.mark.gpu

ROWS = ((4, 8, 5), (4, 16, 27), (4, 128, 64))     # fewer pieces than threads and an odd width; the scalar form; 16-byte form, 8 pieces per thread
NAN = float("nan")
SENTINEL = 0x7FC12345               # a NaN with a payload: any write to a row shows


def _buf(rows, chw, shift=0):
    """[rows][chw] fp32 on the device whose address is 16-byte aligned (shift 0) or one float past it (the scalar path)."""
    t = torch.empty(rows * chw + 4, device="cuda")[shift:shift + rows * chw].view(rows, chw)
    assert t.data_ptr() % 16 == 4 * shift
    return t


def _put(a, shift=0):
    """A numpy [..][chw] array on the device, at the given shift."""
    t = _buf(int(np.prod(a.shape[:-1])), a.shape[-1], shift)
    t.copy_(torch.from_numpy(a).reshape(t.shape))
    return t.view(a.shape)


def _wt(wt):
    return wt.contiguous() if isinstance(wt, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(wt, dtype=np.float32)).cuda()


def _compose(u, c, wt, W, s, phi, out=None):
    """ds_cfg_compose on u [B][chw], c [K][B][chw] (one contiguous block) and wt (K,) / (K, W): (out, gain)."""
    wt = _wt(wt)
    out = torch.empty_like(u) if out is None else out
    gain = torch.full((u.shape[0],), NAN, device="cuda")
    assert c.is_contiguous() and c.shape[1:] == u.shape
    p = L.CfgComposeParams(eps_u=u.data_ptr(), eps_c=c.data_ptr(), wt=wt.data_ptr(), out=out.data_ptr(), gain=gain.data_ptr(), cfg_scale=s,
                           phi=phi, B=u.shape[0], K=c.shape[0], CHW=u.shape[1], W=W, wt_w=1 if wt.dim() == 1 else wt.shape[1])
    L.call("ds_cfg_compose", ctypes.byref(p), L.current_stream())
    return out, gain


def _compose_rows(eps, W, irow, frow, wt, gain=True):
    it, ft = torch.tensor(irow, dtype=torch.int32).cuda(), torch.tensor(frow, dtype=torch.float32).cuda()
    wt = torch.tensor(wt, dtype=torch.float32).cuda()
    g = torch.full((len(irow),), 7.0, device="cuda") if gain else None
    p = L.CfgComposeRowsParams(eps=eps.data_ptr(), irow=it.data_ptr(), frow=ft.data_ptr(), wt=wt.data_ptr(), gain=g.data_ptr() if gain else None,
                               R=len(irow), CHW=eps.shape[1], W=W, Beps=eps.shape[0], n_wt=wt.numel())
    L.call("ds_cfg_compose_rows", ctypes.byref(p), L.current_stream())
    torch.cuda.synchronize()
    return g


def _rescale(u, c, s, phi):
    out = torch.empty_like(u)
    p = L.CfgRescaleParams(eps_u=u.data_ptr(), eps_c=c.data_ptr(), out=out.data_ptr(), gain=None, cfg_scale=s, phi=phi, B=u.shape[0], CHW=u.shape[1])
    L.call("ds_cfg_rescale", ctypes.byref(p), L.current_stream())
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("off", [0.0, 100.0])
@pytest.mark.parametrize("row", ROWS)
def test_kernel_against_float64(row, off):
    (C, H, W), worst = row, [0.0, 0.0]
    chw = C * H * W
    for K in (1, 2, 3, 8):
        for B in (1, 3):
            u_np, c_np = R.case_inputs(B, chw, off, K)
            for wt in (R.case_weights(K), R.case_weights(K, W)):
                assert K == 1 or (wt < 0).any()
                refs = {(s, phi): R.compose(u_np, c_np, wt, W, s, phi, np.float32) for s, phi in ((6.0, 0.7), (20.0, 1.0), (0.5, 0.0))}
                for shift in (0, 1):
                    u, c = _put(u_np, shift), _put(c_np, shift)
                    for (s, phi), (ref, gref) in refs.items():
                        for inplace in (False, True):
                            uu = _put(u_np, shift) if inplace else u
                            out, gain = _compose(uu, c, wt, W, s, phi, out=uu if inplace else _buf(B, chw, shift))
                            assert out.data_ptr() % 16 == 4 * shift
                            err = rel_err(out.cpu(), torch.from_numpy(ref))
                            gerr = float(np.abs(gain.cpu().numpy().astype(np.float64) / gref - 1.0).max())
                            worst[0], worst[1] = max(worst[0], err), max(worst[1], gerr)
                            print(f"[compose] {row} off={off} K={K} B={B} wt{wt.shape} shift={shift} s={s} phi={phi} inplace={inplace}: "
                                  f"rel_err {err:.2e}, gain {gerr:.2e}")
                            assert err < 2e-6 and gerr < 1e-6, (K, B, wt.shape, shift, s, phi, inplace, err, gerr)
                    assert torch.equal(u, torch.from_numpy(u_np).cuda()) and torch.equal(c, torch.from_numpy(c_np).cuda())      # inputs unchanged
    print(f"[compose] {row} off={off}: worst rel_err {worst[0]:.2e}, gain {worst[1]:.2e}")


@pytest.mark.parametrize("row", ROWS)
def test_bit_identities(row):
    C, H, W = row
    chw = C * H * W
    u_np, c_np = R.case_inputs(3, chw, 100.0, 2, seed=1)
    u, c = _put(u_np), _put(c_np)
    one = torch.ones(1, device="cuda")
    for s in (0.5, 6.0):
        # K = 1, a = 1, phi = 0: the step kernels' combine (ds_cfg_rescale at phi = 0), and numpy's
        k1 = [_compose(u, c[k:k + 1], one, W, s, 0.0) for k in range(2)]
        for k in range(2):
            assert _same_bits(k1[k][0], _rescale(u, c[k], s, 0.0)) and (k1[k][1] == 1.0).all()
            assert np.array_equal(k1[k][0].cpu().numpy().view(np.int32), R.mix(u_np, c_np[k:k + 1], np.ones(1), W, s, np.float32)[1].view(np.int32))
        for phi in (0.0, 0.7):
            # a (K, W) table filled with constants is the (K,) form
            wt = R.case_weights(2)
            a, ga = _compose(u, c, wt, W, s, phi)
            b, gb = _compose(u, c, np.repeat(wt[:, None], W, axis=1), W, s, phi)
            assert torch.isfinite(a).all() and _same_bits(a, b) and _same_bits(ga, gb)
            # 0.5 / 0.5 of one condition is K = 1
            a, ga = _compose(u, c[:1], one, W, s, phi)
            b, gb = _compose(u, torch.cat([c[:1], c[:1]]), [0.5, 0.5], W, s, phi)
            assert _same_bits(a, b) and _same_bits(ga, gb) and (phi == 0.0 or not _same_bits(a, k1[0][0]))
        # an envelope 1 | 0 against its complement selects whole columns of the two K = 1 results
        env = np.zeros((2, W), np.float32)
        env[0, :W // 2] = 1.0
        env[1, W // 2:] = 1.0
        got, _ = _compose(u, c, env, W, s, 0.0)
        left = (torch.arange(W, device="cuda") < W // 2).view(1, 1, W)
        want = torch.where(left, k1[0][0].view(3, C * H, W), k1[1][0].view(3, C * H, W))
        assert _same_bits(got.view(3, C * H, W), want) and not _same_bits(got, k1[0][0]) and not _same_bits(got, k1[1][0])


@pytest.mark.parametrize("row", ROWS)
def test_a_row_is_the_same_bits_alone_in_a_batch_and_at_any_address(row):
    C, H, W = row
    chw = C * H * W
    u_np, c_np = R.case_inputs(3, chw, 100.0, 3, seed=1)
    for wt in (R.case_weights(3), R.case_weights(3, W)):
        whole, gw = _compose(_put(u_np), _put(c_np), wt, W, 6.0, 0.7)
        assert torch.isfinite(whole).all() and not torch.equal(whole[0], whole[1])
        for i in range(3):
            alone, ga = _compose(_put(u_np[i:i + 1]), _put(c_np[:, i:i + 1]), wt, W, 6.0, 0.7)
            assert _same_bits(alone[0], whole[i]) and torch.equal(ga[0], gw[i]), i
            moved, gm = _compose(_put(u_np[i:i + 1], 1), _put(c_np[:, i:i + 1], 1), wt, W, 6.0, 0.7, out=_buf(1, chw, 1))
            assert _same_bits(moved[0], whole[i]) and torch.equal(gm[0], gw[i]), i


@pytest.mark.parametrize("row", ROWS)
def test_rows_form_is_the_call_form(row):
    """Five requests' rows permuted inside a buffer of 20, two of them written in place, three to rows of their own, with differing K,
    strides, weights, scales and phi; the rows the table does not name keep the sentinel and the conditional rows their contents."""
    C, H, W = row
    chw = C * H * W
    eps = _buf(20, chw)
    _bits(eps).fill_(SENTINEL)
    # (u row, out row, K, row of c_1, row distance, envelope, scale, phi)
    reqs = [(9, 9, 1, 2, 5, False, 6.0, 0.7), (0, 5, 2, 11, 1, True, 20.0, 1.0), (4, 4, 3, 18, -2, False, 0.5, 0.3),
            (13, 19, 2, 7, 3, True, 6.0, 0.0), (6, 15, 2, 1, 2, False, 3.0, 1.0)]
    wts, wt_off, flat = [], [], [0.25, -0.5]                # (two floats in front: the offsets are not all multiples of anything)
    for n, (ur, orow, K, c0, cs, envl, s, phi) in enumerate(reqs):
        u_np, c_np = R.case_inputs(1, chw, 100.0, K, seed=10 + n)
        eps[ur].copy_(torch.from_numpy(u_np[0]))
        for k in range(K):
            eps[c0 + k * cs].copy_(torch.from_numpy(c_np[k, 0]))
        wts.append(R.case_weights(K, W if envl else None, seed=n))
        wt_off.append(len(flat))
        flat += wts[-1].ravel().tolist()
    before = eps.clone()
    want, want_g = {}, []
    for n, (ur, orow, K, c0, cs, envl, s, phi) in enumerate(reqs):
        c = torch.stack([before[c0 + k * cs] for k in range(K)]).view(K, 1, chw)
        o, g = _compose(before[ur:ur + 1].clone(), c, wts[n], W, s, phi)
        want[orow] = o
        want_g.append(g.item())
    order = [3, 0, 4, 2, 1]
    irow = [[reqs[n][0], reqs[n][1], reqs[n][2], reqs[n][3], reqs[n][4], wt_off[n], W if reqs[n][5] else 1] for n in order]
    frow = [list(reqs[n][6:]) for n in order]
    gain = _compose_rows(eps, W, irow, frow, flat)
    assert gain.cpu().tolist() == [want_g[n] for n in order]
    for r in range(20):
        if r in want:
            assert torch.isfinite(want[r]).all() and _same_bits(eps[r], want[r][0]), r
        else:
            assert _same_bits(eps[r], before[r]), r
    assert all((_bits(eps[r]) == SENTINEL).all() for r in (8, 17))         # the rows nobody names
    eps2 = before.clone()                                                    # without a gain array
    _compose_rows(eps2, W, irow, frow, flat, gain=False)
    assert _same_bits(eps2, eps)


def test_edge_rows():
    C, H, W = 4, 16, 27
    chw = C * H * W
    u_np, c_np = R.case_inputs(2, chw, 0.0, 2, seed=3)
    u_np[1] = 0.0
    c_np[:, 1] = 0.0
    out, gain = _compose(_put(u_np), _put(c_np), [0.6, 0.4], W, 6.0, 0.7)
    assert torch.isfinite(out).all() and (out[1] == 0).all() and gain[1].item() == 1.0 and 0.0 < gain[0].item() < 1.0
    # rows 0 .. 2 of the buffer: u, c_1, c_2; every table row writes a row of its own from 3 on (the last one names a row outside)
    eps = _buf(16, chw)
    eps.copy_(torch.from_numpy(np.concatenate([u_np[:1], c_np[:, 0]] + [u_np[:1]] * 13)))
    before = eps.clone()
    wt = [0.6, 0.4] + [1.0] * 27
    ok = [0, 3, 2, 1, 1, 0, 1]
    bad = {"u row": {0: 16}, "u row < 0": {0: -1}, "c_1 row": {3: 16}, "c_K row": {4: 15}, "c_K row < 0": {4: -2}, "K = 0": {2: 0}, "K = 9": {2: 9},
           "weights past n_wt": {5: 28}, "envelope past n_wt": {2: 2, 5: 2, 6: W}, "weights < 0": {5: -1}, "WTW": {6: 2}}
    irow, frow = [ok], [[6.0, 0.7]]
    for n, change in enumerate(bad.values()):
        irow.append([change.get(i, 4 + n if i == 1 else v) for i, v in enumerate(ok)])
        frow.append([6.0, 0.7])
    irow += [[0, 4 + len(bad), 2, 1, 1, 0, 1], [0, 16, 2, 1, 1, 0, 1]]           # a phi outside [0, 1]; an output row outside the buffer
    frow += [[6.0, 1.5], [6.0, 0.7]]
    assert 4 + len(bad) == 15
    gain = _compose_rows(eps, W, irow, frow, wt)
    good, gg = _compose(before[0:1].clone(), before[1:3].clone().view(2, 1, chw), [0.6, 0.4], W, 6.0, 0.7)
    assert _same_bits(eps[3], good[0]) and gain[0].item() == gg.item()
    for n, kind in enumerate(list(bad) + ["phi"]):
        assert torch.isnan(eps[4 + n]).all() and torch.isnan(gain[1 + n]), kind
    assert torch.isnan(gain[-1])
    assert torch.equal(eps[:3], before[:3])                                  # the neighbours: untouched


def test_copy_rows():
    chw = 4 * 16 * 27
    for shift in (0, 1):
        buf = _buf(10, chw, shift)
        _bits(buf).fill_(SENTINEL)
        src = torch.from_numpy(R.case_inputs(3, chw, 0.0, 1, seed=5)[0]).cuda()
        buf[1], buf[4], buf[7] = src[0], src[1], src[2]
        before = buf.clone()
        pairs = torch.tensor([[1, 0], [4, 9], [1, 2], [7, 7], [10, 3], [4, 10], [-1, 5], [7, -1]], dtype=torch.int32).cuda()
        L.call("ds_copy_rows", buf.data_ptr(), pairs.data_ptr(), len(pairs), chw, 10, L.current_stream())
        for r in range(10):
            want = {0: src[0], 9: src[1], 2: src[0]}.get(r, before[r])
            assert _same_bits(buf[r], want), (shift, r)
        assert all((_bits(buf[r]) == SENTINEL).all() for r in (3, 5, 6, 8))


# ------------------------------------------------------------------------------------------------ sampler
H5, K5, CFG = 16, 5, 6.0


class _Stub:
    """A cheap model whose eps depends on x, t and the condition, in elementwise IEEE operations only (a row's result does not depend on
    the batch it is in)."""

    def __init__(self):
        self.k = torch.linspace(0.2, 0.9, 1000, device="cuda")
        self.rows = []

    def __call__(self, x, t, c):
        self.rows.append(x.shape[0])
        k = self.k[t].view(-1, 1, 1, 1)
        return k * x + c[:, 0].view(-1, 1, 1, 1) + (0.05 * c[:, 1]).view(-1, 1, 1, 1) * (x * x)


class _ByHand:
    """What a sampler with a condition mix computes per step, as a model (taking the (B, K, D) condition) for a sampler without guidance."""

    def __init__(self, model, uncond, wt, scale, phi):
        self.model, self.uncond, self.wt, self.scale, self.phi = model, uncond, _wt(wt), scale, phi

    def __call__(self, x, t, c):
        un = self.uncond.unsqueeze(0).repeat(x.shape[0], 1)
        eu = self.model(x, t, un).contiguous()
        ec = torch.stack([self.model(x, t, c[:, k]) for k in range(c.shape[1])]).contiguous()
        return _compose(eu.flatten(1), ec.flatten(2), self.wt, x.shape[3], self.scale, self.phi)[0].view_as(x)


def _dss5(B, W, cfg=None, uncond=None, phi=0.0, mix=None):
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H5, max_batchsize=B, train_width=W, noise_device="cpu")
    s.respace(list(np.linspace(0, 999, K5, dtype=np.int32)))
    if cfg is not None:
        s.activate_classifier_free_guidance(cfg, uncond, guidance_rescale=phi)
    if mix is not None:
        s.set_condition_mix(mix)
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


def _weights(W, envelope):
    """K = 3, mixed signs; the envelope moves from the first prompt to the second along the note."""
    if not envelope:
        return np.array([0.8, -0.35, 0.5], np.float32)
    ramp = np.linspace(0.0, 1.0, W, dtype=np.float32)
    return np.stack([1.0 - ramp, ramp, np.full(W, -0.25, np.float32)])


@pytest.mark.parametrize("shape", [(2, 4, H5, 20), (1, 4, H5, 27)])
@pytest.mark.parametrize("method", ["sample", "img_guided", "inpaint_static", "inpaint_dynamic"])
@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "dpmpp_2m"])
def test_sampler_composes_at_every_step(sampler, method, shape):
    B, W = shape[0], shape[3]
    model = _Stub()
    cond = synth_input("cm_cond", (B, 3, 8)).cuda()
    un = synth_input("gd_uncond", (8,)).cuda()
    plain = _call(_dss5(B, W, CFG, un), model, method, shape, cond[:, 0].contiguous(), sampler)
    for envelope in (False, True):
        for phi in (0.0, 0.7):
            wt = _weights(W, envelope)
            got = _call(_dss5(B, W, CFG, un, phi, wt), model, method, shape, cond, sampler)
            want = _call(_dss5(B, W), _ByHand(model, un, wt, CFG, phi), method, shape, cond, sampler)
            assert all(torch.isfinite(x).all() for x in want[0])
            assert _same(got, want), (envelope, phi)
            assert torch.equal(got[1], plain[1]) and not torch.equal(plain[0][-1], got[0][-1])        # the mix moves the trajectory
    # set_condition_mix(None) restores the plain bits
    s = _dss5(B, W, CFG, un, 0.0, _weights(W, True))
    s.set_condition_mix(None)
    assert _same(_call(s, model, method, shape, cond[:, 0].contiguous(), sampler), plain)


def test_single_steps_interpolate_and_cfg_one_take_the_mix():
    model = _Stub()
    un = synth_input("gd_uncond", (8,)).cuda()
    cond = synth_input("cm_cond", (2, 3, 8)).cuda()
    x = synth_input("gd_state", (2, 4, H5, 20)).cuda()
    t = torch.tensor([3, 1], device="cuda")
    wt = _weights(20, True)
    for sampler in ("ddim", "dpmpp_2m"):
        got = _dss5(2, 20, CFG, un, 0.7, wt).p_sample(model, x, t, condition=cond, sampler=sampler)
        want = _dss5(2, 20).p_sample(_ByHand(model, un, wt, CFG, 0.7), x, t, condition=cond, sampler=sampler)
        assert torch.isfinite(want).all() and torch.equal(got, want), sampler
    kw = dict(return_tensor=True, condition=synth_input("cm_cond3", (3, 3, 8)).cuda(), sampler="ddim", seed=5)
    got = _dss5(3, 20, CFG, un, 0.7, wt).interpolate(model, (3, 4, H5, 20), 1.0, **kw)
    assert _same(got, _dss5(3, 20).interpolate(_ByHand(model, un, wt, CFG, 0.7), (3, 4, H5, 20), 1.0, **kw))
    # CFG == 1 with a mix: S = 1, and the model is called once per step on (1 + K) B rows
    model.rows = []
    got = _dss5(2, 20, 1.0, un, 0.7, wt).sample(model, (2, 4, H5, 20), return_tensor=True, condition=cond, seed=2)
    assert model.rows == [(1 + 3) * 2] * K5
    want = _dss5(2, 20).sample(_ByHand(model, un, wt, 1.0, 0.7), (2, 4, H5, 20), return_tensor=True, condition=cond, seed=2)
    assert _same(got, want)


# ------------------------------------------------------------------------------------------------ batcher and serving, on the U-Net
H = 32


@pytest.fixture(scope="module")
def unet(unet_sd):
    from diffusynth_amd.unet import ConditionedUnet, PRODUCTION_CONFIG
    m = ConditionedUnet(**PRODUCTION_CONFIG)
    m.load_state_dict(unet_sd)
    return m.to("cuda")


def _dss(B, noise_device, cfg=1.0, uncond=None, phi=0.0, mix=None):
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=max(B, 2), noise_device=noise_device)
    s.respace(list(np.linspace(0, 999, K5, dtype=np.int32)))
    if cfg != 1.0 or mix is not None:
        s.activate_classifier_free_guidance(cfg, uncond, guidance_rescale=phi)
    if mix is not None:
        s.set_condition_mix(mix)
    return s


@pytest.mark.parametrize("W", [20, 27])
def test_half_and_half_of_one_prompt_is_plain_cfg_on_the_unet(unet, W):
    unet.set_compute_dtype("fp32")
    un = synth_input("gd_un512", (512,)).cuda()
    c = synth_input("gd_a", (2, 512)).cuda()
    kw = dict(return_tensor=True, sampler="ddim", seed=1)
    want = _dss(2, "cpu", 6.0, un).sample(unet, (2, 4, H, W), condition=c, **kw)
    got = _dss(2, "cpu", 6.0, un, 0.0, [0.5, 0.5]).sample(unet, (2, 4, H, W), condition=torch.stack([c, c], dim=1), **kw)
    assert all(torch.isfinite(x).all() for x in want[0]) and _same(got, want)


def _mix(W, with_mix=True):
    """One bucket: a K = 2 mix (CFG 6, phi 0.7, ddim, B = 2), a K = 3 envelope mix (CFG 3, dpmpp_2m, inpaint with dynamic masks), a plain
    CFG request with rescale (ddim) and a no-CFG ddpm request.  with_mix=False: the same requests with the mixes dropped (each mix
    request guided by its first prompt alone)."""
    cond = lambda tag, *s: synth_input("gd_" + tag, s).cuda()                                  # noqa: E731
    un = synth_input("gd_un512", (512,)).cuda()
    guide = synth_input("gd_guide64", (1, 4, H, 64)).cuda()
    ramp = np.linspace(0.0, 1.0, W, dtype=np.float32)
    m2, m3 = np.array([0.6, 0.4], np.float32), np.stack([1.0 - ramp, ramp, np.full(W, -0.3, np.float32)])
    ca, cd = cond("cm_a", 2, 2, 512), cond("cm_d", 1, 3, 512)
    if not with_mix:
        m2 = m3 = None
        ca, cd = ca[:, 0].contiguous(), cd[:, 0].contiguous()
    return [
        (lambda: _dss(2, "cpu", 6.0, un, 0.7, m2), "sample", ((2, 4, H, W),), dict(return_tensor=True, condition=ca, sampler="ddim", seed=1)),
        (lambda: _dss(1, "philox", 3.0, un, 0.0, m3), "inpaint_sample", ((1, 4, H, W), 0.7, guide, None),
         dict(return_tensor=True, condition=cd, sampler="dpmpp_2m", use_dynamic_mask=True, end_noise_level_ratio=0.0, mask_flexivity=1.0, seed=4)),
        (lambda: _dss(1, "cpu", 6.0, un, 0.3), "sample", ((1, 4, H, W),), dict(return_tensor=True, condition=cond("b", 1, 512), sampler="ddim", seed=2)),
        (lambda: _dss(1, "philox"), "sample", ((1, 4, H, W),), dict(return_tensor=True, condition=cond("c", 1, 512), sampler="ddpm", seed=3)),
    ]


def _run_batched(unet, mix, max_rows):
    b = SamplingBatcher(unet, max_rows=max_rows)
    handles = [b.submit(mk(), method, *args, **kw) for mk, method, args, kw in mix]
    b.run()
    return b, [h.result() for h in handles]


@pytest.mark.parametrize("W", [20, 27])
@pytest.mark.parametrize("tier", ["fp32", "bf16x3"])
def test_batched_mix_requests_equal_the_calls_alone(unet, tier, W):
    """In the fp32 tier, and in bf16x3 on a model pinned at the batcher's max_rows, every h.result() is the call alone, whatever shares
    the bucket."""
    max_rows = 16
    unet.set_compute_dtype(tier).pin_launch_batch(None if tier == "fp32" else max_rows)
    try:
        b, got = _run_batched(unet, _mix(W), max_rows)
        # 2 x (1 + 2) + 1 x (1 + 3) + 2 + 1 U-Net rows, then (the inpaint call has 3 of the 5 steps) without the K = 3 request's 4; a
        # bucket with a K >= 2 request is never paired
        assert b.unet_batches == {(13, H, W, True, False), (9, H, W, True, False)}
        for i, (mk, method, args, kw) in enumerate(_mix(W)):
            want, want_noise = getattr(mk(), method)(unet, *args, **kw)
            assert torch.equal(got[i][1], want_noise), i
            assert len(got[i][0]) == len(want) > 1, i
            for k, (x, y) in enumerate(zip(got[i][0], want)):
                assert torch.isfinite(y).all() and torch.equal(x, y), (i, k)
        # dropping the mixes changes the mix requests' results, and nothing of their bucket mates'
        b0, got0 = _run_batched(unet, _mix(W, with_mix=False), max_rows)
        assert {k[0] for k in b0.unet_batches} == {9, 7}                    # 2 x 2 + 2 + 2 + 1, then without the inpaint call's 2
        moved = [not torch.equal(a[0][-1], c[0][-1]) for a, c in zip(got, got0)]
        assert moved == [True, True, False, False]
        assert all(torch.equal(x, y) for i in (2, 3) for x, y in zip(got[i][0], got0[i][0]))
    finally:
        unet.set_compute_dtype("fp32").pin_launch_batch(None)


def test_mixed_widths_serving_takes_mix_requests(unet):
    from diffusynth_amd.serving import sample_mixed_widths
    unet.set_compute_dtype("fp32")
    un = synth_input("gd_un512", (512,)).cuda()
    ramp = np.linspace(0.0, 1.0, 27, dtype=np.float32)
    reqs = [{"width": 20, "conditions": synth_input("cm_mw0", (2, 512)), "weights": [0.6, 0.4], "seed": 40},
            {"width": 27, "conditions": synth_input("cm_mw1", (3, 512)), "weights": np.stack([1.0 - ramp, ramp, np.full(27, -0.3, np.float32)]), "seed": 41},
            {"width": 20, "condition": synth_input("gd_mw2", (512,)), "seed": 42}]
    got = sample_mixed_widths(unet, reqs, K5, height=H, cfg_scale=6, unconditional_condition=un, noise_device="cpu", guidance_rescale=0.7)
    for r, g in zip(reqs, got):
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=1, noise_device="cpu")
        s.respace(list(np.linspace(0, 999, K5, dtype=np.int32)))
        s.activate_classifier_free_guidance(6, un, guidance_rescale=0.7)
        if "weights" in r:
            s.set_condition_mix(r["weights"])
        c = (r["conditions"] if "weights" in r else r["condition"]).cuda().float()[None]
        want, _ = s.sample(unet, (1, 4, H, r["width"]), return_tensor=True, condition=c, seed=r["seed"])
        assert len(want) == K5 + 1 and torch.isfinite(want[-1]).all()
        assert torch.equal(g, want[-1][0]), r["width"]
    with pytest.raises(ValueError, match="both"):
        sample_mixed_widths(unet, [dict(reqs[0], condition=reqs[2]["condition"])], K5, height=H, cfg_scale=6, unconditional_condition=un)
    with pytest.raises(ValueError, match="weights"):
        sample_mixed_widths(unet, [dict(reqs[1], width=20)], K5, height=H, cfg_scale=6, unconditional_condition=un)
