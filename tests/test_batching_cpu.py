"""SamplingBatcher without a GPU: argument checks of ds_step_rows, the per-request program the batcher derives (against the CPU
reference sampler) and the submit-time rejections."""
import ctypes

import numpy as np
import pytest
import torch

from diffusynth_amd import _lib as L
from diffusynth_amd.batching import SamplingBatcher, request_program
from diffusynth_amd.sampler import DiffSynthSampler
from oracle import sampler_ref as S
from oracle.sampler_ref import RefSampler

H, K = 16, 6


def test_step_rows_validates_before_device_work():
    lib = L.load()
    p = L.StepRowsParams()
    assert lib.ds_step_rows(ctypes.byref(p), None) == -1
    assert b"step_rows" in lib.ds_last_error_string()
    # every pointer set, inconsistent sizes / counts
    fake = 1 << 20
    ok = dict(x=fake, eps=fake, out=fake, irow=fake, frow=fake, prow=fake, cols=None, R=2, C=4, H=8, W=20, Bx=2, Beps=2, Bout=2, n_cols=0)
    for bad in (dict(R=0), dict(W=0), dict(Bx=0), dict(Beps=-1), dict(n_cols=-1), dict(n_cols=20), dict(R=70000)):
        p = L.StepRowsParams(**dict(ok, **bad))
        assert lib.ds_step_rows(ctypes.byref(p), None) == -1, bad
        assert b"step_rows" in lib.ds_last_error_string()
    for null in ("x", "eps", "out", "irow", "frow", "prow"):
        p = L.StepRowsParams(**dict(ok, **{null: None}))
        assert lib.ds_step_rows(ctypes.byref(p), None) == -1, null
    with pytest.raises(L.DsError, match="step_rows"):
        L.call("ds_step_rows", ctypes.byref(L.StepRowsParams()), None)


def _pair(B=2, cfg=1.0):
    dss = DiffSynthSampler(1000, device="cpu", mute=True, height=H, max_batchsize=B, noise_device="cpu")
    ref = RefSampler(1000, height=H, max_batchsize=B)
    ts = list(np.linspace(0, 999, K, dtype=np.int32))
    dss.respace(ts)
    ref.respace(ts)
    return dss, ref


def _ref_coef(ref, i, eta):
    t = torch.tensor([i])
    a_t = S._coef(ref.alphas_cumprod, t, 1)
    a_p = S._coef(ref.alphas_cumprod_prev, t, 1)
    sig = eta * torch.sqrt((1 - a_p) / (1 - a_t)) * torch.sqrt(1 - a_t / a_p)
    return torch.cat([torch.sqrt(1. - a_t), torch.sqrt(a_t), torch.sqrt(a_p), torch.sqrt(1 - a_p - sig ** 2), sig])


@pytest.mark.parametrize("case", ["sample", "img_guided", "inpaint_fixed", "inpaint_dynamic"])
def test_request_program_matches_reference_schedule(case):
    """The batcher's per-request program (steps, mapped timesteps, coefficient and q rows, blend modes, per-step masks, initial noise)
    is what the CPU reference computes; its draws come from the request's private generator, seeded like torch.manual_seed(seed)."""
    B, seed = 2, 11
    W = 64 if case == "img_guided" else 48          # (img_guided_sample takes a guide of the latent's own width = train_width)
    dss, ref = _pair(B)
    sampler = "ddpm" if case != "img_guided" else "ddim"
    eta = 1.0 if sampler == "ddpm" else 0.0
    guide = torch.randn(B, 4, H, dss.train_width, generator=torch.Generator().manual_seed(3))
    mask = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(4)) > 0.5).float()
    dss._generator = torch.Generator()
    before = torch.get_rng_state()
    if case == "sample":
        prog, _ = request_program(dss, "sample", (B, 4, H, W), condition=None, sampler=sampler, seed=seed)
        ref_call = dict(start_ratio=1.0)
    elif case == "img_guided":
        prog, _ = request_program(dss, "img_guided_sample", (B, 4, H, W), 0.6, guide, sampler=sampler, seed=seed)
        ref_call = dict(start_ratio=0.6, guide_img=guide)
    else:
        dyn = case == "inpaint_dynamic"
        prog, _ = request_program(dss, "inpaint_sample", (B, 4, H, W), 0.7, guide, None if dyn else mask, sampler=sampler, seed=seed,
                                  use_dynamic_mask=dyn, end_noise_level_ratio=0.0, mask_flexivity=1.0)
        ref_call = dict(start_ratio=0.7, guide_img=guide, mask=None if dyn else mask, use_dynamic_mask=dyn, mask_flexivity=1.0)
    assert torch.equal(torch.get_rng_state(), before)              # the global generator was not touched
    torch.manual_seed(seed)
    ref_init, _ = ref.noise(B, W)
    assert torch.equal(prog.initial_noise, ref_init)
    start = int(ref.num_timesteps * ref_call.get("start_ratio", 1.0))
    steps = list(reversed(range(0, start)))
    assert prog.steps == steps and len(steps) > 0
    assert [dss.timestep_map[i] for i in prog.steps] == [ref.timestep_map[i] for i in steps]
    for k, i in enumerate(steps):
        assert torch.equal(prog.coef_cpu[k], _ref_coef(ref, i, eta)), (k, i)
    if "guide_img" in ref_call:
        g, pts = ref.noise(B, W, reference_noise=guide)
        want = ref.q_sample(g, torch.full((B,), start - 1).long(), noise=ref_init)
        assert torch.equal(prog.img, want)
    else:
        assert torch.equal(prog.img, ref_init)
    if case.startswith("inpaint"):
        assert prog.inpaint and len(prog.blends) == len(steps)
        masks = (S.dynamic_masks(start, (B, 4, H, W), pts, dss.train_width, 1.0) if case == "inpaint_dynamic" else [mask] * start)
        cur = None
        for k, i in enumerate(steps):
            mode, m = prog.blends[k]
            if i > 0:
                cur = masks.pop()
                tq = torch.tensor([i - 1])
                assert mode == 1
                assert torch.equal(prog.q_cpu[k], torch.cat([S._coef(ref.sched["sqrt_alphas_cumprod"], tq, 1),
                                                             S._coef(ref.sched["sqrt_one_minus_alphas_cumprod"], tq, 1)]))
            else:
                assert mode == 2
            assert torch.equal(m, torch.as_tensor(cur).float().expand(B, 1, H, W)), (k, i)
        assert torch.equal(prog.guide, ref.noise(B, W, reference_noise=guide)[0])
    else:
        assert not prog.inpaint and prog.blends == []


class _Stub(torch.nn.Module):
    """Stands in for the U-Net at submit time (the batcher only reads its device before a tick)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_submit_rejections():
    b = SamplingBatcher(_Stub(), max_rows=4)
    dss, _ = _pair(2)
    with pytest.raises(ValueError):
        b.submit(dss, "ddim_sample", (2, 4, H, 32))
    with pytest.raises(NotImplementedError):
        b.submit(dss, "sample", (2, 4, H, 32), sampler="other", seed=1)
    assert dss._generator is None
    h = b.submit(dss, "sample", (2, 4, H, 32), sampler="ddim", seed=1)
    assert not h.done()
    with pytest.raises(RuntimeError, match="in flight"):
        b.submit(dss, "sample", (2, 4, H, 32), seed=2)                  # the same sampler object again
    sharded = DiffSynthSampler(1000, device="cpu", mute=True, height=H, max_batchsize=2, noise_device="cpu", shard=(0, 2))
    with pytest.raises(ValueError, match="shard"):
        b.submit(sharded, "sample", (1, 4, H, 32), seed=1)
    big, _ = _pair(4)
    big.activate_classifier_free_guidance(3.0, torch.zeros(8))
    with pytest.raises(ValueError, match="max_rows"):
        b.submit(big, "sample", (3, 4, H, 32), condition=torch.zeros(3, 8), seed=1)        # 6 U-Net rows > 4
    tall = DiffSynthSampler(1000, device="cpu", mute=True, height=2 * H, max_batchsize=2, noise_device="cpu")
    with pytest.raises(AssertionError, match=r"shape\[2\] != self.height"):
        b.submit(tall, "sample", (1, 4, 2 * H, 32), seed=1)
    wide_c = DiffSynthSampler(1000, device="cpu", mute=True, height=H, max_batchsize=2, channels=8, noise_device="cpu")
    with pytest.raises(AssertionError, match=r"shape\[1\] != self.channels"):
        b.submit(wide_c, "sample", (1, 8, H, 32), seed=1)
    other, _ = _pair(2)
    with pytest.raises(AssertionError, match=r"shape\[2\] != self.height"):
        b.submit(other, "sample", (1, 4, H + 1, 32), seed=1)            # the sampler's own assertion
    assert b.active() == 1


def test_seedless_request_draws_its_seed_from_the_global_generator():
    b = SamplingBatcher(_Stub(), max_rows=8)
    dss, _ = _pair(1)
    torch.manual_seed(5)
    b.submit(dss, "sample", (1, 4, H, 32))
    after_one = torch.get_rng_state()
    torch.manual_seed(5)
    torch.randint(0, 2 ** 62, (1,))
    assert torch.equal(after_one, torch.get_rng_state())                # exactly one draw of the global generator


def test_seeded_submit_leaves_the_global_generator_alone():
    """submit() runs the call's prologue on the request's private generator: a seeded call does not reseed torch's global one."""
    b = SamplingBatcher(_Stub(), max_rows=8)
    torch.manual_seed(77)
    before = torch.get_rng_state()
    dss, _ = _pair(1)
    b.submit(dss, "sample", (1, 4, H, 32), seed=3)
    assert torch.equal(torch.get_rng_state(), before)
    assert dss._generator is not None
