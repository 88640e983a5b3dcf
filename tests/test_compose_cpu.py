"""Weighted multi-prompt guidance without a GPU: the identities of the restatement (tests/compose_ref.py), what an fp32 two-pass twin
of the statistics loses on the kernel test's data, and every host-side check of set_condition_mix, of a call with a mix and of
sample_mixed_widths, with CPU objects only."""
import ctypes

import numpy as np
import pytest
import torch

import compose_ref as R
import guidance_ref as G
from diffusynth_amd import _lib as L
from diffusynth_amd.batching import request_program
from diffusynth_amd.sampler import DiffSynthSampler

ROWS = ((4, 8, 5), (4, 16, 27), (4, 128, 64))           # test_hip_compose.py's rows
SCALES = (0.5, 6.0, 20.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_one_condition_at_weight_one_is_the_plain_combine():
    for (C, H, W) in ROWS:
        for off in (0.0, 100.0):
            u, c = R.case_inputs(3, C * H * W, off, 1)
            for s in SCALES:
                p, e = R.mix(u, c, np.ones(1, np.float32), W, s, np.float32)
                assert p.dtype == e.dtype == np.float32
                assert np.array_equal(_bits(e), _bits(G.combine(u, c[0], s, np.float32)))
                out, g = R.compose(u, c, np.ones(1, np.float32), W, s, 0.0, np.float32)
                assert np.array_equal(out, e.astype(np.float64)) and np.array_equal(g, np.ones(3))
                # p = u + (c - u) is not c bit for bit (at off = 100 it is: there c - u is exact): with phi > 0 the gain is
                # guidance_ref's up to that rounding
                assert np.array_equal(_bits(p), _bits(c[0])) == (off == 100.0)
                for phi in (0.7, 1.0):
                    out, g = R.compose(u, c, np.ones(1, np.float32), W, s, phi, np.float32)
                    want, gw = G.rescale(u, c[0], s, phi, np.float32)
                    assert np.abs(g / gw - 1.0).max() < 1e-6 and np.abs(out - want).max() / np.abs(want).max() < 1e-6


def test_half_and_half_of_one_condition_and_column_selection_are_exact():
    for (C, H, W) in ROWS:
        N = C * H * W
        u, c = R.case_inputs(2, N, 100.0, 2, seed=1)
        for s in SCALES:
            one = [R.mix(u, c[k:k + 1], np.ones(1, np.float32), W, s, np.float32)[1] for k in range(2)]
            twice = R.mix(u, np.stack([c[0], c[0]]), np.array([0.5, 0.5], np.float32), W, s, np.float32)[1]
            assert np.array_equal(_bits(twice), _bits(one[0]))
            # an envelope 1 | 0 against its complement: whole columns of the single-prompt results
            env = np.zeros((2, W), np.float32)
            env[0, :W // 2] = 1.0
            env[1, W // 2:] = 1.0
            e = R.mix(u, c, env, W, s, np.float32)[1].reshape(2, C * H, W)
            want = np.where(np.arange(W) < W // 2, one[0].reshape(2, C * H, W), one[1].reshape(2, C * H, W))
            assert np.array_equal(_bits(e), _bits(want))
        z = np.zeros((2, N), np.float32)
        out, g = R.compose(z, np.zeros((3, 2, N), np.float32), R.case_weights(3), W, 6.0, 0.7, np.float32)
        assert np.array_equal(g, np.ones(2)) and np.array_equal(out, z)          # std(e) == 0: ratio 1, no NaN


def _rel_err(a, b):
    d = np.abs(a.astype(np.float64) - b)
    return max(d.max() / np.abs(b).max(), np.linalg.norm(d) / np.linalg.norm(b))


def test_what_an_fp32_two_pass_twin_loses_on_the_kernel_tests_data():
    """test_hip_compose.py holds the kernel to test_hip_guidance.py's bounds: 2e-6 of the restatement for the output, 1e-6 for the gain.
    Behind the fp32 combine, which the restatement reproduces, the kernel's arithmetic is the same float64 two-pass; a twin that takes
    the two variances about the mean in fp32 (pairwise sums) must stay ten times inside the bound for it to be a comfortable one.
    Measured: worst 1.8e-7 for the output (10.9 times inside 2e-6) and 1.4e-7 for the gain (7.3 times inside 1e-6): the gain's
    margin is less than ten times, which is reported here and in DESIGN.md 7g; the bounds stay as they are (the kernel sums in
    float64, not in fp32, and this test holds the twin five times inside both, as test_guidance_cpu.py does)."""
    def pairwise(a):
        a = a.astype(np.float32)
        while a.shape[1] > 1:
            if a.shape[1] % 2:
                a = np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], axis=1)
            a = a[:, 0::2] + a[:, 1::2]
        return a[:, 0]

    worst, worst_g = 0.0, 0.0
    for (C, H, W) in ROWS:
        N = C * H * W
        n = np.float32(N)
        for off in (0.0, 100.0):
            for K in (1, 2, 3, 8):
                for B in (1, 3):
                    u, c = R.case_inputs(B, N, off, K)
                    for wt in (R.case_weights(K), R.case_weights(K, W)):
                        for s, phi in ((6.0, 0.7), (20.0, 1.0)):
                            ref, gref = R.compose(u, c, wt, W, s, phi, np.float32)
                            p, e = R.mix(u, c, wt, W, s, np.float32)
                            var = []
                            for a in (p, e):
                                d = a - (pairwise(a) / n)[:, None]
                                var.append(pairwise(d * d) / (n - 1))
                            g = (np.float32(phi) * np.sqrt(var[0] / var[1]) + np.float32(1.0 - phi)).astype(np.float32)
                            worst = max(worst, _rel_err(g[:, None] * e, ref))
                            worst_g = max(worst_g, float(np.abs(g.astype(np.float64) / gref - 1.0).max()))
    print(f"fp32 two-pass twin: worst output {worst:.2e} ({2e-6 / worst:.1f} times inside 2e-6), gain {worst_g:.2e} "
          f"({1e-6 / worst_g:.1f} times inside 1e-6)")
    assert worst < 2e-6 / 5 and worst_g < 1e-6 / 5


# ------------------------------------------------------------------------------------------------ host-side checks
def _sampler(**kw):
    s = DiffSynthSampler(1000, device="cpu", mute=True, height=16, max_batchsize=2, noise_device="cpu", **kw)
    s.respace(list(np.linspace(0, 999, 5, dtype=np.int32)))
    return s


def test_set_condition_mix_keeps_valid_weights_and_rejects_the_rest():
    s = _sampler()
    assert s._mix is None
    s.set_condition_mix([0.6, 0.4])
    assert s._mix.dtype == np.float32 and s._mix.shape == (2,)
    s.set_condition_mix(torch.ones(3, 20))
    assert s._mix.shape == (3, 20)
    s.set_condition_mix(np.array([[-1.5]]))
    assert s._mix.shape == (1, 1)
    for bad in ([], [[]], np.ones(9), np.ones((9, 20)), np.ones((2, 2, 2)), 0.5, [0.5, float("nan")], [float("inf")], np.ones((2, 257)),
                ["a", "b"]):
        with pytest.raises(ValueError, match="weights"):
            s.set_condition_mix(bad)
        assert s._mix.shape == (1, 1)                                       # a rejected call changes nothing
    s.set_condition_mix(None)
    assert s._mix is None
    with pytest.raises(ValueError, match="shard"):
        _sampler(shard=(0, 2)).set_condition_mix([1.0])


class _NeverCalled:
    def __call__(self, *a, **k):
        raise AssertionError("the model was called")


def test_a_call_with_a_mix_is_checked_before_any_device_work():
    model, shape = _NeverCalled(), (2, 4, 16, 20)
    cond = torch.zeros(2, 3, 8)
    s = _sampler()
    s.set_condition_mix([0.5, 0.3, -0.2])
    with pytest.raises(ValueError, match="unconditional_condition"):        # never activated
        s.sample(model, shape, condition=cond, seed=1)
    s.activate_classifier_free_guidance(1.0, None)
    with pytest.raises(ValueError, match="unconditional_condition"):        # activated without one (legal for CFG == 1 without a mix)
        s.sample(model, shape, condition=cond, seed=1)
    s.activate_classifier_free_guidance(1.0, torch.zeros(8))                # CFG == 1.0 is legal with a mix
    for bad in (None, torch.zeros(2, 8), torch.zeros(2, 2, 8), torch.zeros(3, 3, 8), torch.zeros(2, 3, 8, 1)):
        with pytest.raises(ValueError, match="condition"):
            s.sample(model, shape, condition=bad, seed=1)
        with pytest.raises(ValueError, match="condition"):
            s.p_sample(model, torch.zeros(shape), torch.tensor([3, 1]), condition=bad)
    guide, mask = torch.zeros(shape), torch.zeros(2, 1, 16, 20)
    s.set_condition_mix(np.ones((3, 27)))                                   # an envelope of another width than the call's
    for call in (lambda: s.sample(model, shape, condition=cond, seed=1),
                 lambda: s.interpolate(model, shape, 1.0, condition=cond, seed=1),
                 lambda: s.img_guided_sample(model, shape, 0.6, guide, condition=cond, seed=1),
                 lambda: s.inpaint_sample(model, shape, 0.7, guide, mask, condition=cond, seed=1),
                 lambda: s.p_sample(model, torch.zeros(shape), torch.tensor([3, 1]), condition=cond, sampler="dpmpp_2m")):
        with pytest.raises(ValueError, match="weights"):
            call()
    # a valid call's prologue is the plain sampler's: the mix touches no part of the program
    s.set_condition_mix(np.ones((3, 20)))
    s._generator = torch.Generator()
    prog, _ = request_program(s, "sample", shape, condition=cond, sampler="dpmpp_2m", seed=3)
    plain = _sampler()
    plain._generator = torch.Generator()
    want, _ = request_program(plain, "sample", shape, condition=torch.zeros(2, 8), sampler="dpmpp_2m", seed=3)
    assert prog.steps == [4, 3, 2, 1, 0] and torch.equal(prog.img, want.img) and torch.equal(prog.coef_cpu, want.coef_cpu)
    # a sharded sampler cannot have got a mix through set_condition_mix; one that has it anyhow is refused at the call
    sh = _sampler(shard=(0, 2))
    sh.activate_classifier_free_guidance(1.0, torch.zeros(8))
    sh._mix = np.ones(3, np.float32)
    with pytest.raises(ValueError, match="shard"):
        sh.sample(model, shape, condition=cond, seed=1)


def test_mixed_widths_serving_rejects_malformed_mix_requests():
    from diffusynth_amd.serving import sample_mixed_widths
    model, un = _NeverCalled(), torch.zeros(8)
    ok = {"width": 20, "conditions": torch.zeros(2, 8), "weights": [0.6, 0.4], "seed": 1}
    kw = dict(height=16, device="cpu", noise_device="cpu", unconditional_condition=un)
    with pytest.raises(ValueError, match="both"):                           # both forms
        sample_mixed_widths(model, [dict(ok, condition=torch.zeros(8))], 5, **kw)
    for bad in ([0.6], np.ones((2, 27)), np.ones((3, 20)), np.ones((2, 20, 1))):
        with pytest.raises(ValueError, match="weights"):                    # weights that match neither K nor the request's width
            sample_mixed_widths(model, [ok, dict(ok, weights=bad)], 5, **kw)
    with pytest.raises(ValueError, match="weights"):
        sample_mixed_widths(model, [dict(ok, weights=[0.5, float("nan")])], 5, **kw)
    with pytest.raises(ValueError, match="weights"):
        sample_mixed_widths(model, [{"width": 20, "conditions": torch.zeros(2, 8), "seed": 1}], 5, **kw)
    with pytest.raises(ValueError, match="unconditional_condition"):
        sample_mixed_widths(model, [ok], 5, **dict(kw, unconditional_condition=None))


def test_entry_points_validate_before_device_work():
    lib = L.load()
    fake = 1 << 20
    ok = dict(eps_u=fake, eps_c=fake, wt=fake, out=fake, gain=None, cfg_scale=6.0, phi=0.7, B=2, K=3, CHW=160, W=5, wt_w=5)
    assert L.CC["DS_CC_MAXK"] == 8 and L.CC["DS_CC_NI"] == 7 and L.CC["DS_CC_NF"] == 2
    for bad in (dict(eps_u=None), dict(eps_c=None), dict(wt=None), dict(out=None), dict(B=0), dict(CHW=0), dict(K=0), dict(K=9), dict(W=0),
                dict(W=7), dict(wt_w=2), dict(wt_w=0), dict(W=320, CHW=640, wt_w=320), dict(phi=-0.5), dict(phi=1.5), dict(phi=float("nan"))):
        p = L.CfgComposeParams(**dict(ok, **bad))
        assert lib.ds_cfg_compose(ctypes.byref(p), None) == -1, bad
        assert b"cfg_compose" in lib.ds_last_error_string()
    ok = dict(eps=fake, irow=fake, frow=fake, wt=fake, gain=None, R=2, CHW=160, W=5, Beps=4, n_wt=8)
    for bad in (dict(eps=None), dict(irow=None), dict(frow=None), dict(wt=None), dict(R=0), dict(CHW=-1), dict(W=0), dict(W=7), dict(Beps=0),
                dict(n_wt=0)):
        p = L.CfgComposeRowsParams(**dict(ok, **bad))
        assert lib.ds_cfg_compose_rows(ctypes.byref(p), None) == -1, bad
        assert b"cfg_compose_rows" in lib.ds_last_error_string()
    for args in ((None, fake, 1, 160, 4), (fake, None, 1, 160, 4), (fake, fake, 0, 160, 4), (fake, fake, 1, 0, 4), (fake, fake, 1, 160, 0),
                 (fake, fake, 65536, 160, 4)):
        assert lib.ds_copy_rows(*args, None) == -1, args
        assert b"copy_rows" in lib.ds_last_error_string()
