"""Guidance rescale without a GPU: the identities of the float64 restatement (tests/guidance_ref.py), why the kernel test's bound
tells a variance about the mean from a single-pass one, the sampler's argument checks and the batcher's prologue with phi set."""
import ctypes

import numpy as np
import pytest
import torch

import guidance_ref as G
from diffusynth_amd import _lib as L
from diffusynth_amd.batching import request_program
from diffusynth_amd.sampler import DiffSynthSampler

CASES = [(B, chw, off) for B in (1, 3) for chw in (160, 1728, 32768) for off in (0.0, 100.0)]


def test_restatement_identities():
    for B, chw, off in CASES:
        u, c = G.case_inputs(B, chw, off)
        for s in (0.5, 6.0, 20.0):
            e = G.combine(u, c, s)
            out, g = G.rescale(u, c, s, 0.0)
            assert np.array_equal(out, e) and np.array_equal(g, np.ones(B))                    # phi = 0: the plain combine
            out, g = G.rescale(u, c, s, 1.0)
            assert np.abs(G.row_std(out) / G.row_std(c) - 1.0).max() < 1e-12                   # phi = 1: the conditional eps's std
            _, g7 = G.rescale(u, c, s, 0.7)
            _, gk = G.rescale(3.5 * u.astype(np.float64), 3.5 * c.astype(np.float64), s, 0.7)
            assert np.abs(gk / g7 - 1.0).max() < 1e-12                                         # a common scaling leaves g alone
            assert ((g7 < 1.0) == (s > 1.0)).all()          # guidance beyond 1 widens e, and the rescale narrows it again
    z = np.zeros((2, 160))
    out, g = G.rescale(z, z, 6.0, 0.7)
    assert np.array_equal(g, np.ones(2)) and np.array_equal(out, z)                            # std(e) == 0: ratio 1, no NaN


def _rel_err(a, b):
    d = np.abs(a.astype(np.float64) - b)
    return max(d.max() / np.abs(b).max(), np.linalg.norm(d) / np.linalg.norm(b))


def test_the_kernel_bound_separates_two_pass_from_single_pass():
    """test_hip_guidance.py holds the kernel to 2e-6 of the float64 restatement.  On its data an fp32 twin that takes the variance about
    the mean (pairwise sums) is an order of magnitude inside that bound, and one that takes E[x^2] - mean^2 in fp32 is outside it wherever
    the mean is 100 standard deviations from zero."""
    def pairwise(a):
        a = a.astype(np.float32)
        while a.shape[1] > 1:
            if a.shape[1] % 2:
                a = np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], axis=1)
            a = a[:, 0::2] + a[:, 1::2]
        return a[:, 0]

    def twin(u, c, s, phi, two_pass):
        e = G.combine(u, c, s, np.float32)
        n = np.float32(e.shape[1])
        var = []
        for a in (c, e):
            m = pairwise(a) / n
            if two_pass:
                d = a - m[:, None]
                var.append(pairwise(d * d) / (n - 1))
            else:
                var.append((pairwise(a * a) / n - m * m) * (n / (n - 1)))
        with np.errstate(invalid="ignore", divide="ignore"):
            g = np.float32(phi) * np.sqrt(var[0] / var[1]) + np.float32(1.0 - phi)
        return g.astype(np.float32)[:, None] * e

    worst_two, best_single = 0.0, np.inf
    for B, chw, off in CASES:
        u, c = G.case_inputs(B, chw, off)
        for s in (0.5, 6.0, 20.0):
            for phi in (0.7, 1.0):
                ref, _ = G.rescale(u, c, s, phi, np.float32)
                worst_two = max(worst_two, _rel_err(twin(u, c, s, phi, True), ref))
                if off == 100.0:
                    err = _rel_err(twin(u, c, s, phi, False), ref)
                    best_single = min(best_single, err if np.isfinite(err) else np.inf)
    print(f"fp32 two-pass twin: worst {worst_two:.2e}; fp32 single-pass twin at off = 100: best {best_single:.2e}")
    assert worst_two < 2e-6 / 5 and best_single > 2e-6 * 5


def _sampler(**kw):
    return DiffSynthSampler(1000, device="cpu", mute=True, height=16, max_batchsize=2, noise_device="cpu", **kw)


def test_sampler_keeps_phi_and_rejects_what_is_outside_the_unit_interval():
    s = _sampler()
    un = torch.zeros(8)
    assert s.guidance_rescale == 0.0
    s.activate_classifier_free_guidance(6.0, un)                       # the reference's two positionals, unchanged
    assert s.CFG == 6.0 and s.unconditional_condition is un and s.guidance_rescale == 0.0
    s.activate_classifier_free_guidance(6.0, un, 0.7)
    assert s.guidance_rescale == 0.7
    s.activate_classifier_free_guidance(6.0, un, guidance_rescale=1)
    assert s.guidance_rescale == 1.0 and isinstance(s.guidance_rescale, float)
    for bad in (-0.1, 1.0001, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            s.activate_classifier_free_guidance(6.0, un, bad)
        assert s.guidance_rescale == 1.0 and s.CFG == 6.0              # a rejected call changes nothing
    s.activate_classifier_free_guidance(1.0, None, 0.5)                # no guidance: kept, not applied
    assert s.CFG == 1.0 and s.guidance_rescale == 0.5
    with pytest.raises(AssertionError, match="unconditional_condition must be available"):
        s.activate_classifier_free_guidance(3.0, None, 0.5)


def test_loop_program_prologue_with_phi_set():
    s = _sampler()
    s.respace(list(np.linspace(0, 999, 5, dtype=np.int32)))
    s.activate_classifier_free_guidance(6.0, torch.zeros(8), 0.7)
    s._generator = torch.Generator()
    prog, args = request_program(s, "sample", (2, 4, 16, 20), condition=torch.zeros(2, 8), sampler="dpmpp_2m", seed=3)
    assert prog.steps == [4, 3, 2, 1, 0] and prog.img.shape == (2, 4, 16, 20) and args["sampler"] == "dpmpp_2m"
    plain = _sampler()
    plain.respace(list(np.linspace(0, 999, 5, dtype=np.int32)))
    plain._generator = torch.Generator()
    want, _ = request_program(plain, "sample", (2, 4, 16, 20), condition=torch.zeros(2, 8), sampler="dpmpp_2m", seed=3)
    assert torch.equal(prog.img, want.img) and torch.equal(prog.coef_cpu, want.coef_cpu)       # phi touches no part of the program


def test_entry_points_validate_before_device_work():
    lib = L.load()
    fake = 1 << 20
    ok = dict(eps_u=fake, eps_c=fake, out=fake, gain=None, cfg_scale=6.0, phi=0.7, B=2, CHW=160)
    for bad in (dict(eps_u=None), dict(eps_c=None), dict(out=None), dict(B=0), dict(CHW=0), dict(phi=-0.5), dict(phi=1.5), dict(phi=float("nan"))):
        p = L.CfgRescaleParams(**dict(ok, **bad))
        assert lib.ds_cfg_rescale(ctypes.byref(p), None) == -1, bad
        assert b"cfg_rescale" in lib.ds_last_error_string()
    ok = dict(eps=fake, irow=fake, frow=fake, gain=None, R=2, CHW=160, Beps=4)
    for bad in (dict(eps=None), dict(irow=None), dict(frow=None), dict(R=0), dict(CHW=-1), dict(Beps=0)):
        p = L.CfgRescaleRowsParams(**dict(ok, **bad))
        assert lib.ds_cfg_rescale_rows(ctypes.byref(p), None) == -1, bad
        assert b"cfg_rescale_rows" in lib.ds_last_error_string()
    with pytest.raises(L.DsError, match="cfg_rescale"):
        L.call("ds_cfg_rescale", ctypes.byref(L.CfgRescaleParams()), None)
