"""The Inpaint tab's latent mask on the device (csrc/inpaint_mask.hip, diffusynth_amd/inpaint_mask.py, serving.inpaint_with_text) against
scipy.ndimage.zoom called as webUI/natural_language_guided_4/inpaint_with_text.py:218 calls it, on the int64 mask.

The mask is compared EXACTLY, every pixel: tests/test_inpaint_mask_cpu.py asserts that on these fixtures scipy's float64 value is farther
than 1e-7 from every half-integer, and the device's float64 value is asserted within 1e-12 of scipy's here (rounding noise of the
restatement is 1e-15, FMA contraction may move it an order; 1e-12 is three orders above that and five below the closest half-distance), so
no rounding can flip."""
import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

import inpaint_mask_ref as R
from diffusynth_amd import _lib as L
from diffusynth_amd import inpaint_mask as M
from diffusynth_amd.sampler import DiffSynthSampler
from diffusynth_amd.synth import synth_input

pytestmark = pytest.mark.gpu

FIXTURES = R.fixtures()
IDS = [name for name, _ in FIXTURES]
PRE_TOL = 1e-12


def _shape(m):
    return (R.zoomed_size(m.shape[0]), R.zoomed_size(m.shape[1]))


def _run(whats, **kw):
    """(planes, pre) of a list of masks in one pass of the three kernels; latent shapes from the size rule."""
    shapes = [_shape(w if isinstance(w, (np.ndarray, torch.Tensor)) else w[0]) for w in whats]
    planes, pre = M.run_masks(M.plan_masks(whats, shapes, **kw), want_pre=True)
    torch.cuda.synchronize()
    return planes, pre


@pytest.fixture(scope="module")
def fixture_run():
    """Every fixture through ONE ragged launch per stage, as layers (one or three per mask, alternating) -> name: (plane, pre, scipy float64,
    scipy int64)."""
    whats = [R.layers_of(m, 1 + 2 * (i % 2), seed=i) for i, (_, m) in enumerate(FIXTURES)]
    planes, pre = _run(whats)
    return {name: (p.cpu().numpy(), q.cpu().numpy(), zoom(m.astype(np.float64), (1 / 4, 1 / 4)), zoom(m, (1 / 4, 1 / 4)))
            for (name, m), p, q in zip(FIXTURES, planes, pre)}


# ---------------------------------------------------------------------------------------------------- against scipy
@pytest.mark.parametrize("name", IDS)
def test_mask_equals_scipy_everywhere(name, fixture_run):
    plane, _, _, zi = fixture_run[name]
    want = np.clip(zi, 0, 1)[::-1].astype(np.float32)                       # :219 and :233, no rectangle, "unmasked"
    assert plane.dtype == np.float32 and plane.shape == (1, 1) + want.shape
    wrong = int((plane[0, 0] != want).sum())
    print(f"[inpaint_mask] {name}: {wrong} of {want.size} pixels differ from clip(zoom(int64 mask))")
    assert wrong == 0


@pytest.mark.parametrize("name", IDS)
def test_values_before_rounding_equal_scipy_float64(name, fixture_run):
    _, pre, zf, _ = fixture_run[name]
    err = np.abs(pre - zf).max()
    print(f"[inpaint_mask] {name}: float64 value before rounding vs scipy {err:.2e}")
    assert pre.dtype == np.float64 and err < PRE_TOL


# ---------------------------------------------------------------------------------------------------- the smallest shapes that can go wrong
SMALL = [(64, 36), (8, 8), (24, 82), (24, 86), (9, 7), (6, 130), (130, 6)]      # odd and narrow; every tap mirrors; quarters that round half to
#                                                                                even (20.5 -> 20, 21.5 -> 22); H W no multiple of 4 (single-pixel
#                                                                                layer path); more than one axis-1 tile; more than two axis-0 blocks


@pytest.fixture(scope="module")
def small_masks():
    return [R.random_mask(h, w, seed=100 + h + w) for h, w in SMALL]


@pytest.mark.parametrize("k", range(len(SMALL)), ids=["%dx%d" % s for s in SMALL])
def test_small_shapes(k, small_masks):
    m = small_masks[k]
    (plane,), (pre,) = _run([R.layers_of(m, 2, seed=k)])
    zf, zi = zoom(m.astype(np.float64), (1 / 4, 1 / 4)), zoom(m, (1 / 4, 1 / 4))
    half = np.abs(zf - (np.floor(zf) + 0.5)).min()
    err = np.abs(pre.cpu().numpy() - zf).max()
    print(f"[inpaint_mask] {m.shape} -> {zf.shape}: before rounding vs scipy {err:.2e}, closest half-integer at {half:.1e}")
    assert half > 1e-7                                                      # (the fixture property, for these masks too)
    assert zf.shape == _shape(m) and err < PRE_TOL
    assert np.array_equal(plane.cpu().numpy()[0, 0], np.clip(zi, 0, 1)[::-1].astype(np.float32))


@pytest.mark.parametrize("shape", [(5, 7), (7, 5), (2, 2), (5, 300), (70, 5)], ids=lambda s: "%dx%d" % s)
def test_prefilter_of_lines_shorter_than_the_run_in(shape):
    """n = 5 zooms to one sample, so the whole path refuses it; the prefilter itself takes it: the mirror extension then wraps many times
    inside the 40 samples of run-in."""
    h, w = shape
    m = R.random_mask(h, w, seed=h * w)
    IM = L.IM
    tab = np.zeros((1, IM["DS_IM_NI"]), np.int32)
    tab[0, IM["DS_IM_H"]], tab[0, IM["DS_IM_W"]] = h, w
    tab_dev, plane = torch.from_numpy(tab.reshape(-1)).cuda(), torch.from_numpy(m.astype(np.uint8).reshape(-1)).cuda()
    ws = torch.full((L.load().ds_mask_ws_bytes(h * w) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    L.call("ds_mask_prefilter", plane.data_ptr(), tab_dev.data_ptr(), 1, h, w, h * w, ws.data_ptr(), L.current_stream())
    got = ws[h * w:].view(h, w).cpu().numpy()
    want = R.prefilter(m)                                                   # pinned to scipy.ndimage.spline_filter1d in test_inpaint_mask_cpu.py
    err = np.abs(got - want).max()
    print(f"[inpaint_mask] prefilter {h}x{w}: vs the restatement {err:.2e}")
    assert err < PRE_TOL


def test_a_ragged_batch_equals_its_masks_alone_bit_for_bit(small_masks):
    whats = [R.layers_of(small_masks[0], 3, seed=1), small_masks[4], R.layers_of(small_masks[5], 1, seed=2)]      # layers, a merged plane, layers
    kw = dict(time_ranges=[(0.0, 0.5), None, (2.0, 5.0)], freq_ranges=[(1, 3), None, (-1, 9)], inpaint_areas=["masked", "unmasked", "masked"])
    planes, pre = _run(whats, **kw)
    for i, w in enumerate(whats):
        (p1,), (q1,) = _run([w], time_ranges=kw["time_ranges"][i], freq_ranges=kw["freq_ranges"][i], inpaint_areas=kw["inpaint_areas"][i])
        assert torch.equal(planes[i], p1) and torch.equal(pre[i], q1), i
        m = w if isinstance(w, np.ndarray) else R.merge_layers(w)
        want = R.latent_plane(m, kw["freq_ranges"][i], kw["time_ranges"][i], kw["inpaint_areas"][i])
        assert np.array_equal(planes[i].cpu().numpy()[0, 0], want), i


# ---------------------------------------------------------------------------------------------------- layers
def test_layer_cases():
    h, w = 64, 36
    zeros = lambda: np.zeros((h, w, 4), np.uint8)                            # noqa: E731
    m = R.random_mask(h, w, seed=7)
    (_,), (want,) = _run([m])                                               # the merged plane itself
    for n in (1, 3):
        layers = R.layers_of(m, n, seed=n)
        (_,), (got,) = _run([layers])
        assert torch.equal(got, want), n
        (_,), (got,) = _run([[torch.from_numpy(a).cuda() for a in layers]])                        # device tensors
        assert torch.equal(got, want), n
        (_,), (got,) = _run([[torch.from_numpy(a).cuda() if i % 2 else a for i, a in enumerate(layers)]])      # mixed
        assert torch.equal(got, want), n
    # alpha 1 in a single pixel of the last layer only: (42, 35) is where output (10, 8) reads (10 * 63 / 15 = 42, 8 * 35 / 8 = 35), and a spline
    # through the samples returns the sample there; the outputs around it are 4.2 and 4.4 samples away
    one = np.zeros((h, w), np.int64)
    one[42, 35] = 1
    last = zeros()
    last[42, 35, 3] = 1
    (_,), (want1,) = _run([one])
    (plane1,), (got1,) = _run([[zeros(), zeros(), last]])
    assert torch.equal(got1, want1) and abs(got1[10, 8].item() - 1.0) < PRE_TOL
    assert plane1.sum().item() == 1 and plane1[0, 0, 15 - 10, 8].item() == 1
    # a merged plane that holds 255 where it is painted (what alpha itself looks like) is the 0 / 1 plane
    (_,), (got255,) = _run([(m * 255).astype(np.uint8)])
    assert torch.equal(got255, want)
    # RGB set and alpha 0 does not count
    rgb = np.full((h, w, 4), 255, np.uint8)
    rgb[:, :, 3] = 0
    (plane0,), (got0,) = _run([[rgb, rgb]])
    assert got0.abs().max() == 0 and plane0.abs().max() == 0
    (_,), (got1,) = _run([[rgb, last, rgb]])
    assert torch.equal(got1, want1)


def test_public_entry_single_and_batch():
    m = R.blob_mask(64, 36, seed=3)
    layers = R.layers_of(m, 2, seed=4)
    kw = dict(time_range=(0.25, 1.0), freq_range=(2, 11), inpaint_area="masked")
    plane = M.latent_mask_from_layers(layers, latent_shape=(3, 4, 16, 9), **kw)
    assert plane.shape == (1, 1, 16, 9) and plane.dtype == torch.float32 and plane.is_cuda
    assert np.array_equal(plane.cpu().numpy()[0, 0], R.latent_plane(m, kw["freq_range"], kw["time_range"], "masked"))
    assert torch.equal(M.latent_mask_from_layers(m, latent_shape=(16, 9), **kw), plane)
    both = M.latent_mask_from_layers([layers, m], latent_shape=(16, 9), **kw)
    assert isinstance(both, list) and len(both) == 2 and torch.equal(both[0], plane) and torch.equal(both[1], plane)
    plane64 = M.latent_mask_from_layers(layers, latent_shape=(16, 9), time_resolution=64, **kw)      # 1 s = 4 columns
    assert np.array_equal(plane64.cpu().numpy()[0, 0], R.latent_plane(m, kw["freq_range"], kw["time_range"], "masked", 64))


@pytest.mark.parametrize("area", ["masked", "unmasked"])
def test_rectangle_inversion_and_flip(area):
    m = R.blob_mask(64, 36, seed=3)
    ranges = [(None, None), ((3, 9), (0.5, 2.0)), ((-5, -1), (1.0, 3.0)), ((9, 3), (0.0, 4.0)), ((0, 1000), (2.0, 1.0)), ((-1000, 4), (0.0, 100.0)),
              ((2.9, 7.2), (-1.0, 0.3)), ((5, 5), (0.0, 1.0))]
    planes, _ = _run([m] * len(ranges), freq_ranges=[fr for fr, _ in ranges], time_ranges=[tr for _, tr in ranges], inpaint_areas=area)
    for (fr, tr), p in zip(ranges, planes):
        want = R.reference_mask(m, 1, 1, fr, tr, area, zoom=zoom)             # the reference's lines with scipy and numpy's slice assignment
        assert np.array_equal(p.cpu().numpy(), want), (fr, tr)


def test_refusals_do_not_touch_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the request was checked")
    monkeypatch.setattr(L, "call", no_device)
    monkeypatch.setattr(M, "run_masks", no_device)
    lay = lambda h, w: torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")                # noqa: E731
    for layers, kw in (([], dict(latent_shape=(16, 9))), ([lay(64, 36), lay(64, 40)], dict(latent_shape=(16, 9))),
                       ([lay(64, 36)], dict(latent_shape=(16, 10))), ([lay(64, 5)], dict(latent_shape=(16, 1))), ([lay(4, 36)], dict(latent_shape=(1, 9))),
                       ([lay(64, 36)], dict(latent_shape=(16, 9), inpaint_area="all"))):
        with pytest.raises(ValueError):
            M.latent_mask_from_layers(layers, **kw)


# ---------------------------------------------------------------------------------------------------- serving
H = 32


@pytest.fixture(scope="module")
def unet(unet_sd):
    from diffusynth_amd.unet import ConditionedUnet, PRODUCTION_CONFIG
    m = ConditionedUnet(**PRODUCTION_CONFIG)
    m.load_state_dict(unet_sd)
    return m.to("cuda")


def test_inpaint_with_text_is_the_reference_shaped_call(unet):
    """Two requests of different widths and one with batchsize 2, fp32 tier, ddim: bit for bit what DiffSynthSampler.inpaint_sample returns
    for the reference-shaped (B, C, H, W) mask built with scipy and numpy."""
    from diffusynth_amd import serving
    unet.set_compute_dtype("fp32")
    steps = 3
    drawn = [R.blob_mask(4 * H, 80, seed=21), R.edge_mask(4 * H, 120, seed=22), R.random_mask(4 * H, 80, seed=23)]      # (120: scipy zeroes column 29)
    reqs = [dict(guide=synth_input("im_g0", (1, 4, H, 64)).cuda(), width=20, layers=R.layers_of(drawn[0], 3, seed=1), time_range=(0.5, 0.75), freq_range=(4, 9),
                 inpaint_area="masked", condition=synth_input("im_c0", (512,)), seed=11, noising_strength=0.6),
            dict(guide=synth_input("im_g1", (1, 4, H, 64)).cuda(), width=30, mask=drawn[1], time_range=None, freq_range=None, condition=synth_input("im_c1", (512,)),
                 seed=12, noising_strength=1.0),
            dict(guide=synth_input("im_g2", (1, 4, H, 64)).cuda(), width=20, layers=[torch.from_numpy(a).cuda() for a in R.layers_of(drawn[2], 1, seed=2)],
                 time_range=(0.0, 0.25), freq_range=(-6, 100), inpaint_area="unmasked", condition=synth_input("im_c2", (512,)), seed=13,
                 noising_strength=0.75, batchsize=2)]
    got = serving.inpaint_with_text(unet, reqs, steps, height=H)
    assert len(got) == 3
    for r, m, g in zip(reqs, drawn, got):
        B, W = r.get("batchsize", 1), r["width"]
        mask = torch.from_numpy(R.reference_mask(m, B, 4, r["freq_range"], r["time_range"], r.get("inpaint_area", "unmasked"), zoom=zoom)).cuda()
        assert mask.shape == (B, 4, H, W) and 0 < mask.mean() < 1
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, channels=4, noise_strategy="repeat")
        s.respace(list(np.linspace(0, 999, int(steps / r["noising_strength"]), dtype=np.int32)))
        want, _ = s.inpaint_sample(unet, (B, 4, H, W), r["noising_strength"], r["guide"].repeat(B, 1, 1, 1), mask, return_tensor=True,
                                   condition=r["condition"].cuda()[None].repeat(B, 1), sampler="ddim", seed=r["seed"])
        assert len(want) == int(int(steps / r["noising_strength"]) * r["noising_strength"]) + 1 > 2
        assert g.shape == (B, 4, H, W) and torch.equal(g, want[-1]), W
