"""The Inpaint tab's latent mask without a device: the restatement (tests/inpaint_mask_ref.py) pinned to scipy.ndimage — called exactly as
webUI/natural_language_guided_4/inpaint_with_text.py:218 calls it, on the int64 mask — the size rule, the rectangle against numpy's own slice
assignment, both areas, the flip, the property of the fixtures that makes an exact comparison on the device fair, and the package's host
side: its refusals, its table, the entry points' argument checks."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage as nd

import inpaint_mask_ref as R
from conftest import ROOT
from diffusynth_amd import _lib as L
from diffusynth_amd import inpaint_mask as M

FIXTURES = R.fixtures()
IDS = [name for name, _ in FIXTURES]


@pytest.fixture(scope="module")
def scipy_zooms():
    """name -> (float64 zoom, int64 zoom), computed once."""
    return {name: (nd.zoom(m.astype(np.float64), (1 / 4, 1 / 4)), nd.zoom(m, (1 / 4, 1 / 4))) for name, m in FIXTURES}


# ---------------------------------------------------------------------------------------------------- the restatement against scipy
@pytest.mark.parametrize("n", [2, 3, 5, 36, 83, 512])
def test_prefilter_line_equals_scipy_spline_filter1d(n):
    x = np.random.default_rng(n).random(n)
    want = nd.spline_filter1d(x, 3, mode="mirror")
    assert np.abs(R.prefilter_line(x) - want).max() < 1e-14
    # the kernel's form: independent segments with 40 samples of run-in over the mirror extension (|z|^40 = 1.3e-23)
    assert np.abs(R.prefilter_segments(x) - want).max() < 1e-14
    assert abs(R.POLE) ** R.RUN_IN < 1e-22 and R.RUN_IN == L.IM["DS_IM_RUN_IN"]


@pytest.mark.parametrize("name,m", FIXTURES, ids=IDS)
def test_restatement_equals_scipy_zoom(name, m, scipy_zooms):
    f, i = scipy_zooms[name]
    assert i.dtype == np.int64 and f.shape == i.shape == (R.zoomed_size(m.shape[0]), R.zoomed_size(m.shape[1]))
    got = R.zoom_float(m)
    err = np.abs(got - f).max()
    print(f"[inpaint_mask] {name}: restatement vs scipy float64 {err:.1e}, int64 values {i.min()} .. {i.max()}")
    assert err < 1e-13
    assert np.array_equal(R.zoom_int(m), i)
    assert set(np.unique(i)) <= {-1, 0, 1, 2}
    assert np.array_equal(R.round_half_away(f).astype(np.int64), i)            # scipy's own rounding of its own float64 value


def test_the_segment_form_gives_the_same_zoom():
    name, m = FIXTURES[0]
    assert np.abs(R.zoom_float(m, line=R.prefilter_segments) - nd.zoom(m.astype(np.float64), (1 / 4, 1 / 4))).max() < 1e-13


def test_outputs_whose_coordinate_rounds_outside_the_input_are_zero():
    """scipy's mode "constant": for about one size in ten the last output's coordinate (n_out - 1) ((n - 1) / (n_out - 1)) rounds an ulp
    above n - 1 and the whole last row or column is cval = 0, whatever is painted there.  Every size from 8 to 400, on either axis."""
    hit = [n for n in range(8, 401) if R.outside_last(n)]
    assert hit[:11] == [30, 55, 58, 59, 63, 88, 95, 109, 111, 117, 120] and 252 in hit and R.outside_last(416) and not R.outside_last(512)
    for n in range(8, 401):
        m = R.random_mask(n, 12, seed=n)
        m[-2:] = 1                                                           # painted up to the edge
        for mm in (m, np.ascontiguousarray(m.T)):
            f, i = nd.zoom(mm.astype(np.float64), (1 / 4, 1 / 4)), nd.zoom(mm, (1 / 4, 1 / 4))
            clear = np.abs(f - (np.floor(f) + 0.5)) > 1e-7                  # (these masks are not picked to stay off the half-integers)
            assert np.abs(R.zoom_float(mm) - f).max() < 1e-13 and np.array_equal(R.zoom_int(mm)[clear], i[clear]) and clear.mean() > 0.9, n
        assert (np.abs(f[:, -1]).max() == 0) == (n in hit), n
    for name, m in FIXTURES:
        if name.startswith("edge_"):
            i = nd.zoom(m, (1 / 4, 1 / 4))
            assert m[:, -6:].all() and m[-6:].all()
            oh, ow = R.outside_last(m.shape[0]), R.outside_last(m.shape[1])
            assert i[:, -1].sum() == (0 if ow else i.shape[0] - oh) and i[-1].sum() == (0 if oh else i.shape[1] - ow), name      # (minus the corner)
            assert R.outside_last(m.shape[0]) or R.outside_last(m.shape[1]), name


@pytest.mark.parametrize("name,m", FIXTURES, ids=IDS)
def test_fixtures_stay_clear_of_every_half_integer(name, m, scipy_zooms):
    """What the exact comparison on the device relies on: a tie could only flip within the float64 error (bounded by 1e-12 there)."""
    f = scipy_zooms[name][0]
    d = np.abs(f - (np.floor(f) + 0.5)).min()
    print(f"[inpaint_mask] {name}: closest half-integer at {d:.1e}")
    assert d > 1e-7


def test_size_rule():
    assert [R.zoomed_size(n) for n in (80, 81, 82, 83, 86, 8, 6, 5)] == [20, 20, 20, 21, 22, 2, 2, 1]
    for n in list(range(6, 120)) + [512, 576]:
        assert nd.zoom(np.zeros((n, 8)), (1 / 4, 1 / 4)).shape[0] == R.zoomed_size(n) == M.zoomed_size(n), n
    assert M.zoomed_size(256, VAE_scale=8) == 32


# ---------------------------------------------------------------------------------------------------- rectangle, areas, flip
RANGES = [(None, None), ((3, 9), (0.5, 2.0)), ((-5, -1), (1.0, 3.0)), ((9, 3), (0.0, 4.0)), ((0, 1000), (2.0, 1.0)), ((-1000, 4), (0.0, 100.0)),
          ((2.9, 7.2), (-1.0, 0.3)), ((5, 5), (0.0, 1.0))]


@pytest.mark.parametrize("area", ["masked", "unmasked"])
def test_plane_equals_the_reference_lines_with_numpy_slices(area):
    m = dict(FIXTURES)["blob_64x36"]
    for fr, tr in RANGES:
        for time_resolution in (256, 64):
            want = R.reference_mask(m, 2, 4, fr, tr, area, time_resolution, zoom=nd.zoom)        # the reference's lines with scipy and numpy
            got = R.latent_plane(m, fr, tr, area, time_resolution)
            assert want.shape == (2, 4, 16, 9) and want.dtype == np.float32
            assert np.array_equal(np.broadcast_to(got[None, None], want.shape), want), (fr, tr)
            assert set(np.unique(got)) <= {0.0, 1.0}
            # the package resolves the same four integers
            assert M.rect_bounds(16, 9, fr, tr, time_resolution) == R.rect_bounds(16, 9, fr, tr, time_resolution)
            box = np.zeros((16, 9))
            r0, r1, c0, c1 = M.rect_bounds(16, 9, fr, tr, time_resolution)
            box[r0:max(r0, r1), c0:max(c0, c1)] = 1
            ref = np.zeros((16, 9))
            if fr is not None:
                ref[int(fr[0]):int(fr[1]), int(tr[0] * time_resolution / 16):int(tr[1] * time_resolution / 16)] = 1
            assert np.array_equal(box, ref), (fr, tr)


def test_areas_are_complements_and_the_frequency_axis_is_flipped():
    m = dict(FIXTURES)["blob_64x36"]
    a, b = R.latent_plane(m, (2, 5), (0.0, 1.0), "unmasked"), R.latent_plane(m, (2, 5), (0.0, 1.0), "masked")
    assert np.array_equal(a + b, np.ones_like(a))
    z = np.clip(R.zoom_int(m), 0, 1)
    z[2:5, 0:16] = 1                                                         # rows of the UNFLIPPED mask; 1 s = 16 columns, clipped to the 9 there are
    assert np.array_equal(a[::-1], z) and not np.array_equal(a, z)


def test_merge_is_any_alpha():
    m = dict(FIXTURES)["random_64x36"]
    for n in (1, 3):
        layers = R.layers_of(m, n, 3)
        assert np.array_equal(R.merge_layers(layers), m)
        assert np.array_equal(R.merge_layers(layers), np.any(np.stack(layers)[..., 3] > 0, axis=0).astype(np.int64))
    with pytest.raises(ValueError):
        R.merge_layers([])


# ---------------------------------------------------------------------------------------------------- the package's host side
def test_refusals_come_before_any_device_work():
    lay = lambda h, w: np.zeros((h, w, 4), np.uint8)                         # noqa: E731
    ok = dict(latent_shape=(1, 4, 16, 9))
    for layers, kw, match in (([], ok, "no layers"),
                              ([lay(64, 36), lay(64, 40)], ok, "unequal shape"),
                              ([lay(64, 36), lay(36, 64)], ok, "unequal shape"),
                              ([np.zeros((64, 36, 3), np.uint8)], ok, "uint8"),
                              ([np.zeros((64, 36, 4), np.float32)], ok, "uint8"),
                              ([lay(64, 36)], dict(latent_shape=(1, 4, 16, 10)), "zooms to 16 x 9"),
                              ([lay(64, 36)], dict(latent_shape=(1, 4, 9, 16)), "zooms to 16 x 9"),
                              ([lay(64, 82)], dict(latent_shape=(1, 4, 16, 21)), "zooms to 16 x 20"),
                              ([lay(1, 36)], dict(latent_shape=(1, 4, 0, 9)), "2 samples"),
                              ([lay(64, 5)], dict(latent_shape=(1, 4, 16, 1)), "2 samples"),
                              (np.zeros((64, 36)), dict(latent_shape=(16, 8)), "zooms to 16 x 9"),
                              ([lay(64, 36)], dict(inpaint_area="inverted", **ok), "inpaint_area"),
                              ([lay(64, 36)], dict(inpaint_area=None, **ok), "inpaint_area"),
                              (np.zeros((2, 64, 36, 4), np.uint8), ok, "expected a list"),
                              ([[lay(64, 36)], [lay(64, 36)]], dict(latent_shape=[(16, 9)]), "1 values for 2 masks")):
        with pytest.raises(ValueError, match=match):
            M.latent_mask_from_layers(layers, **kw)
    if not torch.cuda.is_available():                                        # a valid call: no CPU fallback
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.latent_mask_from_layers([lay(64, 36)], **ok)


def test_a_merged_plane_is_thresholded_whatever_its_dtype():
    painted = np.array([[0, 255], [1, 0]])
    for dt in (np.uint8, np.int64, np.float32, bool):
        assert M._flat_u8(painted.astype(dt), threshold=True).tolist() == [0, 1, 1, 0], dt
    assert M._flat_u8(torch.tensor([[0, 255]], dtype=torch.uint8), threshold=True).tolist() == [0, 1]
    assert M._flat_u8(painted.astype(np.uint8)).tolist() == [0, 255, 1, 0]      # a layer's bytes go to the kernel as they are


def test_plan_of_a_ragged_batch():
    lay = lambda h, w: np.zeros((h, w, 4), np.uint8)                         # noqa: E731
    specs = M.plan_masks([[lay(64, 36)] * 3, np.zeros((8, 8)), [torch.zeros(128, 82, 4, dtype=torch.uint8)]], [(16, 9), (2, 2), (1, 4, 32, 20)],
                         time_ranges=[(0.0, 1.0), None, (1.0, -1.0)], freq_ranges=(-3, 100), inpaint_areas=["masked", "unmasked", "masked"])
    assert [(s.H, s.W, s.HO, s.WO, len(s.layers), s.inv) for s in specs] == [(64, 36, 16, 9, 3, 1), (8, 8, 2, 2, 0, 0), (128, 82, 32, 20, 1, 1)]
    assert [s.rect for s in specs] == [(13, 16, 0, 9), (0, 2, 0, 0), (29, 32, 16, 4)]          # (a reversed time range: 16 .. 20 - 16, empty)


def test_serving_refusals_come_before_any_device_work():
    from diffusynth_amd import serving
    g = torch.zeros(1, 4, 32, 64)
    req = dict(guide=g, width=9, layers=[np.zeros((128, 36, 4), np.uint8)], condition=torch.zeros(512), seed=1, noising_strength=0.5)
    with pytest.raises(NotImplementedError, match="deterministic"):
        serving.inpaint_with_text(None, [req], 4, height=32, sampler="ddpm")
    for bad, match in ((dict(req, mask=np.zeros((128, 36))), "either 'layers' or 'mask'"),
                       ({k: v for k, v in req.items() if k != "layers"}, "either 'layers' or 'mask'"),
                       (dict(req, guide=g[0]), "guide"),
                       (dict(req, guide=torch.zeros(2, 4, 32, 64)), "guide"),
                       (dict(req, guide=torch.zeros(1, 4, 32, 9)), "guide"),
                       (dict(req, width=0), "width"),
                       ({k: v for k, v in req.items() if k != "width"}, "zooms to 32 x 9, the latent is .*64"),
                       (dict(req, batchsize=0), "batchsize"),
                       (dict(req, noising_strength=0.0), "noising_strength"),
                       (dict(req, noising_strength=1.5), "noising_strength"),
                       (dict(req, layers=[]), "no layers"),
                       (dict(req, layers=[np.zeros((128, 40, 4), np.uint8)]), "zooms to 32 x 10"),
                       (dict(req, inpaint_area="both"), "inpaint_area"),
                       ({k: v for k, v in req.items() if k != "seed"}, "seed"),
                       (dict(req, seed="7"), "seed"),
                       (dict(req, condition=torch.zeros(1, 512)), "condition"),
                       (dict(req, condition=np.zeros(512, np.float32)), "condition"),
                       (dict(req, condition=torch.zeros(512, dtype=torch.long)), "condition")):
        with pytest.raises(ValueError, match=match):
            serving.inpaint_with_text(None, [req, bad], 4, height=32)
    with pytest.raises(ValueError, match="unconditional_condition"):
        serving.inpaint_with_text(None, [req], 4, height=32, cfg_scale=3.0)
    with pytest.raises(ValueError, match="guide must be .*48"):                # the guide widths are the samplers' constructor arguments
        serving.inpaint_with_text(None, [req], 4, height=32, train_width=48)
    with pytest.raises(ValueError, match="guide must be .*256"):
        serving.inpaint_with_text(None, [req], 4, height=32, noise_strategy="non_repeat")
    assert serving.inpaint_with_text(None, [], 4) == []


def test_the_package_imports_without_scipy():
    import subprocess
    code = ("import sys; sys.modules['scipy'] = None; sys.path.insert(0, %r); import diffusynth_amd; from diffusynth_amd import inpaint_mask, serving; "
            "assert diffusynth_amd.latent_mask_from_layers is inpaint_mask.latent_mask_from_layers and diffusynth_amd.zoomed_size(83) == 21; "
            "assert not [m for m in sys.modules if m.startswith('scipy.')]" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------- header, binding, entry points
def test_header_and_binding_declare_the_entries():
    with open(os.path.join(ROOT, "include", "diffusynth_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", text))
    lib = L.load()
    for name in ("ds_mask_layers", "ds_mask_ws_bytes", "ds_mask_prefilter", "ds_mask_zoom"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert L.IM == {"DS_IM_LOFF": 0, "DS_IM_NL": 1, "DS_IM_POFF": 2, "DS_IM_H": 3, "DS_IM_W": 4, "DS_IM_OOFF": 5, "DS_IM_HO": 6, "DS_IM_WO": 7, "DS_IM_R0": 8,
                    "DS_IM_R1": 9, "DS_IM_C0": 10, "DS_IM_C1": 11, "DS_IM_INV": 12, "DS_IM_NI": 13, "DS_IM_RUN_IN": 40}
    assert lib.ds_mask_ws_bytes(512 * 576) == 2 * 8 * 512 * 576 and lib.ds_mask_ws_bytes(0) == 0


def test_entries_validate_before_any_gpu_work():
    lib = L.load()
    buf = (ctypes.c_char * 1024)()
    p = (ctypes.addressof(buf) + 63) & ~63
    big = 1 << 31
    for name, good, bads in (
            ("ds_mask_layers", [p, p, 1, 64, 64, 64, p, None], [(0, None), (1, None), (6, None), (2, 0), (2, 65536), (3, 3), (4, 0), (5, 0), (4, big), (5, big)]),
            ("ds_mask_prefilter", [p, p, 1, 8, 8, 64, p, None], [(0, None), (1, None), (6, None), (2, 0), (2, 65536), (3, 1), (4, 1), (5, 0), (5, big), (3, (1 << 20) + 1)]),
            ("ds_mask_zoom", [p, p, 1, 4, 64, 4, p, None, None], [(0, None), (1, None), (6, None), (2, 0), (2, 65536), (3, 3), (4, 0), (5, 0), (4, big), (5, big)])):
        fn = getattr(lib, name)
        for i, v in bads:
            args = list(good)
            args[i] = v
            assert fn(*args) == -1, (name, i, v)
            assert name[3:].encode() in lib.ds_last_error_string(), (name, i, v)
    assert lib.ds_mask_layers(p + 8, p, 1, 64, 64, 64, p, None) == -3 and lib.ds_mask_layers(p, p, 1, 64, 64, 64, p + 2, None) == -3
    assert lib.ds_mask_prefilter(p, p, 1, 8, 8, 64, p + 4, None) == -3
    assert lib.ds_mask_zoom(p + 4, p, 1, 4, 64, 4, p, None, None) == -3 and lib.ds_mask_zoom(p, p, 1, 4, 64, 4, p, p + 4, None) == -3
    with pytest.raises(L.DsError, match="mask_zoom"):
        L.call("ds_mask_zoom", p, p, 0, 4, 64, 4, p, None, None)
