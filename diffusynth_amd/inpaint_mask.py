"""What the user drew on the Inpaint tab into the mask `DiffSynthSampler.inpaint_sample` takes, on the GPU.

Replaces the numpy + scipy block of webUI/natural_language_guided_4/inpaint_with_text.py:204-233: average the ImageEditor layers, threshold
the alpha channel, `scipy.ndimage.zoom(merged_mask, (1 / VAE_scale, 1 / VAE_scale))`, clip, set the time / frequency rectangle to 1, invert
if the area is "masked", repeat to (B, C, H, W), flip the frequency axis.  Three launches for any number of masks (ds_mask_layers,
ds_mask_prefilter, ds_mask_zoom: include/diffusynth_hip.h has the definition) and one fp32 (1, 1, H_lat, W_lat) plane per mask, which the
sampler broadcasts over batch and channels itself (sampler.py:_loop_prologue keeps a one-channel mask as a plane).

The reference zooms the INT64 array `np.where(alpha > 0, 1, 0)`, so scipy interpolates in float64 and rounds half away from zero on output:
the zoomed mask holds -1 ... 2 and after np.clip it is BINARY — the spline's fractional values never reach the sampler.  The zoom is scipy's
with its defaults (cubic B-spline, prefilter with whole-sample mirror boundary, taps mirrored at the edges, 0 for an output whose
coordinate rounds to outside the input — the whole last row or column at about one size in ten — output size round(n / VAE_scale) with
Python's half-to-even round), restated in tests/inpaint_mask_ref.py and pinned to scipy there; this package does not import scipy.

What the host can round, floor or clip it does, in integers: the zoomed size and the rectangle's slice bounds (`slice(a, b).indices(n)`:
negative, reversed and out-of-range bounds as numpy resolves them).  No CPU fallback.
"""
import numpy as np
import torch

from . import _lib as L

_IM = L.IM
AREAS = ("masked", "unmasked")
_NO_GPU = "diffusynth_amd inpaint_mask runs on MI355X only (%s); no CPU fallback"


# ---------------------------------------------------------------------------------------------------- the definition, host side
def zoomed_size(n, VAE_scale=4):
    """The samples scipy.ndimage.zoom(x, 1 / VAE_scale) makes of n: int(round(n * (1 / VAE_scale))), Python's round (half to even): 80, 81
    and 82 give 20, 83 gives 21."""
    return int(round(int(n) * (1.0 / VAE_scale)))


def rect_bounds(H, W, freq_range=None, time_range=None, time_resolution=256, VAE_scale=4):
    """(r0, r1, c0, c1): rows and columns of `mask[int(fb):int(fe), int(tb * time_resolution / (VAE_scale * 4)):int(te * ...)] = 1` on the
    UNFLIPPED (H, W) latent mask, numpy's slice semantics resolved (r1 <= r0 or c1 <= c0: nothing is set).  None: no rectangle."""
    fb, fe = (0, 0) if freq_range is None else freq_range
    tb, te = (0, 0) if time_range is None else time_range
    r0, r1, _ = slice(int(fb), int(fe)).indices(H)
    c0, c1, _ = slice(int(tb * time_resolution / (VAE_scale * 4)), int(te * time_resolution / (VAE_scale * 4))).indices(W)
    return r0, r1, c0, c1


def _is_array(x):
    return isinstance(x, (np.ndarray, torch.Tensor))


def _is_spec(x):
    """One mask: a merged 2-D array, or a sequence of layers (an empty one included: it raises later, as the reference does)."""
    if _is_array(x):
        return x.ndim == 2
    return isinstance(x, (list, tuple)) and all(_is_array(a) and a.ndim == 3 for a in x)


def _dtype_is_uint8(a):
    return a.dtype == (torch.uint8 if isinstance(a, torch.Tensor) else np.uint8)


class _Spec:
    """Host side of one mask, checked: its layers (or merged plane), sizes, rectangle and area."""

    def __init__(self, what, latent_shape, VAE_scale, time_resolution, time_range, freq_range, inpaint_area, i):
        tag = "latent_mask_from_layers (mask %d)" % i
        if inpaint_area not in AREAS:
            raise ValueError(f"{tag}: inpaint_area must be 'masked' or 'unmasked' (got {inpaint_area!r})")
        if _is_array(what):
            if what.ndim != 2:
                raise ValueError(f"{tag}: a merged mask is a 2-D 0/1 array (got shape {tuple(what.shape)})")
            self.layers, self.merged = [], what
            self.H, self.W = (int(v) for v in what.shape)
        else:
            layers = list(what)
            if not layers:
                raise ValueError(f"{tag}: no layers (the list of arrays is empty)")
            for a in layers:
                if not _is_array(a) or a.ndim != 3 or a.shape[2] != 4 or not _dtype_is_uint8(a):
                    raise ValueError(f"{tag}: a layer is an (H, W, 4) uint8 array or tensor")
                if tuple(a.shape) != tuple(layers[0].shape):
                    raise ValueError(f"{tag}: layers of unequal shape, {tuple(layers[0].shape)} and {tuple(a.shape)}")
            self.layers, self.merged = layers, None
            self.H, self.W = (int(v) for v in layers[0].shape[:2])
        self.HO, self.WO = zoomed_size(self.H, VAE_scale), zoomed_size(self.W, VAE_scale)
        if min(self.H, self.W, self.HO, self.WO) < 2:
            raise ValueError(f"{tag}: every axis needs 2 samples before and after the zoom ({self.H} x {self.W} -> {self.HO} x {self.WO})")
        if latent_shape is None or tuple(int(v) for v in tuple(latent_shape)[-2:]) != (self.HO, self.WO):
            raise ValueError(f"{tag}: a {self.H} x {self.W} drawing zooms to {self.HO} x {self.WO}, the latent is {latent_shape!r}")
        self.rect = rect_bounds(self.HO, self.WO, freq_range, time_range, time_resolution, VAE_scale)
        self.inv = 1 if inpaint_area == "masked" else 0


def _per_mask(v, n, is_one):
    """One value for every mask (is_one(v)), or a list with one per mask."""
    if is_one(v):
        return [v] * n
    if len(v) != n:
        raise ValueError("latent_mask_from_layers: %d values for %d masks" % (len(v), n))
    return list(v)


def _one_shape(v):
    return v is None or not len(v) or not isinstance(v[0], (list, tuple))


def _one_range(v):
    return v is None or not (isinstance(v, (list, tuple)) and len(v) and (v[0] is None or isinstance(v[0], (list, tuple))))


def plan_masks(whats, latent_shapes, VAE_scale=4, time_resolution=256, time_ranges=None, freq_ranges=None, inpaint_areas="unmasked"):
    """The checked host side of a list of masks (every ValueError of the module is raised here, before any device work).  Every argument
    after `whats` is one value for all masks or a list with one per mask."""
    n = len(whats)
    shapes, trs, frs = _per_mask(latent_shapes, n, _one_shape), _per_mask(time_ranges, n, _one_range), _per_mask(freq_ranges, n, _one_range)
    areas = _per_mask(inpaint_areas, n, lambda v: not isinstance(v, (list, tuple)))
    return [_Spec(w, s, VAE_scale, time_resolution, t, f, a, i) for i, (w, s, t, f, a) in enumerate(zip(whats, shapes, trs, frs, areas))]


def _flat_u8(a, threshold=False):
    """A layer as a flat uint8 tensor on whatever device it is on; threshold: a merged plane of any dtype as 0 / 1 (> 0, as the
    reference thresholds alpha: a plane that holds 255 where it is painted means what one that holds 1 does)."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if threshold:
        t = (t > 0).to(torch.uint8)
    return t.detach().contiguous().reshape(-1)


def _gather(parts, dev):
    """Flat tensors back to back on dev: one host concatenation and one upload when all are on the host."""
    if len(parts) == 1:
        t = parts[0].to(dev)
    elif all(not p.is_cuda for p in parts):
        t = torch.cat(parts).to(dev)
    else:
        t = torch.cat([p.to(dev) for p in parts])
    return t if t.data_ptr() % 16 == 0 else t.clone()


@torch.no_grad()
def run_masks(specs, device="cuda", want_pre=False):
    """The three launches for a list of checked masks -> (planes, pre): planes[i] the fp32 (1, 1, HO, WO) plane of mask i (views of one
    buffer), pre[i] the float64 (HO, WO) values before rounding, unflipped (None unless asked for)."""
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU % "latent_mask_from_layers")
    dev = torch.device(device)
    n = len(specs)
    tab = np.zeros((n, _IM["DS_IM_NI"]), dtype=np.int32)
    parts, loff, poff, ooff = [], 0, 0, 0
    for i, s in enumerate(specs):
        hw = s.H * s.W
        tab[i, _IM["DS_IM_LOFF"]], tab[i, _IM["DS_IM_NL"]] = loff, len(s.layers)
        tab[i, _IM["DS_IM_POFF"]], tab[i, _IM["DS_IM_H"]], tab[i, _IM["DS_IM_W"]] = poff, s.H, s.W
        tab[i, _IM["DS_IM_OOFF"]], tab[i, _IM["DS_IM_HO"]], tab[i, _IM["DS_IM_WO"]] = ooff, s.HO, s.WO
        tab[i, _IM["DS_IM_R0"]:_IM["DS_IM_C1"] + 1] = s.rect
        tab[i, _IM["DS_IM_INV"]] = s.inv
        parts += [_flat_u8(a) for a in s.layers]
        loff += hw * len(s.layers)
        poff += (hw + 3) & ~3                          # every plane starts at a multiple of 4 pixels (ds_mask_layers' 4-byte stores)
        ooff += s.HO * s.WO
    if max(loff, poff) >= 2 ** 31 - 1 - 1024:
        raise ValueError("latent_mask_from_layers: %d pixels in one batch (at most 2^31 - 1025)" % max(loff, poff))
    with torch.cuda.device(dev):
        tab_dev = torch.from_numpy(tab.reshape(-1)).to(dev)
        planes = torch.empty(poff, dtype=torch.uint8, device=dev)
        for i, s in enumerate(specs):
            if s.merged is not None:
                o = int(tab[i, _IM["DS_IM_POFF"]])
                planes[o:o + s.H * s.W].copy_(_flat_u8(s.merged, threshold=True))
        st = L.current_stream()
        if parts:
            lay = _gather(parts, dev)
            L.call("ds_mask_layers", lay.data_ptr(), tab_dev.data_ptr(), n, max(s.H * s.W for s in specs), loff, poff, planes.data_ptr(), st)
        ws = torch.empty(L.load().ds_mask_ws_bytes(poff) // 8, dtype=torch.float64, device=dev)
        L.call("ds_mask_prefilter", planes.data_ptr(), tab_dev.data_ptr(), n, max(s.H for s in specs), max(s.W for s in specs), poff, ws.data_ptr(), st)
        out = torch.empty(ooff, dtype=torch.float32, device=dev)
        pre = torch.empty(ooff, dtype=torch.float64, device=dev) if want_pre else None
        L.call("ds_mask_zoom", ws.data_ptr(), tab_dev.data_ptr(), n, max(s.HO * s.WO for s in specs), poff, ooff, out.data_ptr(), L.ptr(pre), st)
    offs = tab[:, _IM["DS_IM_OOFF"]].tolist()
    views = [out[o:o + s.HO * s.WO].view(1, 1, s.HO, s.WO) for o, s in zip(offs, specs)]
    pres = [pre[o:o + s.HO * s.WO].view(s.HO, s.WO) for o, s in zip(offs, specs)] if want_pre else None
    return views, pres


# ---------------------------------------------------------------------------------------------------- public
def latent_mask_from_layers(layers, *, latent_shape, VAE_scale=4, time_resolution=256, time_range=None, freq_range=None,
                            inpaint_area="unmasked", device="cuda"):
    """inpaint_with_text.py:204-233 -> the fp32 (1, 1, H_lat, W_lat) device plane `inpaint_sample(mask=)` takes (it stands for the
    reference's (B, C, H_lat, W_lat) repeat: the sampler broadcasts it).

    layers: the ImageEditor's `["layers"]` — a list of (H, W, 4) uint8 numpy arrays or tensors on either device — or an already merged 2-D
    0/1 array; or a list of such entries for a batch, which returns a list of planes from the same three launches (latent_shape,
    time_range, freq_range and inpaint_area are then one value for all or a list with one per mask).
    latent_shape: the latent's shape (its last two entries count); time_range (begin, end) in seconds and freq_range (begin, end) in
    latent rows of the unflipped mask: the rectangle set to 1, with numpy's slice semantics; inpaint_area: "masked" inverts.

    ValueError, before any device work: an empty list of layers, layers of unequal shape or not (H, W, 4) uint8, a zoomed size other than
    latent_shape[-2:], an axis shorter than 2 before or after the zoom, an inpaint_area other than the two names."""
    single = _is_spec(layers)
    if not single and not (isinstance(layers, (list, tuple)) and layers and all(_is_spec(w) for w in layers)):
        raise ValueError("latent_mask_from_layers: expected a list of (H, W, 4) uint8 layers, a merged 2-D mask, or a list of those")
    if single:
        specs = [_Spec(layers, latent_shape, VAE_scale, time_resolution, time_range, freq_range, inpaint_area, 0)]
    else:
        specs = plan_masks(list(layers), latent_shape, VAE_scale, time_resolution, time_range, freq_range, inpaint_area)
    planes, _ = run_masks(specs, device)
    return planes[0] if single else planes
