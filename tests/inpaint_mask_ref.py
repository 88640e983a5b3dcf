"""Float64 restatement of the Inpaint tab's latent mask (diffusynth_amd/inpaint_mask.py, csrc/inpaint_mask.hip).

The definition is webUI/natural_language_guided_4/inpaint_with_text.py:204-233: scipy.ndimage.zoom(merged_mask, (1 / VAE_scale,) * 2) with
its defaults (order 3, mode "constant", prefilter, grid_mode False) on the INT64 0/1 mask, so the float64 spline value is rounded half away
from zero before the clip and the mask is binary; then the rectangle, the inversion and the flip.  tests/test_inpaint_mask_cpu.py pins this
file to the real scipy function.  numpy only.

  size       n_out = round(n / VAE_scale), half to even
  prefilter  along axis 0 then axis 1, whole-sample mirror boundary, pole z = sqrt(3) - 2, gain 6:
               c = 6 x;  zn = z^(n-1);  c[0] = (c[0] + zn c[n-1] + sum_{i=1..n-2} z^i (c[i] + zn c[n-1-i])) / (1 - zn^2)
               c[i] += z c[i-1];  c[n-1] = (z c[n-2] + c[n-1]) z / (z^2 - 1);  downwards c[i] = z (c[i+1] - c[i])
             (prefilter_segments: the same values from plain recursions over the mirror-extended line, cut into independent segments)
  taps       output i reads x = i ((n - 1) / (n_out - 1)), the ratio formed first as scipy forms it (the other order moves x by an ulp
             and the value by 1e-13): 4 taps at floor(x) - 1 .. floor(x) + 2, cubic B-spline weights, indices mirrored
  outside    mode "constant": an output whose coordinate is outside the input, x < 0 or x > n - 1 on either axis, is cval = 0.  For about
             one n in ten the LAST output's product (n_out - 1) ((n - 1) / (n_out - 1)) rounds an ulp above n - 1 (n = 30, 63, 120, 252,
             416 ...): scipy then zeroes the whole last row or column of the zoomed mask
  rounding   v > 0 ? floor(v + 0.5) : ceil(v - 0.5), clip to [0, 1]
"""
import numpy as np

POLE = np.sqrt(3.0) - 2.0
RUN_IN = 40                    # |POLE|^40 = 1.3e-23


def zoomed_size(n, VAE_scale=4):
    return int(round(n * (1.0 / VAE_scale)))


def merge_layers(layers):
    """average_np_arrays(layers)[:, :, -1] > 0 as int64 0/1 (a uint8 mean is positive exactly where some layer's alpha is)."""
    if len(layers) == 0:
        raise ValueError("no layers")
    mean = np.mean(np.stack([np.asarray(a) for a in layers]), axis=0)
    return np.where(mean[:, :, -1] > 0, 1, 0)


def prefilter_line(x):
    """scipy.ndimage.spline_filter1d(x, 3, mode="mirror") of one line, float64."""
    c = 6.0 * np.asarray(x, dtype=np.float64)
    n = len(c)
    z = POLE
    zn = z ** (n - 1)
    s = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        s += zi * (c[i] + zn * c[n - 1 - i])
        zi *= z
    c[0] = s / (1.0 - zn * zn)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def mirror(j, n):
    """Whole-sample mirror of any integer index into [0, n - 1]: -1 -> 1, n -> n - 2, period 2 (n - 1)."""
    p = 2 * (n - 1)
    j = np.mod(j, p)
    return np.where(j > n - 1, p - j, j)


def prefilter_segments(x, seg=16, run_in=RUN_IN):
    """prefilter_line by the kernel's form: every segment of `seg` samples runs c+[j] = 6 e[j] + z c+[j-1] from zero over the mirror-extended
    line e from `run_in` samples in front of it to `run_in` behind it, starts downwards from c[s1] = -sum_k z^(k+1) c+[s1 + k] over the
    samples behind it, and keeps c[j] = z (c[j+1] - c+[j]) of its own samples."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    z = POLE
    out = np.empty(n)
    for s0 in range(0, n, seg):
        s1 = min(s0 + seg, n)
        cp, body = 0.0, []
        for j in range(s0 - run_in, s1):
            cp = 6.0 * x[mirror(j, n)] + z * cp
            if j >= s0:
                body.append(cp)
        c, zp = 0.0, z
        for j in range(s1, s1 + run_in):
            cp = 6.0 * x[mirror(j, n)] + z * cp
            c -= zp * cp
            zp *= z
        for j in range(s1 - 1, s0 - 1, -1):
            c = z * (c - body[j - s0])
            out[j] = c
    return out


def prefilter(m, line=prefilter_line):
    """Both passes, axis 0 then axis 1."""
    c = np.asarray(m, dtype=np.float64)
    c = np.stack([line(c[:, j]) for j in range(c.shape[1])], axis=1)
    return np.stack([line(c[i]) for i in range(c.shape[0])], axis=0)


def taps(n_in, n_out):
    """(idx [n_out][4], w [n_out][4], outside [n_out]): the mirrored tap indices, their cubic B-spline weights, and whether the coordinate
    lies outside [0, n_in - 1] (the output is then 0)."""
    x = np.arange(n_out, dtype=np.float64) * ((n_in - 1) / (n_out - 1))
    f = np.floor(x).astype(np.int64)
    idx = f[:, None] + np.arange(-1, 3)[None, :]
    t = np.abs(x[:, None] - idx)
    w = np.where(t < 1.0, 2.0 / 3.0 - t * t + t * t * t / 2.0, np.where(t < 2.0, (2.0 - t) ** 3 / 6.0, 0.0))
    return mirror(idx, n_in), w, (x < 0) | (x > n_in - 1)


def zoom_float(m, VAE_scale=4, line=prefilter_line):
    """scipy.ndimage.zoom(m.astype(float64), (1 / VAE_scale,) * 2)."""
    H, W = m.shape
    c = prefilter(m, line)
    ih, wh, oh = taps(H, zoomed_size(H, VAE_scale))
    iw, ww, ow = taps(W, zoomed_size(W, VAE_scale))
    out = np.zeros((ih.shape[0], iw.shape[0]))
    for a in range(4):
        for b in range(4):
            out += wh[:, a][:, None] * ww[:, b][None, :] * c[ih[:, a][:, None], iw[:, b][None, :]]
    out[oh, :] = 0.0
    out[:, ow] = 0.0
    return out


def round_half_away(v):
    return np.where(v > 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def zoom_int(m, VAE_scale=4):
    """scipy.ndimage.zoom(m, (1 / VAE_scale,) * 2) of the int64 mask: int64, values in {-1, 0, 1, 2}."""
    return round_half_away(zoom_float(m, VAE_scale)).astype(np.int64)


def rect_bounds(H, W, freq_range=None, time_range=None, time_resolution=256, VAE_scale=4):
    """(r0, r1, c0, c1) of mask[int(fb):int(fe), int(tb time_resolution / (VAE_scale 4)):int(te ...)] on an (H, W) array, numpy's slice
    semantics resolved (r1 <= r0 or c1 <= c0: empty)."""
    fb, fe = (0, 0) if freq_range is None else freq_range
    tb, te = (0, 0) if time_range is None else time_range
    r0, r1, _ = slice(int(fb), int(fe)).indices(H)
    c0, c1, _ = slice(int(tb * time_resolution / (VAE_scale * 4)), int(te * time_resolution / (VAE_scale * 4))).indices(W)
    return r0, r1, c0, c1


def latent_plane(merged, freq_range=None, time_range=None, inpaint_area="unmasked", time_resolution=256, VAE_scale=4):
    """The (H_lat, W_lat) float32 plane after clip, rectangle, inversion and flip."""
    if inpaint_area not in ("masked", "unmasked"):
        raise ValueError(inpaint_area)
    m = np.clip(zoom_int(np.asarray(merged), VAE_scale), 0, 1)
    r0, r1, c0, c1 = rect_bounds(m.shape[0], m.shape[1], freq_range, time_range, time_resolution, VAE_scale)
    if r1 > r0 and c1 > c0:
        m[r0:r1, c0:c1] = 1
    if inpaint_area == "masked":
        m = 1 - m
    return m[::-1].astype(np.float32)


def reference_mask(merged, batchsize, channels, freq_range=None, time_range=None, inpaint_area="unmasked", time_resolution=256, VAE_scale=4, zoom=None):
    """inpaint_with_text.py:218-233 line for line with `zoom` (scipy.ndimage.zoom when given, else zoom_int): the (B, C, H, W) float32 array."""
    fb, fe = (0, 0) if freq_range is None else freq_range
    tb, te = (0, 0) if time_range is None else time_range
    latent_mask = zoom_int(merged, VAE_scale) if zoom is None else zoom(merged, (1 / VAE_scale, 1 / VAE_scale))
    latent_mask = np.clip(latent_mask, 0, 1)
    latent_mask[int(fb):int(fe), int(tb * time_resolution / (VAE_scale * 4)):int(te * time_resolution / (VAE_scale * 4))] = 1
    if inpaint_area == "masked":
        latent_mask = 1 - latent_mask
    out = np.broadcast_to(latent_mask[None, None], (batchsize, channels) + latent_mask.shape).astype(np.float32)
    return np.ascontiguousarray(out[:, :, ::-1])


# ---------------------------------------------------------------------------------------------------------------- fixtures
SHAPES = ((64, 36), (512, 80), (512, 81), (512, 82), (512, 83), (512, 576))
EDGE_SHAPES = ((512, 120), (512, 252), (120, 80), (128, 416))      # sizes whose last output coordinate rounds above n - 1 (120, 252, 416)


def outside_last(n, VAE_scale=4):
    """Whether the last output of an axis of n samples reads a coordinate above n - 1."""
    n_out = zoomed_size(n, VAE_scale)
    return bool((n_out - 1) * ((n - 1) / (n_out - 1)) > n - 1)


def random_mask(H, W, seed):
    return (np.random.default_rng(seed).random((H, W)) < 0.5).astype(np.int64)


def blob_mask(H, W, seed):
    """A few filled ellipses and a brush stroke: what a user paints."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), dtype=bool)
    for _ in range(4):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(3, H / 4), rng.uniform(3, max(4.0, W / 4))
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    m |= np.abs(yy - (H / 2 + H / 5 * np.sin(xx / 9.0))) < 3.5
    return m.astype(np.int64)


FIXTURE_SEEDS = {"random": 11, "blob": 5}


def fixtures():
    """[(name, int64 mask)]: a random and a blob mask per shape of SHAPES, a random and an edge-painted mask per shape of EDGE_SHAPES."""
    out = []
    for H, W in SHAPES:
        out.append(("random_%dx%d" % (H, W), random_mask(H, W, FIXTURE_SEEDS["random"] + W)))
        out.append(("blob_%dx%d" % (H, W), blob_mask(H, W, FIXTURE_SEEDS["blob"] + W)))
    for H, W in EDGE_SHAPES:
        out.append(("random_%dx%d" % (H, W), random_mask(H, W, FIXTURE_SEEDS["random"] + W)))
        out.append(("edge_%dx%d" % (H, W), edge_mask(H, W, FIXTURE_SEEDS["blob"] + W)))
    return out


def edge_mask(H, W, seed):
    """A blob mask painted up to its right and bottom edges: what scipy's constant mode cuts off at an affected size."""
    m = blob_mask(H, W, seed)
    m[:, -6:] = 1
    m[-6:, :] = 1
    return m


def layers_of(merged, n_layers, seed):
    """`n_layers` (H, W, 4) uint8 layers whose merged mask is `merged`: every painted pixel has alpha > 0 in at least one layer, RGB is
    arbitrary everywhere (also where alpha is 0)."""
    rng = np.random.default_rng(seed)
    H, W = merged.shape
    owner = rng.integers(0, n_layers, (H, W))
    layers = []
    for l in range(n_layers):
        a = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
        alpha = np.where((merged > 0) & ((owner == l) | (rng.random((H, W)) < 0.3)), rng.integers(1, 256, (H, W)), 0)
        a[:, :, 3] = alpha.astype(np.uint8)
        layers.append(a)
    return layers
