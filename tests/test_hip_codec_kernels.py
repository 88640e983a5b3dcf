"""The codec tail (csrc/tail.hip, csrc/stft_codec.hpp) through the C ABI, on every path its launchers take: ds_vq_nearest, ds_vq_stats,
ds_decoder_tail, ds_istft_plus, ds_istft_plus_loop and ds_stft_plus.  Cases, float64 references, fp32 restatements ("twins") and defect
models: tests/codec_ref.py; tests/test_codec_ref_cpu.py shows without a GPU that every case meets its preconditions, that every twin is
within its rule and that every defect model changes the tensor compared here.

No tolerance is a constant.  A comparison is exact (exact_ref.assert_bits_equal against float64, on data whose margin the builder asserts),
or the measured rule of tests/test_hip_timbre.py / tests/test_hip_support_kernels.py: the device may land four times as far from float64
as the fp32 twin does (conftest.rel_err), both measured in the same run, or one of the two derived bounds of codec_ref.py (VQ_C for a
near-tie of the quantiser, UNIT_NORM_BOUND for |c1^2 + c2^2 - 1|).  Every figure is printed, and appended to $DS_CODEC_PARITY_LOG when
that is set (profiles/codec_kernels_parity.txt keeps those of one green run).

Every input, output and workspace lives in a support_ref.slab: a view inside a NaN-filled allocation, some one float off 16-byte alignment;
inputs are checked unchanged after the call.

Which case reaches which launcher branch:
  ds_vq_nearest, vq_mfma_kernel
    one code tile                        ncodes = 1, 15, 16
    padding codes (ncodes % 16 != 0)     ncodes = 1, 15, 17, 65, 100, 1000 (the zero pixel 0 would choose a padding code of distance 0)
    clamped prefetch (ntiles < 4)        ncodes = 1 .. 48 (1, 1, 1, 2, 3 tiles)
    group boundary                       ncodes = 48, 64, 65 (3, 4, 5 tiles)
    last tile examined again             ntiles % 4 = 1: 65;  2: 17;  3: 48, 100, 1000 (63 tiles) — in ties and mid the tile holds copies of earlier codes
    full loop                            ncodes = 8192 (512 tiles)
    npix < 16, one wave, one block, more (B, HW) = (1, 1), (1, 15) | (1, 16), (1, 17), (1, 128) | (1, 129), (1, 512) | (1, 513)
    a 16-pixel tile over two samples     (B, HW) = (3, 5), (2, 77), (5, 103)
    idx = NULL                           test_vq_nearest_without_indices
    B half decides a tie                 pixels 64 .. 127 of every wave in every case of 128 pixels or more, and by construction in
                                         test_vq_nearest_placed_ties (every pixel tile of every wave; ties inside a lane, between lane groups,
                                         between tiles of one prefetch group, between the first and the last tile)
    g_vq_pack rewritten per call         test_vq_nearest_answers_from_the_new_codebook
  ds_vq_nearest, vq_kernel<4>            ncodes = 8193, 8200 (data sets ties, mid, elow: |z|^2 fits too)
  ds_vq_stats                            second grid trip with ragged tail: npix = 2048 x 256 + 37;  second finish trip: ncodes = 1025, 8192;
                                         indices outside [0, ncodes): usage "outside";  counts cleared per call: every case runs twice on one ws
  ds_decoder_tail                        fp32 and bf16; softplus threshold: the bands of 19.99, 20 and nextafter(20); Cs = 3, 5, 8 with NaN in
                                         channels 3 up;  second grid pass: 8192 x 256 + 2048 pixels, Cs = 3, fp32
  ds_istft_plus                          T = 2 (smallest): (2, 256), (2, 1024);  hop = frame: (2, 1024);  vector gather (T % 4 == 0): (4, 256),
                                         (8, 128), (12, 256);  scalar gather, ragged last block: (2, .), (5, 256), (9, 128), (3, 512), (13, 256);
                                         eight overlapping frames, both clamps of t_lo / t_hi: (8, 128), (9, 128);  misaligned view of a
                                         vector-eligible shape: (8, 128) one float off
  ds_istft_plus_loop                     (8, 128), (2, 512), (4, 256): the smallest T of each hop
  ds_stft_plus                           smallest reflect-padded signal: L = 513;  L not a multiple of hop: 1000 / 256, 1500 / 100;  hops 100, 128,
                                         256, 512;  one frame: L = 1;  T_out = T, T + 1, T + 7;  digital silence;  a signal of 2^-70
  host-side refusals                     test_host_side_refusals"""
import os

import numpy as np
import pytest
import torch

import codec_ref as R
import exact_ref as E
import support_ref as S
from conftest import rel_err
from diffusynth_amd import _lib as L

pytestmark = pytest.mark.gpu


def note(line):
    """Figures worth keeping (profiles/codec_kernels_parity.txt): printed, and appended to $DS_CODEC_PARITY_LOG when that is set."""
    print(line)
    path = os.environ.get("DS_CODEC_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def rule(what, dev, twin, f64):
    """The measured rule: dev within 4 x (fp32 twin vs float64) of float64; a twin at distance zero makes the comparison exact."""
    dev, twin, f64 = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t.cpu()) for t in (dev, twin, f64))
    assert tuple(dev.shape) == tuple(f64.shape) == tuple(twin.shape) and bool(torch.isfinite(dev).all()), what
    cpu, err = rel_err(twin, f64), rel_err(dev, f64)
    note(f"{what}: device vs float64 {err:.3e}, fp32 twin vs float64 {cpu:.3e}")
    assert err <= 4 * cpu, (what, err, cpu)
    return err, cpu


def sync():
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def unchanged(view, src):
    assert torch.equal(bits(view).cpu(), bits(src.to(view.dtype)))


def idx_slab(n, values=None):
    """An int64 [n] view on an int32 slab (support_ref.slab holds 4- and 2-byte types): NaN bit patterns, or `values`."""
    raw = S.nan_slab((2 * n,), torch.int32)
    v = raw.view(torch.int64)
    if values is not None:
        v.copy_(values)
    return raw, v


# ================================================================================================= ds_vq_nearest
def _vq_call(z, cb, esq, B, HW, ncodes, q, idx):
    L.call("ds_vq_nearest", z.data_ptr(), cb.data_ptr(), esq.data_ptr(), B, 4, HW, ncodes, q.data_ptr(), L.ptr(idx), L.current_stream())


def _vq_run(c, B, HW, off=0, with_idx=True, codes=None):
    """One launch on the first B * HW pool pixels of data set c; returns (idx [npix] int64 cpu or None, q [npix][4] fp32 cpu)."""
    zc = R.vq_layout(c.z, B, HW).float()
    cbc, esqc = c.cb.float(), c.esq.float()
    z, cb, esq = S.slab(zc, offset_floats=off), codes[0] if codes else S.slab(cbc, offset_floats=off), codes[1] if codes else S.slab(esqc, offset_floats=off)
    q = S.nan_slab((B, 4, HW), offset_floats=off)
    raw, idx = idx_slab(B * HW) if with_idx else (None, None)
    _vq_call(z, cb, esq, B, HW, c.ncodes, q, idx)
    sync()
    S.check_guards(*(t for t in (z, cb, esq, q, raw) if t is not None))
    unchanged(z, zc)
    unchanged(cb, cbc)
    unchanged(esq, esqc)
    return (idx.cpu() if with_idx else None), R.vq_unlayout(q.cpu())


def _vq_exact(c, B, HW, off=0, codes=None):
    npix = B * HW
    idx, q = _vq_run(c, B, HW, off, codes=codes)
    what = f"ds_vq_nearest {c.kind} ncodes={c.ncodes} B={B} HW={HW}"
    E.assert_bits_equal(idx, c.idx[:npix], what + " idx")
    E.assert_bits_equal(q, R.vq_q(c.z[:npix], c.cb, c.idx[:npix]), what + " q")
    assert torch.equal(q.double(), c.cb[c.idx[:npix]])                        # integers: z + (e - z) is e


@pytest.mark.parametrize("kind", R.VQ_SETS)
@pytest.mark.parametrize("ncodes", R.VQ_NCODES)
def test_vq_nearest_exact(ncodes, kind):
    """Every (B, HW) of the list with every ncodes and every data set: the float64 first minimum at every pixel, q bit for bit.  The
    codebook and esq are uploaded once per (data set, ncodes); (B, HW) = (1, 17) and (2, 77) run one float off 16-byte alignment."""
    c = R.vq_data(kind, ncodes)
    codes = (S.slab(c.cb.float()), S.slab(c.esq.float()))
    for B, HW in R.VQ_BHW:
        _vq_exact(c, B, HW, off=1 if (B, HW) in ((1, 17), (2, 77)) else 0, codes=codes)
    note(f"ds_vq_nearest exact {kind} ncodes={ncodes}: margin {c.margin:.4g} of 2^24, tied minima on {c.tied.double().mean().item():.3f} of the pixels, "
         f"shares of operands with a second / third part: z {c.shares['z2']:.2f} / {c.shares['z3']:.2f}, -2 cb {c.shares['e2']:.2f} / {c.shares['e3']:.2f}, "
         f"esq {c.shares['q2']:.2f} / {c.shares['q3']:.2f}: {len(R.VQ_BHW)} launches equal to float64")


@pytest.mark.parametrize("kind", [k for k in R.VQ_SETS if k != "zlow"])
@pytest.mark.parametrize("ncodes", R.VQ_NCODES_SCALAR)
def test_vq_nearest_scalar_fallback_exact(ncodes, kind):
    c = R.vq_data(kind, ncodes)
    assert ncodes > 8192 and c.scalar_exact
    for B, HW in ((1, 1), (1, 257), (5, 103)):
        _vq_exact(c, B, HW)


def test_vq_nearest_placed_ties():
    c = R.vq_placed_ties()
    idx, q = _vq_run(c, 1, 512)
    for p, (a, b) in c.placed.items():
        assert idx[p].item() == a, (p, a, b, idx[p].item())
    E.assert_bits_equal(idx, c.idx, "ds_vq_nearest placed ties idx")
    E.assert_bits_equal(q, R.vq_q(c.z, c.cb, c.idx), "ds_vq_nearest placed ties q")


@pytest.mark.parametrize("ncodes", [100, 8200])
def test_vq_nearest_without_indices(ncodes):
    c = R.vq_data("mid", ncodes)
    idx, q = _vq_run(c, 2, 77, with_idx=False)
    assert idx is None
    E.assert_bits_equal(q, R.vq_q(c.z[:154], c.cb, c.idx[:154]), "ds_vq_nearest idx = NULL q")


def test_vq_nearest_answers_from_the_new_codebook():
    """g_vq_pack is a device global: a launch with another codebook right after the first answers from the new one."""
    a, b = R.vq_data("mid", 1000), R.vq_data("ties", 100)
    for first, second in ((a, b), (b, a)):
        z1, cb1, e1 = S.slab(R.vq_layout(first.z, 1, 513).float()), S.slab(first.cb.float()), S.slab(first.esq.float())
        z2, cb2, e2 = S.slab(R.vq_layout(second.z, 1, 513).float()), S.slab(second.cb.float()), S.slab(second.esq.float())
        q1, q2 = S.nan_slab((1, 4, 513)), S.nan_slab((1, 4, 513))
        (r1, i1), (r2, i2) = idx_slab(513), idx_slab(513)
        _vq_call(z1, cb1, e1, 1, 513, first.ncodes, q1, i1)
        _vq_call(z2, cb2, e2, 1, 513, second.ncodes, q2, i2)
        sync()
        S.check_guards(z1, cb1, e1, z2, cb2, e2, q1, q2, r1, r2)
        E.assert_bits_equal(i1.cpu(), first.idx[:513], "first launch")
        E.assert_bits_equal(i2.cpu(), second.idx[:513], "second launch, other codebook")
        E.assert_bits_equal(R.vq_unlayout(q2.cpu()), R.vq_q(second.z[:513], second.cb, second.idx[:513]), "second launch q")


@pytest.mark.parametrize("book,zscale", R.VQ_FLOAT)
def test_vq_nearest_float_data_within_the_derived_bound(book, zscale):
    """Production-like data: the float64 distance of the chosen code exceeds the float64 minimum by at most VQ_C 2^-24 (esq + 2 sum |z||e|)
    at the worse of the two codes (codec_ref.py derives VQ_C); where the index is the float64 argmin q is bit-equal."""
    c = R.vq_float_case(book, zscale)
    zc = R.vq_layout(c.z, c.B, c.HW)
    z, cb, esq = S.slab(zc, offset_floats=1), S.slab(c.cb), S.slab(c.esq)
    q = S.nan_slab((c.B, 4, c.HW), offset_floats=1)
    raw, idx = idx_slab(c.B * c.HW)
    _vq_call(z, cb, esq, c.B, c.HW, 8192, q, idx)
    sync()
    S.check_guards(z, cb, esq, q, raw)
    unchanged(z, zc)
    unchanged(cb, c.cb)
    got = idx.cpu()
    assert int(got.min()) >= 0 and int(got.max()) < 8192
    excess, allow, ref = R.vq_excess(c.z, c.cb, c.esq, got)
    worst = (excess / allow).max().item()
    note(f"ds_vq_nearest float {book} z x {zscale}: {int((got != ref).sum())} of {got.numel()} indices differ from the float64 argmin, worst excess "
         f"{worst:.4f} of the bound {R.VQ_C:g} x 2^-24 x S")
    assert bool((excess <= allow).all()), worst
    E.assert_bits_equal(R.vq_unlayout(q.cpu()), R.vq_q(c.z, c.cb, got), "q of the chosen code")


# ================================================================================================= ds_vq_stats
def _vqs_run(c, ws, cc, ema):
    zc, qc = c.z.float(), c.q.float()
    z, q = S.slab(zc, offset_floats=1), S.slab(qc)
    raw, idx = idx_slab(c.npix, c.idx.cuda())
    out = S.nan_slab((3,))
    L.call("ds_vq_stats", z.data_ptr(), q.data_ptr(), idx.data_ptr(), c.B, c.D, c.HW, c.ncodes, cc, ema, out.data_ptr(), ws.data_ptr(), L.current_stream())
    sync()
    S.check_guards(z, q, raw, out, ws)
    unchanged(z, zc)
    unchanged(q, qc)
    assert torch.equal(idx.cpu(), c.idx)
    return out.cpu()


VQS_PAIRS = [(R.VQS_CASES[i], R.VQS_CASES[(i + 1) % len(R.VQS_CASES)]) for i in range(len(R.VQS_CASES))]


@pytest.mark.parametrize("case,other", VQS_PAIRS, ids=["D%d_B%d_HW%d_K%d_%s" % a for a, _ in VQS_PAIRS])
def test_vq_stats(case, other):
    """mse and loss bit for bit on integer data, both flavours; ws exactly ds_vq_stats_ws_bytes long inside its slab and used twice: first
    by a call with the counts of ANOTHER usage pattern over the same codes, then by the case (the counts are cleared per call).  The
    perplexities are held to the rule as one vector by test_vq_stats_perplexities; with every pixel on one code it is exactly 1.0."""
    c = R.vqs_case(*case)
    o = R.vqs_case(c.D, c.B, c.HW, c.ncodes, other[4] if other[4] not in ("uniform", c.usage) else "high")
    nbytes = L.load().ds_vq_stats_ws_bytes(c.ncodes)
    assert nbytes == c.ncodes * 4 + 2048 * 8 + 8
    ws = S.nan_slab((nbytes // 4,))
    _vqs_run(o, ws, 0.25, 1)
    for cc, ema in ((0.25, 1), (0.4, 0)):
        got = _vqs_run(c, ws, cc, ema)
        mse, loss, p32, p64 = R.vqs_expect(c, cc, ema)
        E.assert_bits_equal(got[0], mse, f"ds_vq_stats mse {case}")
        E.assert_bits_equal(got[2], loss, f"ds_vq_stats loss {case} ema={ema}")
        if c.usage == "one":
            assert got[1].item() == 1.0
        note(f"ds_vq_stats D={c.D} npix={c.npix} ncodes={c.ncodes} {c.usage} ema={ema}: mse, loss bit-equal; perplexity device {got[1].item()!r}, "
             f"fp32 twin {p32.item()!r}, float64 {p64.item()!r}")


def test_vq_stats_perplexities():
    """Every case's perplexity divided by its float64 value, as one vector under the rule (codec_ref.py says why not one by one); uniform
    usage of 64 codes gives 64 by that rule."""
    dev, twin, f64 = [], [], []
    for case in R.VQS_CASES:
        c = R.vqs_case(*case)
        ws = S.nan_slab((L.load().ds_vq_stats_ws_bytes(c.ncodes) // 4,))
        got = _vqs_run(c, ws, 0.25, 1)
        _, _, p32, p64 = R.vqs_expect(c, 0.25, 1)
        dev.append(got[1].item())
        twin.append(p32.item())
        f64.append(p64.item())
    f64 = torch.tensor(f64, dtype=torch.float64)
    rule("ds_vq_stats perplexity / float64, all cases", torch.tensor(dev, dtype=torch.float64) / f64, torch.tensor(twin, dtype=torch.float64) / f64,
         torch.ones_like(f64))


# ================================================================================================= ds_decoder_tail
def _tail_call(x, dt, B, Cs, HW, off=0):
    xd = S.slab(x, offset_floats=off)
    out = S.nan_slab((B, 3, HW), offset_floats=off)
    L.call("ds_decoder_tail", xd.data_ptr(), dt, B, Cs, HW, out.data_ptr(), L.current_stream())
    sync()
    S.check_guards(xd, out)
    assert torch.equal(bits(xd[..., :3]).cpu(), bits(x[..., :3])) and bool(torch.isnan(xd[..., 3:]).all())
    return out.cpu()


def _tail_bands(what, vals, band, got, twin, f64):
    """Channel 0 (softplus) and channels 1, 2 (tanh) of every group of bands (codec_ref.tail_groups) under the rule; the figures of the worst
    group are noted."""
    n = vals.numel()
    flat = lambda t: t.permute(1, 0, 2).reshape(3, -1)[:, :n]                                             # noqa: E731
    g, t, f = flat(got), flat(twin), flat(f64)
    assert bool(torch.isfinite(got).all())
    worst, ngroups = {}, {}
    anchor = R.tail_anchor(vals, band)
    for name, rows in (("softplus", slice(0, 1)), ("tanh", slice(1, 3))):
        group = R.tail_groups(f[rows], band, anchor)
        ngroups[name] = len(group.unique())
        for k in group.unique().tolist():
            m = group == k
            cpu, err = rel_err(t[rows][:, m], f[rows][:, m]), rel_err(g[rows][:, m], f[rows][:, m])
            assert err <= 4 * cpu, (what, name, "group", k, vals[m][0].item(), err, cpu)
            w = worst.get(name)
            if w is None or err > w[0]:
                worst[name] = (err, cpu, vals[m].abs().min().item(), vals[m].abs().max().item())
    for name, (err, cpu, lo, hi) in worst.items():
        note(f"{what} {name}: {ngroups[name]} groups of bands within the rule; worst group (|x| in [{lo:.4g}, {hi:.4g}]): device vs float64 {err:.3e}, fp32 twin vs float64 {cpu:.3e}")


@pytest.mark.parametrize("Cs,B", [(3, 1), (5, 3), (8, 2)])
def test_decoder_tail_fp32_ladder(Cs, B):
    vals, band = R.tail_ladder_f32()
    x, hw = R.tail_input(vals, B, Cs, torch.float32)
    got = _tail_call(x, L.DS_F32, B, Cs, hw, off=B // 3)
    _tail_bands(f"ds_decoder_tail fp32 Cs={Cs} B={B}", vals, band, got, R.tail_twin(x), R.tail_ref64(x))


@pytest.mark.parametrize("Cs,B", [(3, 1), (5, 3), (8, 2)])
def test_decoder_tail_bf16_every_value(Cs, B):
    vals, band = R.tail_values_bf16()
    x, hw = R.tail_input(vals, B, Cs, torch.bfloat16)
    got = _tail_call(x, L.DS_BF16, B, Cs, hw, off=B // 3)
    _tail_bands(f"ds_decoder_tail bf16 Cs={Cs} B={B}", vals, band, got, R.tail_twin(x), R.tail_ref64(x))


def test_decoder_tail_second_grid_pass():
    B, HW = R.TAIL_BIG
    assert B * HW > R.TAIL_GRID
    x = torch.randn(B, HW, 3, generator=torch.Generator().manual_seed(21)) * 3.0
    got = _tail_call(x, L.DS_F32, B, 3, HW)
    twin, f64 = R.tail_twin(x), R.tail_ref64(x)
    rule("ds_decoder_tail fp32 Cs=3, 8192 x 256 + 2048 pixels", got, twin, f64)
    k = R.TAIL_GRID - HW                                                     # the second pass: pixels TAIL_GRID .. of sample 1
    rule("ds_decoder_tail second grid pass alone", got[1, :, k:], twin[1, :, k:], f64[1, :, k:])


# ================================================================================================= ds_istft_plus
def _istft_call(enc, B, T, hop, off=0, loop=False):
    e = S.slab(enc, offset_floats=off)
    nws = L.load().ds_istft_ws_floats(B, 512, T)
    assert nws == B * T * 1024
    ws = S.nan_slab((B, T, 1024))
    Lr = hop * T if loop else hop * (T - 1)
    audio = S.nan_slab((B, Lr), offset_floats=off)
    L.call("ds_istft_plus_loop" if loop else "ds_istft_plus", e.data_ptr(), B, 512, T, hop, ws.data_ptr(), audio.data_ptr(), L.current_stream())
    sync()
    S.check_guards(e, ws, audio)
    unchanged(e, enc)
    assert (e.data_ptr() % 16 == 0) == (off == 0)
    return ws.cpu(), audio.cpu()


@pytest.mark.parametrize("B", R.ISTFT_B)
@pytest.mark.parametrize("T,hop", R.ISTFT_SHAPES)
def test_istft_frames_and_overlap_add_apart(T, hop, B):
    enc = R.istft_input(B, T)
    ws, audio = _istft_call(enc, B, T, hop)
    tag = f"ds_istft_plus T={T} hop={hop} B={B}"
    tw = R.frames_twin(enc.numpy())
    rule(tag + " frames (ws)", ws, tw, R.frames_ref64(enc.numpy()))
    rule(tag + " overlap-add of the device's frames", audio, R.ola(ws.numpy(), hop, np.float32), R.ola(ws.numpy(), hop, np.float64))
    rule(tag + " audio vs the oracle", audio, R.ola(tw, hop, np.float32), R.istft_ref64(enc.numpy(), hop))


def test_istft_misaligned_view_has_the_bits_of_the_aligned_run():
    enc = R.istft_input(3, 8)
    ws0, a0 = _istft_call(enc, 3, 8, 128)
    ws1, a1 = _istft_call(enc, 3, 8, 128, off=1)
    assert torch.equal(bits(ws0), bits(ws1)) and torch.equal(bits(a0), bits(a1))


@pytest.mark.parametrize("T,hop", R.ISTFT_LOOP_SHAPES)
def test_istft_loop_smallest_periods(T, hop):
    assert T == 1024 // hop
    enc = R.istft_input(3, T)
    ws, audio = _istft_call(enc, 3, T, hop, loop=True)
    tw = R.frames_twin(enc.numpy())
    tag = f"ds_istft_plus_loop T={T} hop={hop}"
    rule(tag + " frames (ws)", ws, tw, R.frames_ref64(enc.numpy()))
    rule(tag + " audio vs the circular restatement", audio, R.ola_loop(tw, hop, np.float32), R.istft_loop_ref64(enc.numpy(), hop))
    _, rolled = _istft_call(torch.roll(enc, 1, dims=-1).contiguous(), 3, T, hop, loop=True)
    assert torch.equal(bits(rolled), bits(torch.roll(audio, hop, dims=-1)))


# ================================================================================================= ds_stft_plus
def _stft_call(audio, hop, reflect, T_out, off=0):
    B, Ln = audio.shape
    a = S.slab(audio, offset_floats=off)
    enc = S.nan_slab((B, 3, 512, T_out), offset_floats=off)
    L.call("ds_stft_plus", a.data_ptr(), B, Ln, hop, int(reflect), T_out, enc.data_ptr(), L.current_stream())
    sync()
    S.check_guards(a, enc)
    unchanged(a, audio)
    return enc.cpu()


def _check_padding_and_norm(what, enc, T):
    pad = enc[..., T:]
    want = torch.tensor([0.0, 1.0, 0.0]).view(1, 3, 1, 1).expand_as(pad)
    assert torch.equal(bits(pad), bits(want.contiguous())), what + ": columns past T are not exactly (0, 1, 0)"
    e = enc[..., :T].double()
    live = e[:, 0] > 0
    dev = (e[:, 1] ** 2 + e[:, 2] ** 2 - 1).abs()
    worst = dev[live].max().item() if bool(live.any()) else 0.0
    assert worst <= R.UNIT_NORM_BOUND, (what, worst, R.UNIT_NORM_BOUND)
    dead = ~live
    assert bool((e[:, 1][dead] == 1).all()) and bool((e[:, 2][dead] == 0).all()), what + ": a bin of magnitude 0 is not (0, 1, 0)"
    return worst


@pytest.mark.parametrize("Ln,hop,pads", R.STFT_CASES, ids=["L%d_hop%d" % (a, b) for a, b, _ in R.STFT_CASES])
def test_stft_plus_every_bin(Ln, hop, pads):
    T = 1 + Ln // hop
    for pad in pads:
        reflect = pad == "reflect"
        for k, (extra, B) in enumerate(R.STFT_TOUT_B):
            audio = R.stft_audio(B, Ln)
            enc = _stft_call(audio, hop, reflect, T + extra, off=k % 2)
            tag = f"ds_stft_plus L={Ln} hop={hop} {pad} B={B} T_out=T+{extra}"
            worst = _check_padding_and_norm(tag, enc, T)
            ref = R.stft_ref64(audio.numpy(), hop, reflect)
            tw = R.stft_twin(audio.numpy(), hop, reflect)
            d, f = R.per_frame(R.spectrum_of(enc[..., :T].numpy()), ref)
            t, _ = R.per_frame(R.spectrum_of(tw), ref)
            rule(tag + " expm1(c0) (c1, c2) per bin / frame maximum", d, t, f)
            note(f"{tag}: worst |c1^2 + c2^2 - 1| = {worst / R.U:.3f} x 2^-24 (bound {R.UNIT_NORM_BOUND / R.U:.3f})")


def test_stft_plus_digital_silence():
    zero3 = torch.tensor([0.0, 1.0, 0.0]).view(1, 3, 1, 1)
    enc = _stft_call(torch.zeros(2, 1000), 256, False, 6)
    assert torch.equal(bits(enc), bits(zero3.expand_as(enc).contiguous()))
    audio = R.stft_audio(3, 1000).clone()
    audio[1] = 0.0
    for reflect in (False, True):
        enc = _stft_call(audio, 256, reflect, 4)
        assert torch.equal(bits(enc[1]), bits(zero3[0].expand_as(enc[1]).contiguous()))
        assert bool((enc[0, 0] > 0).any()) and bool((enc[2, 0] > 0).any())


@pytest.mark.parametrize("power", [-70, 100])
@pytest.mark.parametrize("Ln,hop,reflect", [(2560, 256, False), (1000, 256, True)])
def test_stft_plus_quiet_signal_keeps_its_phase(Ln, hop, reflect, power):
    """The same audio times 2^-70 (and times 2^100, where the squares of a bin overflow instead): the transform is linear, the scale a power of two and nothing in between is denormal, so (c1, c2) are
    bit-equal to the unscaled run's, c0 is log1pf of the scaled magnitude, and the unit-norm bound holds.  Before stft_plus_encode
    scaled the pair by a power of two ahead of its squares (bins of 1e-19 .. 1e-23: denormal or zero squares) this failed: at L = 2560,
    32 528 of 33 792 phase values differed from the unscaled run's, by up to 3.6e-2, |c1^2 + c2^2 - 1| reached 0.082; at L = 1000
    (reflect) 11 784 of 12 288 differed, by up to 2.0 (a pair of (-1, 0) collapsed to (1, 0)), |c1^2 + c2^2 - 1| reached 0.18."""
    audio = R.stft_audio(3, Ln)
    quiet = (audio.double() * 2.0 ** power).float()
    assert torch.equal(quiet.double() * 2.0 ** -power, audio.double())
    T = 1 + Ln // hop
    loud, soft = _stft_call(audio, hop, reflect, T), _stft_call(quiet, hop, reflect, T)
    tag = f"ds_stft_plus signal x 2^{power} L={Ln} hop={hop} reflect={reflect}"
    diff = (bits(loud[:, 1:]) != bits(soft[:, 1:]))
    n2 = (soft[:, 1].double() ** 2 + soft[:, 2].double() ** 2 - 1).abs().max().item()
    note(f"{tag}: {int(diff.sum())} of {diff.numel()} phase values differ in bits from the unscaled run; worst |c1^2 + c2^2 - 1| = {n2 / R.U:.4g} x 2^-24; "
         f"largest |c1, c2 difference| = {(loud[:, 1:].double() - soft[:, 1:].double()).abs().max().item():.3e}")
    _check_padding_and_norm(tag, soft, T)
    E.assert_bits_equal(soft[:, 1:], loud[:, 1:], tag + " (c1, c2) against the unscaled run")
    assert bool(torch.isfinite(soft).all())
    if power < 0:
        # c0 = log1pf(mag) = mag at 1e-19 (times 2^70: out of reach of rel_err's floor of 1e-30) against the float64 magnitude, by the rule,
        # with the twin run on the same scaled audio.  (Not at 2^100: the logarithm of a large magnitude turns every weak bin's RELATIVE
        # error into an absolute one, which is no quantity of one scale for the rule to weigh.)
        ref = np.abs(R.stft_ref64(quiet.numpy(), hop, reflect))
        tw = R.stft_twin(quiet.numpy(), hop, reflect)
        up = 2.0 ** -power
        rule(tag + f" c0 x 2^{-power}", soft[:, 0].double() * up, torch.from_numpy(tw[:, 0]).double() * up, torch.from_numpy(np.log1p(ref) * up))


# ================================================================================================= host-side refusals
def test_host_side_refusals():
    """Each returns the library's error before anything is launched: the NaN-filled outputs stay untouched."""
    lib, st = L.load(), L.current_stream()
    c = R.vq_data("ties", 16)
    z, cb, esq = S.slab(torch.zeros(1, 3, 16)), S.slab(c.cb.float()), S.slab(c.esq.float())
    q = S.nan_slab((1, 3, 16))
    raw, idx = idx_slab(16)
    enc = S.slab(R.istft_input(1, 4))
    ws, audio = S.nan_slab((4 * 1024,)), S.nan_slab((4 * 1024,))
    sig = S.slab(R.stft_audio(1, 1000)[:, :512].contiguous())
    out = S.nan_slab((1, 3, 512, 8))
    calls = (("ds_vq_nearest", (z.data_ptr(), cb.data_ptr(), esq.data_ptr(), 1, 3, 16, 16, q.data_ptr(), idx.data_ptr(), st), "embedding_dim"),
             ("ds_istft_plus", (enc.data_ptr(), 1, 512, 4, 100, ws.data_ptr(), audio.data_ptr(), st), "hop"),
             ("ds_istft_plus", (enc.data_ptr(), 1, 256, 4, 256, ws.data_ptr(), audio.data_ptr(), st), "n_fft"),
             ("ds_istft_plus", (enc.data_ptr(), 1, 512, 1, 256, ws.data_ptr(), audio.data_ptr(), st), "bad args"),
             ("ds_stft_plus", (sig.data_ptr(), 1, 512, 256, 0, 2, out.data_ptr(), st), "T_out"),
             ("ds_stft_plus", (sig.data_ptr(), 1, 512, 256, 1, 8, out.data_ptr(), st), "reflect"))
    for name, args, word in calls:
        assert getattr(lib, name)(*args) != 0, name
        with pytest.raises(L.DsError, match=word):
            L.call(name, *args)
    sync()
    nan32 = lambda t: bool((bits(t) == 0x7FC00000).all())                                                  # noqa: E731
    assert nan32(q) and nan32(raw) and nan32(ws) and nan32(audio) and nan32(out)
    S.check_guards(z, cb, esq, q, raw, enc, ws, audio, sig, out)
