"""The inputs of tests/test_hip_codec_kernels.py can tell a faulty kernel from a right one (no GPU needed).

Every case of tests/codec_ref.py is built again here, which asserts its preconditions (the exactness margin, the emulated split-precision
distances equal to float64, the shares of operands that need a second and a third bf16 part, the share of tied minima); every twin is held
to its rule (the quantiser's fp32 emulation to the derived near-tie bound, the encode twin to the unit-norm bound, every other twin to a
distance from float64 that an fp32 evaluation can have: below the one a defect model causes, by the factor the GPU test allows and ten
more); and every defect model changes the tensor the GPU test compares: on exact data the expected tensor differs, on tolerance data the
result moves by at least ten times the allowance (four times the twin's distance)."""
import numpy as np
import pytest
import torch

import codec_ref as R
import exact_ref as E
from conftest import rel_errs
from oracle import vocoder_ref as V


def rel_err(a, b):
    """Both error norms of the suite, the larger one — without conftest.rel_err's log: the figures here are deliberate faults, not parity."""
    return max(rel_errs(torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b))))


# a sanity ceiling for the transform twins, not a tolerance of any GPU test: ten radix-2 levels (five radix-4 passes), an ulp each
FFT_TWIN_CEILING = 10 * 2.0 ** -23


def shows(mutant, twin, f64):
    """A defect on tolerance data: at least ten times the GPU test's allowance away from float64."""
    return rel_err(mutant, f64) >= 10 * 4 * rel_err(twin, f64)


# ================================================================================================= ds_vq_nearest
VQ_ALL = [(k, n) for k in R.VQ_SETS for n in R.VQ_NCODES + R.VQ_NCODES_SCALAR]


@pytest.mark.parametrize("kind,ncodes", VQ_ALL)
def test_vq_case_and_its_defect_models(kind, ncodes):
    c = R.vq_data(kind, ncodes)
    print(f"{kind} ncodes={ncodes}: margin {c.margin:.4g} < 2^24, tied {c.tied.double().mean().item():.3f}, part shares {c.shares}")
    # the preconditions, stated again from the case's tensors
    for t in (c.z, c.cb, c.esq):
        assert E.is_f32(t) and torch.equal(t, t.round())
    assert (c.esq.abs()[None] + 2 * (c.z.abs() @ c.cb.abs().T)).max().item() < 2 ** 24
    assert c.z.shape == (R.VQ_POOL, 4) and R.VQ_POOL == max(b * hw for b, hw in R.VQ_BHW) and bool((c.z[0] == 0).all())
    d = c.esq[None] - 2 * (c.z @ c.cb.T)
    assert torch.equal(R.vq_dist_parts(c.z, c.cb, c.esq), d)
    # the fp32 slot-by-slot emulation is exact too, and so is the scalar kernel's form where |z|^2 fits
    assert torch.equal(R.vq_twin_f32(c.z.float(), c.cb.float(), c.esq.float()).double(), d)
    if c.scalar_exact:
        zf, cf = c.z.float(), c.cb.float()
        zz = (zf * zf).sum(1, keepdim=True)
        dot = torch.zeros(zf.shape[0], cf.shape[0])
        for k in range(4):
            dot = dot + zf[:, k:k + 1] * cf[:, k][None]
        assert torch.equal(((zz + c.esq.float()[None]) - 2.0 * dot).double(), d + (c.z * c.z).sum(1, keepdim=True))
    else:
        assert kind == "zlow"
    assert torch.equal(c.idx, d.argmin(1)) or ncodes > 1                   # (first_min is the definition; torch.argmin agrees where it is unique)
    assert bool((d[torch.arange(R.VQ_POOL), c.idx] == d.min(1).values).all())
    assert bool((d[:, :1] > d.min(1, keepdim=True).values).logical_or(c.idx[:, None] == 0).all())
    if kind == "ties" and ncodes >= 2:
        assert c.tied.double().mean().item() >= 0.25
    if kind == "mid":
        assert c.shares["z2"] >= 0.25 and c.shares["e2"] >= 0.25
    if kind == "zlow":
        assert c.shares["z3"] >= 0.25
    if kind == "elow":
        assert c.shares["e3"] >= 0.25 and c.shares["q3"] >= 0.25
    ntiles = (ncodes + 15) // 16
    if ntiles >= 2 and ncodes <= 8192:
        # the last code tile holds copies of earlier codes only: examining it again must change nothing
        for j in range(16 * (ntiles - 1), ncodes):
            assert bool((c.cb[:16 * (ntiles - 1)] == c.cb[j]).all(1).any()) or kind in ("zlow", "elow")
    # q on integers is the code itself
    assert torch.equal(R.vq_q(c.z, c.cb, c.idx).double(), c.cb[c.idx])
    for kind_m in R.VQ_MUTANTS:
        m = R.vq_mutant(c, kind_m)
        if ncodes > 8192:
            assert m is None
        elif m is not None and ncodes >= 100 and R.VQ_MUTANT_SET.get(kind_m, kind) == kind and not (kind_m == "groups_no_index" and kind == "elow"):
            assert not torch.equal(m, c.idx), kind_m


def test_every_vq_defect_model_shows():
    """Each defect model changes the expected indices in a case the GPU test runs, the dropped-part ones on the data set built for them, the
    B-half one inside the first 128 pixels' second half only, the padding one at pixel 0."""
    for kind_m in R.VQ_MUTANTS:
        kind = R.VQ_MUTANT_SET.get(kind_m, "ties")
        seen = {}
        for n in R.VQ_NCODES:
            c = R.vq_data(kind, n)
            m = R.vq_mutant(c, kind_m)
            if m is not None:
                seen[n] = int((m != c.idx).sum())
        print(kind_m, "on", kind, seen)
        assert sum(v > 0 for v in seen.values()) >= 3, (kind_m, seen)
    c = R.vq_data("ties", 100)
    m = R.vq_mutant(c, "b_half_tile")
    i = torch.arange(R.VQ_POOL)
    assert bool((m == c.idx)[i % 128 < 64].all()) and bool((m != c.idx)[i % 128 >= 64].any())
    assert R.vq_mutant(c, "padding_wins")[0].item() == 100 and R.vq_mutant(R.vq_data("ties", 64), "padding_wins") is None
    # the share of argmins the code-side third part decides on `elow` at the production size
    c = R.vq_data("elow", 8192)
    flipped = (R.vq_mutant(c, "cb_third") != c.idx).double().mean().item()
    print(f"elow 8192: {flipped:.3f} of the argmins change without the code side's third part")
    assert flipped >= 0.25


def test_vq_placed_ties():
    c = R.vq_placed_ties()
    assert len(c.placed) == 128
    tiles = {(p // 128, (p % 128) // 16) for p in c.placed}
    assert tiles == {(w, t) for w in range(4) for t in range(8)}
    (a0, b0), (a1, b1), (a2, b2), (a3, b3) = R.VQ_PLACED_PAIRS
    lane = lambda j: (j // 16, (j % 16) // 4, j % 4)                                                      # noqa: E731  (tile, lane group, r)
    assert lane(a0)[:2] == lane(b0)[:2] and lane(a0)[2] != lane(b0)[2]
    assert lane(a1)[0] == lane(b1)[0] and lane(a1)[1] != lane(b1)[1]
    assert a2 // 64 == b2 // 64 and a2 // 16 != b2 // 16 and lane(a2)[1] > lane(b2)[1]
    assert a3 // 16 == 0 and b3 // 16 == 511
    for kind_m in ("last_index", "groups_no_index", "b_half_tile"):
        assert not torch.equal(R.vq_mutant(c, kind_m), c.idx), kind_m
    m = R.vq_mutant(c, "last_index")
    assert all(m[p].item() == b for p, (a, b) in c.placed.items())
    m = R.vq_mutant(c, "groups_no_index")
    assert any(m[p].item() == b for p, (a, b) in c.placed.items())


@pytest.mark.parametrize("book,zscale", R.VQ_FLOAT)
def test_vq_float_twin_is_within_the_derived_bound(book, zscale):
    c = R.vq_float_case(book, zscale)
    tw = R.vq_twin_f32(c.z, c.cb, c.esq)
    # distance by distance: the emulation's error against float64 within half the two-distance bound
    d64, s = R.vq_dist64(c.z, c.cb, c.esq), R.vq_bound(c.z, c.cb, c.esq)
    ratio = ((tw.double() - d64).abs() / (0.5 * R.VQ_C * R.U * s)).max().item()
    idx = R.first_min(tw.double())[0]
    excess, allow, ref = R.vq_excess(c.z, c.cb, c.esq, idx)
    print(f"{book} x {zscale}: worst |twin - float64| = {ratio:.4f} of 33 u S; {int((idx != ref).sum())} indices differ, worst excess {(excess / allow).max().item():.4f}")
    assert ratio <= 1.0 and bool((excess <= allow).all())
    # distances from a pixel side that lost its second and third part are outside the bound
    bad = R.vq_twin_f32(R.bf(c.z.double()).float(), c.cb, c.esq)
    assert ((bad.double() - d64).abs() / (0.5 * R.VQ_C * R.U * s)).max().item() > 1.0


# ================================================================================================= ds_vq_stats
@pytest.mark.parametrize("case", R.VQS_CASES)
def test_vq_stats_case_and_its_defect_models(case):
    c = R.vqs_case(*case)
    assert E.is_f32(c.z) and E.is_f32(c.q) and ((c.q - c.z) ** 2).sum(1).max().item() < 2 ** 24
    mse, loss, p32, p64 = R.vqs_expect(c, 0.25, 1)
    mse2, loss2, _, _ = R.vqs_expect(c, 0.4, 0)
    assert mse.dtype == torch.float32 and torch.equal(mse, mse2) and not torch.equal(loss, loss2)
    assert abs(mse.double().item() - ((c.q - c.z) ** 2).mean().item()) <= 2.0 ** -24 * mse.item()
    assert abs(p32.item() / p64.item() - 1) < 1e-5
    if c.usage == "one":
        assert p32.item() == 1.0 and p64.item() < 1.0
    if c.usage == "uniform":
        assert abs(p64.item() - 64) < 1e-6
    shown = {}
    before = R.vqs_case(c.D, c.B, c.HW, c.ncodes, "high" if c.usage != "high" else "skew")
    for kind in R.VQS_MUTANTS:
        m = R.vqs_expect(c, 0.25, 1, mutant=kind, before=before)
        shown[kind] = (not torch.equal(m[0], mse)) or abs(m[3].item() / p64.item() - 1) > 1e-3
    print(case, shown)
    assert shown["counts_kept"] or c.ncodes == 1
    assert shown["grid_one_trip"] == (c.npix > R.VQS_GRID)
    assert shown["outside_clamped"] == (c.usage == "outside")
    if c.usage == "high" and c.ncodes > 1024:
        assert shown["finish_one_trip"]


# ================================================================================================= ds_decoder_tail
def test_decoder_tail_values_twin_and_threshold():
    vals, band = R.tail_ladder_f32()
    assert vals.numel() == len(R.TAIL_LADDER) * (2 * R.TAIL_BAND + 1)
    assert float(np.nextafter(np.float32(20), np.float32(np.inf))) in R.TAIL_LADDER and bool((vals > 20).any()) and bool((vals == 20).any())
    vb, bb = R.tail_values_bf16()
    assert bool((vb.bfloat16().float() == vb).all()) and vb.abs().max().item() == 128 and len(torch.unique(vb)) == vb.numel() - 1      # (+0 and -0)
    for v, b, dt in ((vals, band, torch.float32), (vb, bb, torch.bfloat16)):
        for Cs, B in ((3, 1), (5, 3), (8, 2)):
            x, hw = R.tail_input(v, B, Cs, dt)
            assert x.shape == (B, hw, Cs) and bool(torch.isnan(x[..., 3:]).all()) and bool(torch.isfinite(x[..., :3]).all())
            tw, f = R.tail_twin(x), R.tail_ref64(x)
            assert tw.shape == (B, 3, hw) and bool(torch.isfinite(tw).all()) and bool(torch.isfinite(f).all())
        n = v.numel()
        flat = lambda t: t.permute(1, 0, 2).reshape(3, -1)[:, :n]                                         # noqa: E731
        twf, ff, nothr = flat(tw), flat(f), flat(R.tail_ref64(x, threshold=False))
        for rows in (slice(0, 1), slice(1, 3)):
            group = R.tail_groups(ff[rows], b, R.tail_anchor(v, b))
            for k in group.unique().tolist():
                m = group == k
                assert rel_err(twf[rows][:, m], ff[rows][:, m]) <= 2.0 ** -23        # an fp32 evaluation: within an ulp of the largest output
        # a softplus without its threshold overflows from 88.7 on (the ladder's 104 and 1e30): not finite
        if dt == torch.float32:
            assert not bool(torch.isfinite(nothr).all())
    # channels 3 up never reach the output: a kernel that read channel 3 for channel 2 would store NaN
    x, hw = R.tail_input(vals, 1, 5, torch.float32)
    assert not bool(torch.isfinite(torch.tanh(x[..., 3])).any())


# ================================================================================================= ds_istft_plus
@pytest.mark.parametrize("T,hop", R.ISTFT_SHAPES)
def test_istft_twin_and_defect_models(T, hop):
    assert 1024 % hop == 0 and T >= 2
    enc = R.istft_input(3, T).numpy()
    tw, f = R.frames_twin(enc), R.frames_ref64(enc)
    e_fr = rel_err(tw, f)
    a64 = R.istft_ref64(enc, hop)
    e_au = rel_err(R.ola(tw, hop, np.float32), a64)
    e_ola = rel_err(R.ola(tw, hop, np.float32), R.ola(tw, hop, np.float64))
    print(f"T={T} hop={hop}: frames twin {e_fr:.3e}, audio twin {e_au:.3e}, overlap-add twin on its own {e_ola:.3e}")
    assert 0 < e_fr < FFT_TWIN_CEILING
    # the float64 overlap-add of the float64 frames IS the oracle (same arithmetic, same order up to rounding)
    assert rel_err(R.ola(f, hop, np.float64), a64) < 1e-12
    # defect models: a spectrum without its conjugate half (the real part of a one-sided transform), a hop of 256 taken for granted
    onesided = f * 0.5
    onesided[..., 0] = f[..., 0]
    assert shows(onesided, tw, f)
    if hop != 256:
        assert shows(R.ola(tw, hop, np.float32, "hop256"), R.ola(tw, hop, np.float32), R.ola(tw, hop, np.float64))
    # frames and overlap-add are checked apart: a frame fault that the overlap-add's division hides from the audio norm still moves ws
    if T >= 4:
        broken = tw.copy()
        broken[:, 1, :16] = 0
        assert shows(broken, tw, f)


@pytest.mark.parametrize("T,hop", R.ISTFT_LOOP_SHAPES)
def test_istft_loop_twin(T, hop):
    assert T == 1024 // hop
    enc = R.istft_input(3, T).numpy()
    tw = R.frames_twin(enc)
    want = R.istft_loop_ref64(enc, hop)
    assert rel_err(R.ola_loop(R.frames_ref64(enc), hop, np.float64), want) < 1e-12
    assert 0 < rel_err(R.ola_loop(tw, hop, np.float32), want) < FFT_TWIN_CEILING
    rolled = R.ola_loop(R.frames_twin(np.roll(enc, 1, axis=-1)), hop, np.float32)
    assert np.array_equal(rolled, np.roll(R.ola_loop(tw, hop, np.float32), hop, axis=-1))


# ================================================================================================= ds_stft_plus
@pytest.mark.parametrize("Ln,hop,pads", R.STFT_CASES)
def test_stft_twin_and_defect_models(Ln, hop, pads):
    for pad in pads:
        reflect = pad == "reflect"
        assert not reflect or Ln > 512
        a = R.stft_audio(3, Ln).numpy()
        ref = R.stft_ref64(a, hop, reflect)
        T = 1 + Ln // hop
        assert ref.shape == (3, 512, T)
        # the float64 reference is the oracle's transform before its rounding to complex64
        v = np.stack([V.stft(s, hop_length=hop, pad_mode=pad) for s in a])[:, 1:]
        assert np.abs(v - ref).max() <= 2.0 ** -22 * np.abs(ref).max()
        tw = R.stft_twin(a, hop, reflect, T + 1)
        assert np.array_equal(tw[..., T], np.broadcast_to(np.array([0, 1, 0], np.float32)[None, :, None], (3, 3, 512)))
        tw = tw[..., :T]
        norm = np.abs(tw[:, 1].astype(np.float64) ** 2 + tw[:, 2].astype(np.float64) ** 2 - 1).max()
        assert norm <= R.UNIT_NORM_BOUND
        d, f = R.per_frame(R.spectrum_of(tw), ref)
        e = rel_err(d, f)
        print(f"L={Ln} hop={hop} {pad}: twin {e:.3e}, worst |c1^2 + c2^2 - 1| = {norm / R.U:.3f} u")
        assert 0 < e < FFT_TWIN_CEILING
        for kind in ("reflect_as_constant", "tail_wraps"):
            m, _ = R.per_frame(R.spectrum_of(R.stft_twin(a, hop, reflect, mutant=kind)), ref)
            if kind == "reflect_as_constant" and not reflect:
                assert torch.equal(m, d)
            elif kind == "tail_wraps" and reflect:
                pass                                                    # (the reflection folds the tail before the wrap is looked at)
            else:
                assert shows(m, d, f), kind
        # a wrong phase in ONE weak bin (|X| a thousandth of its frame's maximum or less) is seen: the comparison is per bin
        weak = np.abs(ref) <= 1e-3 * np.abs(ref).max(axis=1, keepdims=True)
        if weak.any():
            b, k, t = np.argwhere(weak)[0]
            bad = tw.copy()
            bad[b, 1, k, t], bad[b, 2, k, t] = -tw[b, 2, k, t], tw[b, 1, k, t]
            m, _ = R.per_frame(R.spectrum_of(bad), ref)
            assert rel_errs(m, f)[0] > 4 * e or np.abs(ref[b, k, t]) / np.abs(ref[b, :, t]).max() < 4 * e


@pytest.mark.parametrize("power", [-70, 100])
@pytest.mark.parametrize("Ln,hop,reflect", [(2560, 256, False), (1000, 256, True)])
def test_stft_quiet_signal_shows_an_encode_without_prescale(Ln, hop, reflect, power):
    """The audio times 2^-70 (2^100): the twin of the encode keeps every bit of (c1, c2); the same encode without the power-of-two prescale
    (squares of 1e-19 .. 1e-23 are denormal or zero, those of 1e30 infinite) loses them: pairs off unit length, (1, 0) or (0, 0)."""
    a = R.stft_audio(3, Ln)
    q = (a.double() * 2.0 ** power).float()
    assert torch.equal(q.double() * 2.0 ** -power, a.double())
    loud, soft = R.stft_twin(a.numpy(), hop, reflect), R.stft_twin(q.numpy(), hop, reflect)
    assert np.array_equal(loud[:, 1:].view(np.int32), soft[:, 1:].view(np.int32))
    if power < 0:
        up = 2.0 ** -power
        assert rel_err(soft[:, 0].astype(np.float64) * up, np.log1p(np.abs(R.stft_ref64(q.numpy(), hop, reflect))) * up) < FFT_TWIN_CEILING
    assert np.isfinite(soft).all()
    with np.errstate(over="ignore", invalid="ignore"):
        bad = R.stft_twin(q.numpy(), hop, reflect, mutant="encode_unscaled")
    differ = int((bad[:, 1:].view(np.int32) != loud[:, 1:].view(np.int32)).sum())
    norm = np.nanmax(np.abs(bad[:, 1].astype(np.float64) ** 2 + bad[:, 2].astype(np.float64) ** 2 - 1))
    print(f"L={Ln} x 2^{power}: without the prescale {differ} of {bad[:, 1:].size} phase values change, worst |c1^2 + c2^2 - 1| = {norm:.3e}")
    assert differ > 0 and norm > R.UNIT_NORM_BOUND
    # on the audio as it is the two encodes agree bit for bit: the prescale keeps the bits of normal-range inputs
    assert np.array_equal(R.stft_twin(a.numpy(), hop, reflect, mutant="encode_unscaled").view(np.int32), loud.view(np.int32))


def test_unit_norm_bound_on_random_pairs():
    g = np.random.default_rng(5)
    xr = (g.standard_normal(200000) * np.exp(g.uniform(-40, 40, 200000))).astype(np.float32)
    xi = (g.standard_normal(200000) * np.exp(g.uniform(-40, 40, 200000))).astype(np.float32)
    _, c1, c2 = R.encode_twin(xr, xi)
    worst = np.abs(c1.astype(np.float64) ** 2 + c2.astype(np.float64) ** 2 - 1).max()
    print(f"worst |c1^2 + c2^2 - 1| over 200 000 pairs of 1e-17 .. 1e17: {worst / R.U:.3f} u (bound {R.UNIT_NORM_BOUND / R.U:.3f} u)")
    assert worst <= R.UNIT_NORM_BOUND
