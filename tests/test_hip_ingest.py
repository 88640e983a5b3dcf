"""The ingest path on the GPU (diffusynth_amd/ingest.py, ds_resample_poly) against its float64 restatement (tests/ingest_ref.py, pinned to
scipy.signal.resample_poly in tests/test_ingest_cpu.py).

Tolerance rule: that of tests/test_hip_arranger.py, unchanged — the device gets 8 x the error of the float32 twin against the float64 form,
never less than 2e-6 and never more than 1e-3, through conftest.rel_err (max-norm and rms both held).  Figure and bound are printed.
Outputs are pre-filled with NaN wherever the test owns the buffer; the package's own buffers are checked for NaN instead.
"""
import functools

import numpy as np
import pytest
import torch

import ingest_ref as R
from conftest import rel_err, rel_errs
from diffusynth_amd import _lib as L
from diffusynth_amd import ingest as G

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 160, 441, 442, 1000, 3001, 7777)
RATES = ((44100, 16000), (48000, 16000), (8000, 16000), (11025, 16000), (22050, 16000), (16000, 48000), (16000, 44100), (8000, 16000))
# per signal: longer than NRES, shorter, equal, ... (NRES = 1, 1, 320, 640, 321, 3000, 8272, 15554)
TARGETS = (5, 1, 200, 1500, 321, 2048, 8272, 20000)


def bound(twin, want):
    """8 x the twin's error, inside [2e-6, 1e-3]."""
    return min(max(8.0 * max(rel_errs(twin, want)), 2e-6), 1e-3)


def check(got, want, twin, what):
    err, tol = rel_err(got, want), bound(twin, want)
    print(f"{what}: device {err:.2e}, twin {max(rel_errs(twin, want)):.2e}, bound {tol:.2e}")
    assert err < tol, (what, err, tol)


@functools.lru_cache(maxsize=None)
def signal(i):
    return R.probe_signal(LENGTHS[i], seed=40 + i)


@functools.lru_cache(maxsize=None)
def reference(i, f32):
    """The restatement of signal i at its rate pair (computed once per session; callers do not write to it)."""
    up, down, _ = R.rate_pair(*RATES[i])
    return R.resample(signal(i), up, down, np.float32 if f32 else np.float64)


def device_signals():
    return [torch.from_numpy(signal(i)).cuda() for i in range(len(LENGTHS))]


def raw_launch(sigs, rates, targets):
    """ds_resample_poly on an output buffer the test owns, pre-filled with NaN, with a guard of 64 floats on either side."""
    bank = G.filter_bank("cuda")
    p = G._Plan([len(s) for s in sigs], [a for a, _ in rates], [b for _, b in rates], targets, bank)
    assert not p.same
    tab = p.tab.copy()
    tab[:, L.RP["DS_RP_OOFF"]] += 64
    x = torch.from_numpy(np.concatenate(sigs)).cuda()
    out = torch.full((p.total_out + 128,), float("nan"), device="cuda")
    dtab, filt = torch.from_numpy(tab.reshape(-1)).cuda(), bank.device(torch.device("cuda"))       # (named: both must outlive the launch)
    L.call("ds_resample_poly", x.data_ptr(), dtab.data_ptr(), filt.data_ptr(), len(p.rows),
           p.max_blocks, p.max_taps, p.span, p.total_in, p.total_out + 128, bank.total, out.data_ptr(), L.current_stream())
    host = out.cpu().numpy()
    assert np.isnan(host[:64]).all() and np.isnan(host[-64:]).all()           # nothing outside the rows is written
    return [host[64 + o:64 + o + n] for o, n in zip(p.ooff, p.olen)], p


# ---------------------------------------------------------------------------------------------------- 1. parity of a ragged batch
def test_ragged_batch_matches_the_restatement():
    outs, p = raw_launch([signal(i) for i in range(8)], RATES, None)           # one launch, eight rate pairs, NaN pre-fill
    assert p.max_blocks > 1 and len(p.rows) == 8
    for i, o in enumerate(outs):
        want = reference(i, False)
        assert o.dtype == np.float32 and o.shape == want.shape and not np.isnan(o).any()
        check(o, want, reference(i, True), f"resample_poly[{i}] {RATES[i][0]} -> {RATES[i][1]}, N = {LENGTHS[i]}")
    pub = G.resample_poly(device_signals(), [a for a, _ in RATES], [b for _, b in RATES])      # the public call: the same launch
    for i, o in enumerate(pub):
        assert o.dtype == torch.float32 and np.array_equal(o.cpu().numpy(), outs[i]), i


def test_ragged_batch_with_targets_longer_and_shorter_than_nres():
    outs, p = raw_launch([signal(i) for i in range(8)], RATES, list(TARGETS))
    for i, (o, nres) in enumerate(zip(outs, p.nres)):
        want = R.fix_length(reference(i, False), TARGETS[i])
        twin = R.fix_length(reference(i, True), TARGETS[i])
        assert len(o) == TARGETS[i] and nres == len(reference(i, False))                    # exact output lengths
        assert not np.isnan(o).any()                                                       # every element of the row is written
        assert not o[nres:].any() and not np.signbit(o[nres:]).any()                       # exact zeros past NRES
        check(o, want, twin, f"fit[{i}] {RATES[i][0]} -> {RATES[i][1]}, N = {LENGTHS[i]}, NRES = {nres}, OLEN = {TARGETS[i]}")
    assert {int(np.sign(t - len(reference(i, False)))) for i, t in enumerate(TARGETS)} == {-1, 0, 1}     # longer, equal and shorter in ONE batch
    pub = G.resample_poly(device_signals(), [a for a, _ in RATES], [b for _, b in RATES], lengths=list(TARGETS))
    for i, o in enumerate(pub):
        assert o.shape == (TARGETS[i],) and np.array_equal(o.cpu().numpy(), outs[i]), i


def test_the_tensor_form():
    same = G.resample_poly(torch.from_numpy(np.stack([signal(5), signal(5)])).cuda(), 16000, 48000)          # (B, L) form
    assert same.shape == (2, 3000) and torch.equal(same[0], same[1])
    check(same[0].cpu(), reference(5, False), reference(5, True), "(B, L) form")


# ---------------------------------------------------------------------------------------------------- 2. alignment, exactly
@pytest.mark.parametrize("orig,target", [(44100, 16000), (16000, 44100)])
def test_an_impulse_returns_the_taps_bit_for_bit(orig, target):
    up, down, half = G.rate_pair(orig, target)
    h = G.filter_bank("cuda").taps(up, down)
    n = 700
    nres = R.resampled_length(n, up, down)
    pos = (0, 1, n - 1)
    x = np.zeros((3, n), np.float32)
    for row, n0 in enumerate(pos):
        x[row, n0] = 1.0
    outs, p = raw_launch(list(x), [(orig, target)] * 3, None)
    m = np.arange(nres, dtype=np.int64)
    hits = 0
    for n0, o in zip(pos, outs):
        k = half + m * down - n0 * up
        ok = (k >= 0) & (k <= 2 * half)
        want = np.zeros(nres, np.float32)
        want[ok] = h[k[ok]]
        assert o.shape == want.shape and np.array_equal(o.view(np.uint32), want.view(np.uint32)), (orig, target, n0)   # the fp32 taps, 0 outside
        hits += int(ok.sum())
    assert hits >= 30                                                          # (the three impulses do reach the output)


# ---------------------------------------------------------------------------------------------------- 3. independence
def test_a_signal_alone_equals_its_slice_of_the_batch_and_runs_repeat():
    sigs = device_signals()
    srs, trs = [a for a, _ in RATES], [b for _, b in RATES]
    a = G.resample_poly(sigs, srs, trs)
    b = G.resample_poly(sigs, srs, trs)
    for i in range(8):
        assert torch.equal(a[i], b[i]), i                                         # no atomics: two runs are bit-equal
        assert torch.equal(a[i], G.resample_poly([sigs[i]], srs[i], trs[i])[0]), i    # what shares the launch does not matter


# ---------------------------------------------------------------------------------------------------- 4. equal rates
def test_equal_rates_return_the_input_bits():
    x = torch.from_numpy(signal(5)).cuda()
    y = torch.from_numpy(signal(3)).cuda()
    same, other, short, long_ = G.resample_poly([x, y, x, x], [16000, 44100, 16000, 16000], 16000, lengths=[1000, 160, 300, 1500])
    assert torch.equal(same, x) and torch.equal(short, x[:300])
    assert torch.equal(long_[:1000], x) and long_.shape == (1500,) and not long_[1000:].any()
    assert torch.equal(other, G.resample_poly([y], 44100, 16000)[0])
    alone = G.resample_poly([x], 16000, 16000)                                     # nothing to launch at all
    assert torch.equal(alone[0], x) and alone[0].data_ptr() != x.data_ptr()


# ---------------------------------------------------------------------------------------------------- 5. adjust_audio_length
def test_adjust_audio_length_is_resample_poly_with_one_signal():
    x = torch.from_numpy(signal(6)).cuda()
    for n, orig in ((5000, 44100), (100, 48000), (3001, 16000), (4000, 16000)):
        got = G.adjust_audio_length(x, n, orig, 16000)
        assert got.shape == (n,) and torch.equal(got, G.resample_poly([x], orig, 16000, lengths=n)[0])
    with pytest.raises(ValueError, match="mono"):
        G.adjust_audio_length(torch.zeros(2, 100, device="cuda"), 50, 44100, 16000)
    with pytest.raises(ValueError, match="15999"):
        G.adjust_audio_length(x, 50, 15999, 16000)


# ---------------------------------------------------------------------------------------------------- 6. uploads_to_stft
@pytest.fixture(scope="module")
def vae(vqgan_sd):
    from diffusynth_amd.vqgan import PRODUCTION_CONFIG, VQGAN
    m = VQGAN(**PRODUCTION_CONFIG)
    m.load_state_dict(vqgan_sd)
    return m.to("cuda")


@functools.lru_cache(maxsize=None)
def uploads():
    a = np.round(R.probe_signal(13230, 1).astype(np.float64) * 30000).astype(np.int16)
    b = R.probe_signal(48000, 2).astype(np.float64) * 0.37
    c = R.probe_signal(5000, 3)
    return ((44100, a), (48000, b), (16000, c))


@pytest.mark.parametrize("duration", [1, 2.2])
def test_uploads_to_stft(vae, duration):
    from diffusynth_amd.vocoder import InputBatch2Encode_STFT, audio_to_stft_representation
    ups = [(sr, s if i != 1 else torch.from_numpy(s)) for i, (sr, s) in enumerate(uploads())]       # numpy int16, a float64 tensor, numpy fp32
    enc, audio = G.uploads_to_stft(ups, duration, time_resolution=48)
    n = R.upload_length(duration, 48)
    assert audio.shape == (3, n) and audio.dtype == torch.float32 and audio.is_cuda and not torch.isnan(audio).any()
    want = R.ingest(uploads(), duration, time_resolution=48)
    twin = R.ingest(uploads(), duration, time_resolution=48, dtype=np.float32)
    for i in range(3):
        check(audio[i].cpu(), want[i], twin[i], f"uploads_to_stft audio[{i}] {uploads()[i][0]} Hz, duration {duration}")
    assert enc.shape == (3, 3, 512, 48) and torch.equal(enc, audio_to_stft_representation(audio, 48))
    out = InputBatch2Encode_STFT(vae._encoder, enc, quantizer=vae._vq_vae)
    assert out[3].shape == (3, 4, 128, 12) and out[4].shape == (3, 4, 128, 12)
    with pytest.raises(ValueError, match="mono"):
        G.uploads_to_stft(ups + [(44100, np.zeros((1000, 2), np.int16))], duration, time_resolution=48)


def test_uploads_accept_device_tensors():
    ups = [(sr, torch.as_tensor(s).cuda()) for sr, s in uploads()]
    enc, audio = G.uploads_to_stft(ups, 1, time_resolution=48)
    enc2, audio2 = G.uploads_to_stft(list(uploads()), 1, time_resolution=48)
    assert torch.equal(audio, audio2) and torch.equal(enc, enc2)
