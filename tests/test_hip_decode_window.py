"""Windowed decoding on the GPU: ds_stft_window_merge on synthetic windows and ds_istft_plus_loop against the float64 restatements
(tests/decode_window_ref.py), WindowedDecoder / WindowedEncoder on the production VQGAN (synthetic weights) against the restatement fed
with the same decoder output, locality, the seam of a loop, and the audio helpers on the wrapper."""
import ctypes

import numpy as np
import pytest
import torch

import decode_window_ref as D
import window_ref as R
from conftest import rel_err
from diffusynth_amd import _lib as L
from diffusynth_amd.synth import synth_input
from diffusynth_amd.windowed import WindowedDecoder, WindowedEncoder
from oracle import vocoder_ref as V

pytestmark = pytest.mark.gpu

MAXM = L.WM["DS_WM_MAXM"]
# frame plans (T, w, stride, loop): 16-byte pieces (T = 40, 32), the scalar kernel (T = 43, 42), four entries, the 16-byte kernel on
# offsets that are no multiple of 4 (T = 44, stride 6), and two loops
PLANS = [(40, 16, 8, False), (43, 16, 8, False), (32, 16, 4, False), (44, 16, 6, False), (40, 16, 8, True), (42, 16, 12, True)]
Rk = 2


# ------------------------------------------------------------------------------------------------ ds_stft_window_merge
def _tables(entries, T):
    wcol = np.zeros((MAXM, T, L.WM["DS_WM_NI"]), dtype=np.int32)
    wcol[:, :, L.WM["DS_WM_WIN"]] = -1
    wcoef = np.zeros((MAXM, T), dtype=np.float32)
    for x, ent in enumerate(entries):
        for m, (j, c, f) in enumerate(ent):
            wcol[m, x, L.WM["DS_WM_WIN"]], wcol[m, x, L.WM["DS_WM_COL"]], wcoef[m, x] = j, c, f
    return wcol, wcoef


def _merge(encw, out, erow, wcol, wcoef, R_, n):
    et, ct, ft = torch.from_numpy(np.asarray(erow, dtype=np.int32)).cuda(), torch.from_numpy(wcol).cuda(), torch.from_numpy(wcoef).cuda()
    p = L.StftWindowMergeParams(encw=encw.data_ptr(), out=out.data_ptr(), erow=et.data_ptr(), wcol=ct.data_ptr(), wcoef=ft.data_ptr(), R=R_, n=n,
                                F=encw.shape[2], T=out.shape[3], w=encw.shape[3], Bw=encw.shape[0], Bout=out.shape[0])
    L.call("ds_stft_window_merge", ctypes.byref(p), L.current_stream())
    torch.cuda.synchronize()


def _windows(rows, F, w, seed):
    """(rows, 3, F, w): log-magnitudes in [0, 6], (cos, sin) pairs of lengths 0.1 ... 1 — not unit length, as the decoder's are not."""
    g = torch.Generator().manual_seed(seed)
    mag = 6.0 * torch.rand(rows, F, w, generator=g)
    ang = 2 * np.pi * torch.rand(rows, F, w, generator=g)
    length = 0.1 + 0.9 * torch.rand(rows, F, w, generator=g)
    return torch.stack([mag, length * torch.cos(ang), length * torch.sin(ang)], dim=1)


@pytest.mark.parametrize("F", [5, 8])
@pytest.mark.parametrize("T,w,stride,loop", PLANS)
def test_stft_merge_is_the_restatement(T, w, stride, loop, F):
    offsets, entries = R.plan(T, w, stride, loop)
    n = len(offsets)
    wcol, wcoef = _tables(entries, T)
    encw = _windows(Rk * n + 2, F, w, seed=100 + T)
    erow = np.random.RandomState(T).permutation(Rk * n + 2)[:Rk * n].reshape(Rk, n)
    many = [x for x, ent in enumerate(entries) if len(ent) > 1]
    j, c, _ = entries[many[0]][1]
    encw[erow[1, j], 1:, F // 2, c] = 0.0                          # an exact (0, 0) pair under two windows: phase 0
    unused = sorted(set(range(Rk * n + 2)) - set(erow.ravel().tolist()))
    encw[unused] = float("nan")                                    # rows no table entry names are not read
    want = D.stft_merge(encw.numpy()[erow], entries)
    assert np.isfinite(want).all()
    encw = encw.cuda()
    out = torch.full((Rk + 1, 3, F, T), 7.0, device="cuda")
    _merge(encw, out, erow, wcol, wcoef, Rk, n)
    err = rel_err(D.spectrum(out[:Rk].cpu()), D.spectrum(want))
    print(f"ds_stft_window_merge vs float64, T={T} w={w} stride={stride} loop={loop} F={F}: {err:.2e}")
    assert err < 1e-4                                              # test_stft_plus_and_audio_round_trip's bound for log1p / rsqrt
    assert (out[Rk] == 7.0).all()                                  # an output row beyond R is untouched
    one = [x for x, ent in enumerate(entries) if len(ent) == 1]
    assert one or loop
    for x in one:                                                  # a frame under one window keeps the window's bits
        j, c, f = entries[x][0]
        assert f == 1.0 and torch.equal(out[:Rk, :, :, x], encw[torch.from_numpy(erow[:, j]).cuda(), :, :, c])
    for x in many:                                                 # a blended frame is a representation
        assert ((out[:Rk, 1, :, x] ** 2 + out[:Rk, 2, :, x] ** 2) - 1).abs().max() < 1e-5
    # a row with a window row out of range reads nothing and is NaN; its neighbour keeps its bits
    for badrow in (Rk * n + 2, -1):
        e2 = erow.copy()
        e2[1, n - 1] = badrow
        out2 = torch.full_like(out, 7.0)
        _merge(encw, out2, e2, wcol, wcoef, Rk, n)
        assert torch.isnan(out2[1]).all() and torch.equal(out2[0], out[0]) and torch.equal(out2[2:], out[2:])
    # an entry that names no window (or no frame of one) makes that frame NaN in all three channels, and only that one
    for x in (5, many[0]):
        for field, value in ((L.WM["DS_WM_WIN"], n), (L.WM["DS_WM_COL"], w), (L.WM["DS_WM_COL"], -1)):
            c2 = wcol.copy()
            c2[0, x, field] = value
            out3 = torch.full_like(out, 7.0)
            _merge(encw, out3, erow, c2, wcoef, Rk, n)
            keep = [y for y in range(T) if y != x]
            assert torch.isnan(out3[:Rk, :, :, x]).all() and torch.equal(out3[..., keep], out[..., keep])


def test_stft_merge_without_overlap_is_indexing():
    T, w, F = 48, 16, 8
    offsets, entries = R.plan(T, w, 16, False)
    assert offsets == [0, 16, 32] and all(len(e) == 1 for e in entries)
    wcol, wcoef = _tables(entries, T)
    encw = _windows(Rk * 3, F, w, seed=1).cuda()
    erow = np.random.RandomState(1).permutation(Rk * 3).reshape(Rk, 3)
    out = torch.full((Rk, 3, F, T), 7.0, device="cuda")
    _merge(encw, out, erow, wcol, wcoef, Rk, 3)
    want = torch.cat([encw[torch.from_numpy(erow[:, j]).cuda()] for j in range(3)], dim=-1)
    assert torch.equal(out, want)


@pytest.mark.parametrize("T,w,F", [(40, 16, 8), (42, 12, 5)])
def test_stft_merge_rotating_the_windows_of_a_loop_rolls_the_output(T, w, F):
    """stride = w / 2: every frame lies under two windows, and two addends commute."""
    stride = w // 2
    offsets, entries = R.plan(T, w, stride, True)
    n = len(offsets)
    assert T % stride == 0 and all(len(e) == 2 for e in entries)
    wcol, wcoef = _tables(entries, T)
    encw = _windows(Rk * n, F, w, seed=T).cuda()
    erow = np.arange(Rk * n).reshape(Rk, n)
    a, b = torch.full((Rk, 3, F, T), 7.0, device="cuda"), torch.full((Rk, 3, F, T), 7.0, device="cuda")
    _merge(encw, a, erow, wcol, wcoef, Rk, n)
    _merge(encw, b, np.roll(erow, 1, axis=1), wcol, wcoef, Rk, n)  # window j + 1 now holds what window j held
    assert torch.isfinite(a).all() and torch.equal(b, torch.roll(a, stride, dims=-1))


# ------------------------------------------------------------------------------------------------ ds_istft_plus_loop
def _representation(B, F, T, seed):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(B, 3, F, T, generator=g)
    enc[:, 0] = enc[:, 0].abs() * 0.5
    return enc


@pytest.mark.parametrize("T", [12, 13])
def test_istft_loop_is_the_circular_restatement(T):
    from diffusynth_amd.vocoder import stft_representation_to_audio
    enc = _representation(2, 512, T, seed=T)
    audio = stft_representation_to_audio(enc.cuda(), loop=True)
    assert audio.shape == (2, 256 * T)
    want = np.stack([D.istft_loop(V.depad_stft(D.decode(e.numpy())), 256) for e in enc])
    err = rel_err(audio.cpu(), want)
    print(f"ds_istft_plus_loop vs the circular restatement, T={T}: {err:.2e}")
    assert err < 1e-3                                              # test_latents_to_audio_matches_oracle's bound
    rolled = stft_representation_to_audio(torch.roll(enc, 4, dims=-1).cuda(), loop=True)
    assert torch.equal(rolled, torch.roll(audio, 4 * 256, dims=-1))


def test_istft_loop_rejects_a_loop_shorter_than_a_frame_and_leaves_the_plain_path_alone():
    from diffusynth_amd.vocoder import stft_representation_to_audio
    with pytest.raises(L.DsError, match="istft_plus_loop"):
        stft_representation_to_audio(_representation(1, 512, 3, seed=0).cuda(), loop=True)
    enc = _representation(2, 512, 12, seed=1).cuda()
    plain = stft_representation_to_audio(enc)
    ws = torch.empty(L.load().ds_istft_ws_floats(2, 512, 12), dtype=torch.float32, device="cuda")
    direct = torch.empty((2, 256 * 11), dtype=torch.float32, device="cuda")
    L.call("ds_istft_plus", enc.data_ptr(), 2, 512, 12, 256, ws.data_ptr(), direct.data_ptr(), L.current_stream())
    assert plain.shape == (2, 256 * 11) and torch.equal(plain, direct)
    assert torch.equal(stft_representation_to_audio(enc, loop=False), direct)


# ------------------------------------------------------------------------------------------------ the production VQGAN, fp32
H, KW = 128, dict(window=4, stride=2)
UP = 4


@pytest.fixture(scope="module")
def vae(vqgan_sd):
    from diffusynth_amd.vqgan import PRODUCTION_CONFIG, VQGAN
    m = VQGAN(**PRODUCTION_CONFIG)
    m.load_state_dict(vqgan_sd)
    m = m.to("cuda")
    m._decoder.set_compute_dtype("fp32")
    m._encoder.set_compute_dtype("fp32")
    return m


def _window_rows(x, offsets, window):
    """(B, C, H, W) -> (B n, C, H, window) in the order (row, window): the batch the wrappers show their module."""
    xw = torch.from_numpy(R.split(x.cpu().numpy(), offsets, window))
    return xw.reshape((-1,) + tuple(xw.shape[2:])).cuda()


@pytest.mark.parametrize("W,loop", [(10, False), (11, False), (10, True)])
def test_windowed_decoder_on_the_vqgan(vae, W, loop):
    from diffusynth_amd.vocoder import latents_to_audio
    dec = vae._decoder
    q = synth_input("decwin_q%d" % W, (2, 4, H, W)).cuda()
    wdec = WindowedDecoder(dec, loop=loop, **KW)
    got = wdec(q)
    assert got.shape == (2, 3, 4 * H, UP * W)
    offsets, _ = R.plan(W, 4, 2, loop)
    n = len(offsets)
    assert wdec.rows_per_sample(W) == n
    encw = dec(_window_rows(q, offsets, 4))                        # the same (row, window) batch: batch effects cancel
    assert encw.shape == (2 * n, 3, 4 * H, UP * 4)
    _, entries = D.frame_plan(W, 4, 2, loop, UP)
    want = D.stft_merge(encw.cpu().numpy().reshape((2, n) + tuple(encw.shape[1:])), entries)
    err = rel_err(D.spectrum(got.cpu()), D.spectrum(want))
    audio = latents_to_audio(wdec, q)
    spec = [V.depad_stft(D.decode(w_)) for w_ in want]
    ref = np.stack([D.istft_loop(s, 256) if loop else V.istft(s, 256, 1024) for s in spec])
    assert audio.shape == ref.shape == (2, 256 * (UP * W if loop else UP * W - 1))
    aerr = rel_err(audio.cpu(), ref)
    chunked = WindowedDecoder(dec, loop=loop, max_rows=3, **KW)(q)
    print(f"WindowedDecoder on the VQGAN, W={W} loop={loop}: spectrum {err:.2e}, audio {aerr:.2e}")
    assert err < 1e-4 and aerr < 1e-3
    assert torch.equal(chunked, got)                               # the fp32 decoder is batch-invariant


def test_a_width_of_one_window_is_the_decoder(vae):
    q = synth_input("decwin_q4", (2, 4, H, 4)).cuda()
    assert torch.equal(WindowedDecoder(vae._decoder, **KW)(q), vae._decoder(q))


def test_decoder_locality(vae):
    """W = 12: windows at 0, 2, 4, 6, 8.  Columns >= 8 lie in the last three only, and frames < 8 come from the first window alone."""
    dec = vae._decoder
    q = synth_input("decwin_q12", (2, 4, H, 12)).cuda()
    q2 = q.clone()
    q2[..., 8:] += synth_input("decwin_bump", (2, 4, H, 4)).cuda()
    wdec = WindowedDecoder(dec, **KW)
    a, b = wdec(q), wdec(q2)
    assert torch.equal(a[..., :8], b[..., :8]) and not torch.equal(a[..., 32:], b[..., 32:])
    assert not torch.equal(dec(q)[..., :8], dec(q2)[..., :8])       # the full-width decoder normalises over everything


def test_a_loop_has_no_seam(vae):
    """Rolling the latent of a loop by one stride rolls the audio: the cut is nowhere.  The plain decoder's audio has ends."""
    from diffusynth_amd.vocoder import latents_to_audio
    dec = vae._decoder
    q = synth_input("decwin_loop12", (2, 4, H, 12)).cuda()
    shift = 2 * UP * 256
    wdec = WindowedDecoder(dec, loop=True, **KW)
    a, b = latents_to_audio(wdec, q), latents_to_audio(wdec, torch.roll(q, 2, dims=-1))
    assert a.shape == (2, 256 * UP * 12)
    seam = ((b - torch.roll(a, shift, dims=-1)).abs().max() / a.abs().max()).item()
    pa, pb = latents_to_audio(dec, q), latents_to_audio(dec, torch.roll(q, 2, dims=-1))
    assert pa.shape == (2, 256 * (UP * 12 - 1))
    plain = ((pb - torch.roll(pa, shift, dims=-1)).abs().max() / pa.abs().max()).item()
    print(f"loop W=12 rolled by a stride: windowed {seam:.2e} of the peak, plain decoder + ds_istft_plus {plain:.2e}")
    assert seam < 1e-3
    assert not plain < 1e-3


def test_the_batch_helper_on_the_wrapper(vae):
    from diffusynth_amd.vocoder import encodeBatch2GradioOutput_STFT
    q = synth_input("decwin_q10", (2, 4, H, 10))
    for loop, samples in ((True, 256 * 40), (False, 256 * 39)):
        wdec = WindowedDecoder(vae._decoder, loop=loop, **KW)
        orig = wdec(q.cuda()).cpu()
        out = encodeBatch2GradioOutput_STFT(wdec, q.numpy(), original_STFT_batch=orig)
        assert len(out) == 6 and all(isinstance(o, list) and len(o) == 2 for o in out)
        for k in (0, 1, 3, 4):
            assert all(im.shape == (513, 40, 3) and im.dtype == np.uint8 for im in out[k])
        for k in (2, 5):
            assert all(s.shape == (samples,) and s.dtype == np.float64 and np.isfinite(s).all() for s in out[k])


@pytest.mark.parametrize("loop", [False, True])
def test_windowed_encoder_on_the_vqgan(vae, loop):
    enc = vae._encoder
    x = vae._decoder(synth_input("decwin_q10", (2, 4, H, 10)).cuda())     # a representation with the decoder's statistics
    assert x.shape == (2, 3, 512, 40)
    wenc = WindowedEncoder(enc, loop=loop, **KW)
    got = wenc(x)
    assert got.shape == (2, 4, 128, 10)
    foff, _ = D.frame_plan(10, 4, 2, loop, 4)
    offsets, entries = R.plan(10, 4, 2, loop)
    zw = enc(_window_rows(x, foff, 16))                            # the same batched encoder output
    want = R.merge(zw.cpu().numpy().reshape((2, len(offsets)) + tuple(zw.shape[1:])), entries)
    assert np.isfinite(want).all() and torch.equal(got.cpu(), torch.from_numpy(want))
