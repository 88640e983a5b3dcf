"""Windowed decoding on the host: the frame plan against the latent plan, the circular inverse STFT restatement against the linear
oracle, and WindowedDecoder / WindowedEncoder on CPU tensors with stub modules against tests/decode_window_ref.py."""
import numpy as np
import pytest
import torch
from torch import nn

import decode_window_ref as D
import window_ref as R
from conftest import rel_err
from diffusynth_amd.windowed import WindowedDecoder, WindowedEncoder, WindowedUnet, window_plan
from oracle import vocoder_ref as V

UP = 4
# (W, window, stride, loop) in latent columns
PLANS = [(10, 4, 2, False), (83, 32, 16, False), (10, 4, 2, True), (42, 16, 12, True)]


# ------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("W,window,stride,loop", PLANS)
@pytest.mark.parametrize("weights", ["hann", "uniform", "array"])
def test_frame_plan_is_the_latent_plan_scaled(W, window, stride, loop, weights):
    wt = np.linspace(0.5, 2.0, window) if weights == "array" else weights
    dec = WindowedDecoder(lambda q: q, window, stride, loop, wt)
    lp, fp = dec.plan(W), dec.plan(W, UP)
    assert lp.W == W and fp.W == UP * W and fp.window == UP * window and fp.n == lp.n
    assert np.array_equal(fp.offsets, UP * lp.offsets)
    for x in range(W):
        for u in range(UP):                                         # the frames of a column lie under that column's windows
            assert np.array_equal(fp.win[UP * x + u], lp.win[x])
            live = lp.win[x] >= 0
            assert np.array_equal(fp.col[UP * x + u][live], UP * lp.col[x][live] + u)
    # the package's frame plan is the restatement's
    offsets, entries = D.frame_plan(W, window, stride, loop, UP, wt)
    assert list(fp.offsets) == offsets
    for x, ent in enumerate(entries):
        assert [(j, c, f) for j, c, f in ent] == [(fp.win[x, m], fp.col[x, m], fp.coef[x, m]) for m in range(fp.cover[x])]
    assert np.allclose(fp.coef.sum(axis=1), 1.0, atol=1e-6)


def test_the_long_loop_has_three_windows_over_some_columns():
    p = window_plan(4 * 496, 4 * 64, 4 * 32, True)
    assert p.n == 16 and p.cover.max() == 3 and np.array_equal(p.offsets, 4 * window_plan(496, 64, 32, True).offsets)


# ------------------------------------------------------------------------------------------------ circular iSTFT
@pytest.mark.parametrize("T", [4, 12, 13])
def test_circular_istft_is_the_linear_one_on_a_tiled_spectrum(T):
    rng = np.random.RandomState(T)
    spec = rng.randn(513, T) + 1j * rng.randn(513, T)
    y, wss = D.istft_loop(spec, 256, with_wss=True)
    period = 256 * T
    tiled = V.istft(np.tile(spec, (1, 3)), 256, 1024)               # frame T of the tiling is centred on sample `period`
    assert y.shape == (period,) and tiled.shape == (256 * (3 * T - 1),)
    err = np.abs(y - tiled[period:2 * period]).max() / np.abs(y).max()
    print(f"circular iSTFT vs the linear one tiled three times, T={T}: {err:.1e}")
    assert err < 1e-12
    assert np.abs(wss - 1.5).max() < 1e-12
    # a roll of the frames is a roll of the period
    assert np.abs(D.istft_loop(np.roll(spec, 3, axis=1), 256) - np.roll(y, 3 * 256)).max() < 1e-12 * np.abs(y).max()


# ------------------------------------------------------------------------------------------------ WindowedDecoder on a stub
class StubDecoder(nn.Module):
    """(R, 4, H, w) -> (R, 3, 4 H, UP w): a fixed elementwise map of the window plus an offset per row that depends on the row's own
    content only — what a row gives does not depend on the batch it is in, and two windows disagree where they overlap."""
    cfg = {"stub": True}

    def __init__(self, up=UP, extra=0):
        super().__init__()
        self.up, self.extra, self.calls, self.last, self.dtype_set = up, extra, [], None, None

    def set_compute_dtype(self, name):
        self.dtype_set = name

    def forward(self, q):
        self.calls.append(q.shape[0])
        b = q.repeat_interleave(4, dim=2).repeat_interleave(self.up, dim=3)
        b = b * (1.0 + 0.125 * (torch.arange(b.shape[-1]) % self.up))
        off = q[:, :1, :1, :1] * 0.25 + q[:, 3:4, -1:, -1:] * 0.5
        out = torch.stack([(b[:, 0] + off[:, 0]).abs() * 1.5, torch.tanh(b[:, 1] + off[:, 0]), torch.tanh(b[:, 2] - off[:, 0])], dim=1)
        if self.extra:
            out = torch.cat([out, out[..., :self.extra]], dim=-1)
        self.last = out
        return out


def _latent(B, W, seed=0, H=3):
    return torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(seed))


def _decoded_windows(stub, q, window, stride, loop):
    """The stub on the (row, window) batch, as (B, n, 3, F, UP window) numpy, and the frame entries."""
    offsets, _ = R.plan(q.shape[-1], window, stride, loop)
    qw = torch.from_numpy(R.split(q.numpy(), offsets, window))     # (B, n, C, H, w)
    encw = stub(qw.reshape((-1,) + tuple(qw.shape[2:]))).numpy()
    _, entries = D.frame_plan(q.shape[-1], window, stride, loop, UP)
    return encw.reshape((q.shape[0], len(offsets)) + encw.shape[1:]), entries


@pytest.mark.parametrize("W,window,stride,loop", PLANS + [(11, 4, 2, False), (12, 4, 1, True)])
def test_windowed_decoder_is_the_restatement(W, window, stride, loop):
    stub = StubDecoder()
    q = _latent(2, W, seed=W)
    dec = WindowedDecoder(stub, window, stride, loop)
    got = dec(q)
    assert got.shape == (2, 3, 12, UP * W) and got.dtype == torch.float32 and stub.calls == [2 * dec.rows_per_sample(W)]
    encw, entries = _decoded_windows(StubDecoder(), q, window, stride, loop)
    err = rel_err(D.spectrum(got), D.spectrum(D.stft_merge(encw, entries)))
    print(f"CPU WindowedDecoder vs the float64 restatement, W={W} window={window} stride={stride} loop={loop}: {err:.2e}")
    assert err < 1e-5
    one =[x for x, ent in enumerate(entries) if len(ent) == 1]
    assert one or loop
    for x in one:                                                   # a frame under one window keeps the decoder's bits
        j, c, f = entries[x][0]
        assert f == 1.0 and torch.equal(got[..., x], torch.from_numpy(encw[:, j, :, :, c]))
    for x, ent in enumerate(entries):                               # a blended frame is a representation: its pair has unit length
        if len(ent) > 1:
            assert ((got[:, 1, :, x] ** 2 + got[:, 2, :, x] ** 2) - 1).abs().max() < 1e-5
    # chunks: the same bits
    chunked = WindowedDecoder(StubDecoder(), window, stride, loop, max_rows=3)
    assert torch.equal(chunked(q), got) and max(chunked.decoder.calls) <= 3 and sum(chunked.decoder.calls) == stub.calls[0]


def test_windowed_decoder_passes_through_and_passes_on():
    stub = StubDecoder()
    dec = WindowedDecoder(stub, 4, 2)
    q = _latent(2, 4)
    assert dec(q) is stub.last and stub.calls == [2] and dec.rows_per_sample(4) == 1 and dec.rows_per_sample(10) == 4
    assert dec.loop is False and WindowedDecoder(stub, 4, 2, loop=True).loop is True
    assert dec.cfg is stub.cfg and dec.set_compute_dtype("bf16") is dec and stub.dtype_set == "bf16"
    real = WindowedDecoder(nn.Conv2d(4, 3, 1), 4, 2)
    assert len(list(real.parameters())) == 2
    # a loop of one window's width is still windowed: its ends are blended
    assert WindowedDecoder(stub, 4, 2, loop=True).rows_per_sample(4) == 2


def test_windowed_decoder_errors():
    stub = StubDecoder()
    for kw in (dict(stride=0), dict(stride=5), dict(weights="triangle"), dict(weights=[1.0, 2.0]), dict(weights=[1.0, -1.0, 1.0, 1.0]),
               dict(max_rows=0), dict(window=0)):
        with pytest.raises(ValueError):
            WindowedDecoder(stub, **dict(dict(window=4, stride=2), **kw))
    with pytest.raises(ValueError, match="DS_WM_MAXM"):
        WindowedDecoder(stub, 64, 4)(_latent(1, 128))
    with pytest.raises(ValueError, match="narrower"):
        WindowedDecoder(stub, 4, 2, loop=True)(_latent(1, 3))
    with pytest.raises(ValueError, match="multiple of 4"):
        WindowedDecoder(StubDecoder(extra=1), 4, 2)(_latent(1, 10))


def test_the_shared_part_is_shared():
    """One copy of plans, tables and layouts for the three wrappers."""
    from diffusynth_amd import windowed
    for name in ("plan", "windowed", "rows_per_sample", "_layout", "_column_tables", "_split", "_merge", "_call_chunks"):
        owners = {getattr(cls, name).__qualname__.split(".")[0] for cls in (WindowedUnet, WindowedDecoder, WindowedEncoder)}
        assert owners == {windowed._Windowed.__name__}, (name, owners)


# ------------------------------------------------------------------------------------------------ WindowedEncoder on a stub
class StubEncoder(nn.Module):
    """(R, 3, F, T) -> (R, 4, F / 4, T / 4): strided picks and elementwise arithmetic, plus an offset of the row's own content."""
    cfg = {"stub": True}

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x):
        self.calls.append(tuple(x.shape))
        off = x[:, :1, :1, :1] * 0.5 - x[:, 2:3, -1:, -1:]
        return torch.stack([x[:, c % 3, (c % 2)::4, ::4] * (1.0 + 0.25 * c) + x[:, (c + 1) % 3, 1::4, 2::4] + off[:, 0] for c in range(4)], dim=1)


@pytest.mark.parametrize("W,window,stride,loop", [(10, 4, 2, False), (11, 4, 3, False), (10, 4, 2, True), (9, 4, 3, True)])
def test_windowed_encoder_is_one_call_per_window(W, window, stride, loop):
    x = torch.randn(2, 3, 8, 4 * W, generator=torch.Generator().manual_seed(W))
    enc = WindowedEncoder(StubEncoder(), window, stride, loop)
    got = enc(x)
    want = D.windowed_encode(StubEncoder(), x, window, stride, loop, 4)
    assert got.shape == (2, 4, 2, W) and torch.isfinite(want).all() and torch.equal(got, want)
    n = enc.rows_per_sample(W)
    assert enc.encoder.calls == [(2, 3, 8, 4 * W), (2 * n, 3, 8, 4 * window)]     # the first call reads the frames per column
    assert torch.equal(enc(x), want) and enc.encoder.calls[2:] == [(2 * n, 3, 8, 4 * window)]
    chunked = WindowedEncoder(StubEncoder(), window, stride, loop, max_rows=3)
    assert torch.equal(chunked(x), want) and all(c[0] <= 3 for c in chunked.encoder.calls[1:])


def test_windowed_encoder_passes_through_and_errors():
    stub = StubEncoder()
    enc = WindowedEncoder(stub, 4, 2)
    x = torch.randn(2, 3, 8, 16)
    assert torch.equal(enc(x), stub(x)) and enc.cfg is stub.cfg and enc.loop is False
    with pytest.raises(ValueError, match="multiple"):
        enc(torch.randn(1, 3, 8, 42))
    with pytest.raises(ValueError):
        WindowedEncoder(stub, 4, 5)
