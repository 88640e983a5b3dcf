"""Windowed sampling without a GPU: window_plan against the restatement (tests/window_ref.py), its coverage and coefficients, every
ValueError, and WindowedUnet on CPU tensors with a stub model against RefWindowed (one model call per window), bit for bit."""
import numpy as np
import pytest
import torch

import window_ref as R
from diffusynth_amd.windowed import MAXM, WindowedUnet, window_plan

# (W, window, stride, loop)
PLANS = [(40, 16, 8, False), (43, 16, 8, False), (32, 16, 4, False), (200, 64, 32, False), (40, 16, 8, True), (42, 16, 12, True)]


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("weights", ["hann", "uniform"])
@pytest.mark.parametrize("W,window,stride,loop", PLANS)
def test_plan_is_the_restatement(W, window, stride, loop, weights):
    p = window_plan(W, window, stride, loop, weights)
    offsets, entries = R.plan(W, window, stride, loop, weights)
    assert p.n == len(offsets) and list(p.offsets) == offsets
    assert p.win.shape == p.col.shape == p.coef.shape == (W, MAXM) and p.coef.dtype == np.float32
    for x, ent in enumerate(entries):
        M = len(ent)
        assert p.cover[x] == M
        assert list(p.win[x, :M]) == [j for j, _, _ in ent] and (p.win[x, M:] == -1).all()
        assert list(p.col[x, :M]) == [c for _, c, _ in ent]
        assert np.array_equal(_bits(p.coef[x, :M]), _bits(np.array([f for _, _, f in ent])))


def test_the_named_plans():
    assert list(window_plan(43, 16, 8).offsets) == [0, 8, 16, 24, 27]
    assert window_plan(32, 16, 4).cover.max() == 4
    assert window_plan(200, 64, 32).n == 6
    loop = window_plan(42, 16, 12, loop=True)
    assert list(loop.offsets) == [0, 12, 24, 36]
    assert list(loop.win[0, :2]) == [0, 3] and list(loop.col[0, :2]) == [0, 6]       # the wrap falls inside window 3
    assert window_plan(40, 16, 8, loop=True).n == 5


@pytest.mark.parametrize("weights", ["hann", "uniform", "array"])
@pytest.mark.parametrize("W,window,stride,loop", PLANS)
def test_coverage_and_coefficients(W, window, stride, loop, weights):
    if weights == "array":
        weights = np.linspace(0.25, 3.0, window)
    p = window_plan(W, window, stride, loop, weights)
    assert (p.cover >= 1).all()                                             # every column is covered
    valid = p.win >= 0
    assert ((p.col >= 0) & (p.col < window))[valid].all() and (p.win < p.n).all()
    assert (p.coef[valid] > 0).all() and (p.coef[~valid] == 0).all()
    for x in range(W):
        M = int(p.cover[x])
        if M == 1:
            assert p.coef[x, 0] == np.float32(1.0)                          # one window: its bits are returned
        # M quotients in (0, 1], each rounded once to fp32: at most 2^-24 (in fact 2^-25) each
        assert abs(p.coef[x, :M].astype(np.float64).sum() - 1.0) <= M * 2.0 ** -23
        for m in range(M):
            assert (p.offsets[p.win[x, m]] + p.col[x, m]) % W == x
    if not loop:
        assert p.cover[0] == 1 and p.coef[0, 0] == np.float32(1.0)          # (the first column lies under window 0 only)


def test_value_errors():
    with pytest.raises(ValueError, match="DS_WM_MAXM"):
        window_plan(64, 32, 2)                                              # 16 windows over a column
    with pytest.raises(ValueError, match="stride"):
        window_plan(64, 16, 0)
    with pytest.raises(ValueError, match="stride"):
        window_plan(64, 16, 17)
    for bad in (np.zeros(16), -np.ones(16), np.full(16, np.nan), np.full(16, np.inf), np.ones(15), "triangle", [["a"]]):
        with pytest.raises(ValueError, match="weights"):
            window_plan(64, 16, 8, weights=bad)
    with pytest.raises(ValueError, match="loop"):
        window_plan(12, 16, 8, loop=True)
    window_plan(16, 16, 8, loop=True)                                       # W == window is a loop
    with pytest.raises(ValueError, match="nothing to cut"):
        window_plan(16, 16, 8)
    # the wrapper checks its arguments when it is built, and the width when it is asked
    with pytest.raises(ValueError, match="stride"):
        WindowedUnet(lambda x, t, c=None: x, window=16, stride=32)
    with pytest.raises(ValueError, match="max_rows"):
        WindowedUnet(lambda x, t, c=None: x, max_rows=0)
    with pytest.raises(ValueError, match="loop"):
        WindowedUnet(lambda x, t, c=None: x, window=16, stride=8, loop=True).rows_per_sample(12)


class Stub:
    """Depends on the neighbouring column (with a wrap at the width it is shown), on time and on the condition; exact IEEE
    multiplies and adds only, so a row's result does not depend on its batch."""
    cfg_paired_halves = True

    def __init__(self):
        self.calls = []

    def __call__(self, x, time, condition=None, paired_halves=False):
        self.calls.append((tuple(x.shape), bool(paired_halves)))
        if paired_halves:
            h = x.shape[0] // 2
            assert x.shape[0] % 2 == 0 and torch.equal(x[:h], x[h:]) and torch.equal(time[:h], time[h:])
        out = x * x * 0.125 + torch.roll(x, 1, dims=-1) * 0.25 + time.float().view(-1, 1, 1, 1) * 0.001
        if condition is not None:
            out = out + condition[:, 0].view(-1, 1, 1, 1)
        return out


def _inputs(B, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4, 8, W, generator=g), torch.arange(B) * 37 + 5, torch.randn(B, 3, generator=g)


@pytest.mark.parametrize("W,window,stride,loop", PLANS)
def test_cpu_wrapper_is_ref_windowed_bit_for_bit(W, window, stride, loop):
    x, t, c = _inputs(3, W)
    m = Stub()
    net = WindowedUnet(m, window, stride, loop)
    got = net(x, t, c)
    want = R.RefWindowed(Stub(), window, stride, loop)(x, t, c)
    assert got.shape == x.shape and torch.isfinite(want).all() and np.array_equal(_bits(got), _bits(want))
    n = net.rows_per_sample(W)
    assert n == window_plan(W, window, stride, loop).n and m.calls == [((3 * n, 4, 8, window), False)]
    assert not torch.equal(got, Stub()(x, t, c))                            # the windows are in use
    assert np.array_equal(_bits(net(x, t)), _bits(R.RefWindowed(Stub(), window, stride, loop)(x, t)))       # no condition


def test_pass_through_returns_the_models_tensor():
    class Keep(Stub):
        def __call__(self, *a, **k):
            self.last = super().__call__(*a, **k)
            return self.last
    x, t, c = _inputs(2, 16)
    m = Keep()
    net = WindowedUnet(m, 16, 8)
    assert net(x, t, c) is m.last and net(x[..., :9], t, c) is m.last and net.rows_per_sample(16) == net.rows_per_sample(9) == 1
    xx, tt = torch.cat([x, x]), torch.cat([t, t])
    assert net(xx, tt, torch.cat([c, -c]), paired_halves=True) is m.last and m.calls[-1] == ((4, 4, 8, 16), True)
    assert WindowedUnet(m, 16, 8, loop=True).rows_per_sample(16) == 2       # a loop of one window's width is still windowed


@pytest.mark.parametrize("W,loop", [(43, False), (40, True)])
def test_paired_order_keeps_the_halves_and_chunks_change_nothing(W, loop):
    x, t, c = _inputs(2, W, seed=1)
    xx, tt, cc = torch.cat([x, x]), torch.cat([t, t]), torch.cat([c, -c])
    m = Stub()
    net = WindowedUnet(m, 16, 8, loop)
    n = net.rows_per_sample(W)
    whole = net(xx, tt, cc)
    paired = net(xx, tt, cc, paired_halves=True)                            # (the stub checks that its halves are halves)
    assert m.calls == [((4 * n, 4, 8, 16), False), ((4 * n, 4, 8, 16), True)]
    assert np.array_equal(_bits(paired), _bits(whole))
    assert np.array_equal(_bits(whole), _bits(R.RefWindowed(Stub(), 16, 8, loop)(xx, tt, cc)))
    for max_rows in (6, 7, 4 * n - 1, 2):
        mc = Stub()
        chunked = WindowedUnet(mc, 16, 8, loop, max_rows=max_rows)
        assert np.array_equal(_bits(chunked(xx, tt, cc)), _bits(whole)), max_rows
        k = len(mc.calls)
        assert np.array_equal(_bits(chunked(xx, tt, cc, paired_halves=True)), _bits(whole)), max_rows
        for calls, is_paired in ((mc.calls[:k], False), (mc.calls[k:], True)):
            sizes = [s[0] for s, _ in calls]
            assert max(sizes) <= max_rows and sum(sizes) == 4 * n and len(sizes) > 1
            assert all(p == is_paired for _, p in calls)                    # a paired call's chunks are paired (the stub checks them)
    with pytest.raises(ValueError, match="max_rows"):
        WindowedUnet(Stub(), 16, 8, loop, max_rows=1)(xx, tt, cc, paired_halves=True)


def test_the_wrapper_passes_on_what_callers_ask_of_a_model():
    class Model(torch.nn.Module):
        cfg_paired_halves = True

        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(3))
            self._engine, self.asked = "engine", []

        def pin_launch_batch(self, n):
            self.asked.append(("pin", n))

        def set_compute_dtype(self, name):
            self.asked.append(("dtype", name))

        def use_hip_graph(self, on=True):
            self.asked.append(("graph", on))

    m = Model()
    net = WindowedUnet(m)
    assert [p is m.p for p in net.parameters()] == [True] and net.cfg_paired_halves is True and net._engine == "engine"
    assert net.pin_launch_batch(8) is net and net.set_compute_dtype("bf16x3") is net and net.use_hip_graph() is net
    assert m.asked == [("pin", 8), ("dtype", "bf16x3"), ("graph", True)]
    assert WindowedUnet(lambda x, t, c=None: x).cfg_paired_halves is False
    assert (net.rows_per_sample(64), net.rows_per_sample(65), net.rows_per_sample(256), net.rows_per_sample(1024)) == (1, 2, 7, 31)
