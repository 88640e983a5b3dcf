"""Windowed sampling on the GPU: ds_window_split against indexing and ds_window_merge against the numpy restatement
(tests/window_ref.py) bit for bit, WindowedUnet on the production U-Net (synthetic weights) against RefWindowed — one model call per
window, blended on the host — locality, loop equivariance, the tiers, every sampler entry point, the batcher and serving."""
import ctypes

import numpy as np
import pytest
import torch

import window_ref as R
from conftest import rel_err
from diffusynth_amd import _lib as L
from diffusynth_amd.batching import SamplingBatcher
from diffusynth_amd.sampler import DiffSynthSampler
from diffusynth_amd.synth import synth_input
from diffusynth_amd.windowed import WindowedUnet

pytestmark = pytest.mark.gpu

MAXM = L.WM["DS_WM_MAXM"]
# (W, window, stride, loop): 16-byte pieces (W = 40, 32, 200), the scalar kernel (W = 43, 42), a wrap, four windows over a column,
# and (W = 44, stride 6) the 16-byte kernel on offsets that are no multiple of 4
PLANS = [(40, 16, 8, False), (43, 16, 8, False), (32, 16, 4, False), (200, 64, 32, False), (40, 16, 8, True), (42, 16, 12, True),
         (44, 16, 6, False), (44, 16, 6, True)]
Cc, Hk, Rk = 4, 8, 3


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32).view(np.uint32)


def _randn(*shape, seed=0):
    return torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


# ------------------------------------------------------------------------------------------------ ds_window_split
def _split(x, out, rows, w):
    t = torch.tensor(rows, dtype=torch.int32).reshape(-1, L.WS["DS_WS_NI"]).cuda()
    p = L.WindowSplitParams(x=x.data_ptr(), out=out.data_ptr(), rows=t.data_ptr(), R=t.shape[0], C=x.shape[1], H=x.shape[2], W=x.shape[3], w=w,
                            Bx=x.shape[0], Bout=out.shape[0])
    L.call("ds_window_split", ctypes.byref(p), L.current_stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("W,window,stride,loop", PLANS)
def test_split_is_indexing(W, window, stride, loop):
    offsets, _ = R.plan(W, window, stride, loop)
    n = len(offsets)
    x = _randn(Rk, Cc, Hk, W, seed=W)
    perm = np.random.RandomState(W).permutation(Rk * n)           # the destination rows are the caller's to choose
    rows = [(r, offsets[j], int(perm[r * n + j])) for r in range(Rk) for j in range(n)]
    out = torch.full((Rk * n + 1, Cc, Hk, window), 7.0, device="cuda")
    _split(x, out, rows, window)
    want = torch.from_numpy(R.split(x.cpu().numpy(), offsets, window))
    for r, o, d in rows:
        assert torch.equal(out[d].cpu(), want[r, offsets.index(o)]), (r, o, d)
    assert (out[Rk * n] == 7.0).all()                           # a row no table row names is not written
    # malformed rows: a source row or an offset out of range is NaN and reads nothing, a destination out of range writes nothing
    out2 = torch.full_like(out, 7.0)
    bad = [(Rk, 0, 0), (0, W, 1), (0, -1, 2), (1, offsets[1], Rk * n + 1), (1, offsets[1], -1), (2, offsets[1], 3)]
    _split(x, out2, bad, window)
    assert torch.isnan(out2[:3]).all() and torch.equal(out2[3].cpu(), want[2, 1]) and (out2[4:] == 7.0).all()


# ------------------------------------------------------------------------------------------------ ds_window_merge
def _tables(entries, W):
    wcol = np.zeros((MAXM, W, L.WM["DS_WM_NI"]), dtype=np.int32)
    wcol[:, :, L.WM["DS_WM_WIN"]] = -1
    wcoef = np.zeros((MAXM, W), dtype=np.float32)
    for x, ent in enumerate(entries):
        for m, (j, c, f) in enumerate(ent):
            wcol[m, x, L.WM["DS_WM_WIN"]], wcol[m, x, L.WM["DS_WM_COL"]], wcoef[m, x] = j, c, f
    return wcol, wcoef


def _merge(eps, out, erow, wcol, wcoef, R_, n):
    et, ct, ft = torch.from_numpy(np.asarray(erow, dtype=np.int32)).cuda(), torch.from_numpy(wcol).cuda(), torch.from_numpy(wcoef).cuda()
    p = L.WindowMergeParams(eps=eps.data_ptr(), out=out.data_ptr(), erow=et.data_ptr(), wcol=ct.data_ptr(), wcoef=ft.data_ptr(), R=R_, n=n,
                            C=eps.shape[1], H=eps.shape[2], W=out.shape[3], w=eps.shape[3], Beps=eps.shape[0], Bout=out.shape[0])
    L.call("ds_window_merge", ctypes.byref(p), L.current_stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("W,window,stride,loop", PLANS)
def test_merge_is_the_restatement_bit_for_bit(W, window, stride, loop):
    offsets, entries = R.plan(W, window, stride, loop)
    n = len(offsets)
    wcol, wcoef = _tables(entries, W)
    eps = _randn(Rk * n + 2, Cc, Hk, window, seed=100 + W)
    erow = np.random.RandomState(W).permutation(Rk * n + 2)[:Rk * n].reshape(Rk, n)
    unused = sorted(set(range(Rk * n + 2)) - set(erow.ravel().tolist()))
    eps[unused] = float("nan")                                  # rows no table entry names are not read
    want = R.merge(eps.cpu().numpy()[erow], entries)
    assert np.isfinite(want).all()
    out = torch.full((Rk + 1, Cc, Hk, W), 7.0, device="cuda")
    _merge(eps, out, erow, wcol, wcoef, Rk, n)
    assert np.array_equal(_bits(out[:Rk]), _bits(want))
    assert (out[Rk] == 7.0).all()                               # an output row beyond R is untouched
    one = [x for x, ent in enumerate(entries) if len(ent) == 1]
    if not loop:
        assert one
    for x in one:                                               # a coefficient of 1.0 returns the window's bits
        j, c, f = entries[x][0]
        assert f == 1.0 and torch.equal(out[:Rk, :, :, x], eps[torch.from_numpy(erow[:, j]).cuda(), :, :, c])
    # a row with an eps row out of range reads nothing and is NaN; its neighbours keep their bits
    for badrow in (Rk * n + 2, -1):
        e2 = erow.copy()
        e2[1, n - 1] = badrow
        out2 = torch.full_like(out, 7.0)
        _merge(eps, out2, e2, wcol, wcoef, Rk, n)
        assert torch.isnan(out2[1]).all() and torch.equal(out2[0], out[0]) and torch.equal(out2[2:], out[2:])
    # a column entry that names no window (or no column of one) makes that column NaN, and only that one
    for field, value in ((L.WM["DS_WM_WIN"], n), (L.WM["DS_WM_COL"], window), (L.WM["DS_WM_COL"], -1)):
        c2 = wcol.copy()
        c2[0, 5, field] = value
        out3 = torch.full_like(out, 7.0)
        _merge(eps, out3, erow, c2, wcoef, Rk, n)
        keep = [x for x in range(W) if x != 5]
        assert torch.isnan(out3[:Rk, :, :, 5]).all() and torch.equal(out3[..., keep], out[..., keep])


# ------------------------------------------------------------------------------------------------ U-Net, fp32 tier
H = 32
KW = dict(window=32, stride=16)


@pytest.fixture(scope="module")
def unet(unet_sd):
    from diffusynth_amd.unet import ConditionedUnet, PRODUCTION_CONFIG
    m = ConditionedUnet(**PRODUCTION_CONFIG)
    m.load_state_dict(unet_sd)
    return m.to("cuda")


def _cfg_rows(W, B=2):
    """The doubled batch of classifier-free guidance: (x, t, c) of 2 B rows."""
    x, t = synth_input("win_x%d" % W, (B, 4, H, W)).cuda(), torch.tensor([700, 90][:B], device="cuda")
    c, un = synth_input("win_c", (B, 512)).cuda(), synth_input("win_un", (512,)).cuda()
    return torch.cat([x, x]), torch.cat([t, t]), torch.cat([un[None].repeat(B, 1), c])


@pytest.mark.parametrize("W,loop,n,last", [(80, False, 4, 48), (83, False, 5, 51), (80, True, 5, 64)])
def test_windowed_unet_is_ref_windowed(unet, W, loop, n, last):
    unet.set_compute_dtype("fp32")
    x, t, c = _cfg_rows(W)
    net = WindowedUnet(unet, loop=loop, **KW)
    assert net.rows_per_sample(W) == n and net.plan(W).offsets[-1] == last
    want = R.RefWindowed(unet, loop=loop, **KW)(x, t, c)
    got = net(x, t, c)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    assert torch.equal(net(x, t, c, paired_halves=True), want)
    chunked = WindowedUnet(unet, loop=loop, max_rows=6, **KW)
    assert torch.equal(chunked(x, t, c), want) and torch.equal(chunked(x, t, c, paired_halves=True), want)


def test_a_width_of_one_window_is_the_model(unet):
    unet.set_compute_dtype("fp32")
    x, t, c = _cfg_rows(32)
    net = WindowedUnet(unet, **KW)
    assert net.rows_per_sample(32) == 1
    assert torch.equal(net(x, t, c), unet(x, t, c)) and torch.equal(net(x, t, c, paired_halves=True), unet(x, t, c))


def test_locality(unet):
    """Columns >= 64 lie in the last window (48 ... 79) only and output columns < 32 come from the first two (0 ... 47)."""
    unet.set_compute_dtype("fp32")
    x, t, c = _cfg_rows(80)
    x2 = x.clone()
    x2[..., 64:] += synth_input("win_bump", (4, 4, H, 16)).cuda()
    net = WindowedUnet(unet, **KW)
    a, b = net(x, t, c), net(x2, t, c)
    assert torch.equal(a[..., :32], b[..., :32]) and not torch.equal(a[..., 64:], b[..., 64:])
    assert not torch.equal(unet(x, t, c)[..., :32], unet(x2, t, c)[..., :32])          # the full-width call sees everything


def test_loop_equivariance(unet):
    """Rolling a loop by one stride rolls the result: the windows are the same, one place on, and the two addends of a column commute."""
    unet.set_compute_dtype("fp32")
    x, t, c = _cfg_rows(80)
    net = WindowedUnet(unet, loop=True, **KW)
    assert (net.plan(80).cover == 2).all()
    assert torch.equal(net(torch.roll(x, 16, dims=-1), t, c), torch.roll(net(x, t, c), 16, dims=-1))
    plain = WindowedUnet(unet, **KW)                            # without the wrap the ends differ
    assert not torch.equal(plain(torch.roll(x, 16, dims=-1), t, c), torch.roll(plain(x, t, c), 16, dims=-1))


def test_tiers(unet):
    x, t, c = _cfg_rows(80)
    net = WindowedUnet(unet, **KW)
    unet.set_compute_dtype("fp32")
    ref32 = net(x, t, c).clone()
    try:
        assert net.set_compute_dtype("bf16x3") is net and unet.compute_dtype == "bf16x3"
        e = rel_err(net(x, t, c), ref32)
        print(f"windowed bf16x3 (unpinned) vs windowed fp32 tier, W=80: {e:.2e}")
        assert e < 1e-4                                         # test_hip_unet.py: the tier against the fp32 tier
        net.pin_launch_batch(16)                                # 4 rows of 4 windows
        assert unet.launch_batch == 16
        assert torch.equal(net(x, t, c), R.RefWindowed(unet, **KW)(x, t, c))
    finally:
        unet.pin_launch_batch(None)
        unet.set_compute_dtype("fp32")


# ------------------------------------------------------------------------------------------------ sampler
USE = [int(v) for v in np.linspace(0, 999, 4, dtype=np.int32)]
W80 = 80


def _sampler(strategy, B=2, cfg=3.0, noise_device="cpu", use=USE):
    s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=B, max_width=96, noise_strategy=strategy, noise_device=noise_device)
    s.respace(use)
    if cfg != 1.0:
        s.activate_classifier_free_guidance(cfg, synth_input("win_un", (512,)).cuda())
    return s


def _same_trajectory(got, want):
    assert len(got) == len(want) > 1
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(b).all() and torch.equal(a, b), k


@pytest.mark.parametrize("strategy", ["repeat", "non_repeat"])
@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "dpmpp_2m"])
def test_sample_on_the_wrapper_is_sample_on_ref_windowed(unet, sampler, strategy):
    unet.set_compute_dtype("fp32")
    cond = synth_input("win_c", (2, 512)).cuda()
    run = lambda model: _sampler(strategy).sample(model, (2, 4, H, W80), return_tensor=True, condition=cond, sampler=sampler, seed=3)  # noqa: E731
    got, want = run(WindowedUnet(unet, **KW)), run(R.RefWindowed(unet, **KW))
    assert torch.equal(got[1], want[1])
    _same_trajectory(got[0], want[0])


@pytest.mark.parametrize("strategy", ["repeat", "non_repeat"])
def test_inpaint_on_the_wrapper_is_inpaint_on_ref_windowed(unet, strategy):
    unet.set_compute_dtype("fp32")
    cond, guide = synth_input("win_c", (2, 512)).cuda(), synth_input("win_guide", (2, 4, H, 64)).cuda()
    run = lambda model: _sampler(strategy).inpaint_sample(model, (2, 4, H, W80), 1.0, guide, None, return_tensor=True, condition=cond,  # noqa: E731
                                                          sampler="ddim", use_dynamic_mask=True, mask_flexivity=1.0, seed=4)
    got, want = run(WindowedUnet(unet, loop=True, **KW)), run(R.RefWindowed(unet, loop=True, **KW))
    _same_trajectory(got[0], want[0])


def test_edit_on_the_wrapper_is_edit_on_ref_windowed(unet):
    unet.set_compute_dtype("fp32")
    src, dst = synth_input("win_c", (2, 512)).cuda(), synth_input("win_dst", (2, 512)).cuda()
    x0 = synth_input("win_x0", (2, 4, H, W80)).cuda()
    out = []
    for model in (WindowedUnet(unet, **KW), R.RefWindowed(unet, **KW)):
        s = _sampler("non_repeat")
        inv = s.edit_invert(model, x0, condition=src, seed=5)
        out.append((inv, s.edit_sample(model, inv, condition=dst, return_tensor=True)[0]))
    (a, ta), (b, tb) = out
    assert torch.isfinite(b.z).all() and torch.equal(a.z, b.z) and torch.equal(a.x_start, b.x_start)
    _same_trajectory(ta, tb)


# ------------------------------------------------------------------------------------------------ batcher and serving
def test_windowed_requests_share_the_batcher_and_equal_the_calls_alone(unet):
    """A CFG request and a plain one a tick later at W = 80 (4 windows), one at W = 56 (3 windows) and a pass-through at W = 24."""
    unet.set_compute_dtype("fp32")
    net = WindowedUnet(unet, **KW)
    cond = lambda tag: synth_input("win_" + tag, (1, 512)).cuda()                              # noqa: E731
    mix = [
        (0, lambda: _sampler("repeat", 1), "sample", ((1, 4, H, 80),), dict(return_tensor=True, condition=cond("a"), sampler="ddim", seed=1)),
        (0, lambda: _sampler("repeat", 1, 1.0, "philox"), "sample", ((1, 4, H, 56),), dict(return_tensor=True, condition=cond("b"), sampler="ddpm", seed=2)),
        (0, lambda: _sampler("repeat", 1, 1.0), "sample", ((1, 4, H, 24),), dict(return_tensor=True, condition=cond("c"), sampler="dpmpp_2m", seed=3)),
        (1, lambda: _sampler("non_repeat", 1, 1.0), "sample", ((1, 4, H, 80),), dict(return_tensor=True, condition=cond("d"), sampler="dpmpp_2m", seed=4)),
    ]
    b = SamplingBatcher(net, max_rows=64)
    handles, tick = [None] * len(mix), 0
    while any(h is None for h in handles) or b.active():
        for i, (at, mk, method, args, kw) in enumerate(mix):
            if handles[i] is None and at <= tick:
                handles[i] = b.submit(mk(), method, *args, **kw)
        b.step()
        tick += 1
    # real U-Net rows: W = 80: the CFG pair alone (2 x 4), with the late request (3 x 4), the late request alone (4)
    assert b.ticks == 5
    assert {k[0] for k in b.unet_batches if k[2] == 80} == {8, 12, 4}
    assert {k[0] for k in b.unet_batches if k[2] == 56} == {3} and {k[0] for k in b.unet_batches if k[2] == 24} == {1}
    for i, (at, mk, method, args, kw) in enumerate(mix):
        want, first = getattr(mk(), method)(net, *args, **kw)
        got = handles[i].result()
        assert torch.equal(got[1], first), i
        _same_trajectory(got[0], want)
    # admission is by real rows
    with pytest.raises(ValueError, match="needs 8 U-Net rows, more than max_rows=7"):
        SamplingBatcher(net, max_rows=7).submit(mix[0][1](), "sample", *mix[0][3], **mix[0][4])
    SamplingBatcher(unet, max_rows=7).submit(mix[0][1](), "sample", *mix[0][3], **mix[0][4])       # the plain model: 2 rows


def test_mixed_widths_serving_on_the_wrapper(unet):
    from diffusynth_amd.serving import sample_mixed_widths
    unet.set_compute_dtype("fp32")
    net = WindowedUnet(unet, **KW)
    un = synth_input("win_un", (512,)).cuda()
    reqs = [{"width": w, "condition": synth_input("win_mw%d" % i, (512,)), "seed": 70 + i} for i, w in enumerate((24, 80, 80))]
    got = sample_mixed_widths(net, reqs, 4, height=H, cfg_scale=3.0, unconditional_condition=un, noise_device="cpu")
    for r, g in zip(reqs, got):
        s = DiffSynthSampler(1000, mute=True, device="cuda", height=H, max_batchsize=1, noise_device="cpu")
        s.respace(list(np.linspace(0, 999, 4, dtype=np.int32)))
        s.activate_classifier_free_guidance(3.0, un)
        want, _ = s.sample(net, (1, 4, H, r["width"]), return_tensor=True, condition=r["condition"].cuda().float()[None], seed=r["seed"])
        assert torch.isfinite(want[-1]).all() and torch.equal(g, want[-1][0]), r["width"]
