"""The mastering stage on the GPU: ds_master_gain to one fp32 ulp of the float64 restatement (tests/master_ref.py), ds_master_limit bit for
bit against the restatement evaluated at the device's gain, every signal its own, identity, degenerate inputs, PCM, bounds, and the wiring
through Track.render and DiffSynth.arrange.

Why one ulp for the gain: each of the <= 2^24 squares is exact in float64 and each partial sum is rounded once, so in any order the total
is within 2^-29 (relative) of the true sum; the square root, the division and the minimum add a few float64 roundings; after the rounding
to fp32 two such values differ by at most one ulp.  Everything behind the gain has no tolerance: np.array_equal."""
import functools

import numpy as np
import pytest
import torch

import arranger_ref as R
import master_ref as M
from conftest import load_golden
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

pytestmark = pytest.mark.gpu
MS, PV = L.MS, L.PV
T, SR, F32 = L.MS["DS_MS_TILE"], 16000, np.float32
GAIN = dict(target_rms=3.0, max_gain=2.0)        # with the test signal's spikes of 2^9 c: |u| <= 2^10 c whatever the gain comes to
CASES = [(0, 0), (1, 1), (80, 800), (1024, 8192)]


def mastering(a, h, **kw):
    m = A.Mastering(lookahead=(a + 0.5) / SR, hold=(h + 0.5) / SR, **{**GAIN, **kw})
    assert m.samples(SR) == (a, h)
    return m


def lengths_of(a, h):
    return [1, T + 1, 2 * T + h + 3 * a + 5] if a == 1024 else [1, 2, 80, 161, T - 1, T, T + 1, 2 * T + h + 3 * a + 5]


def cuda(xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def host(stats):
    return {k: getattr(stats, k).cpu().numpy() for k in stats._fields}


@functools.lru_cache(maxsize=None)
def batch(a, h):
    """One ragged launch per (A, R), shared by the tests below: (signals, outputs, stats on the host, the restatement of every signal at the
    DEVICE's gain)."""
    xs = [M.signal(n, a, h, seed=k, tile=T) for k, n in enumerate(lengths_of(a, h))]
    m = mastering(a, h)
    out, stats = A.master(cuda(xs), m, sample_rate=SR, return_stats=True)
    st = host(stats)
    refs = [M.master(x, a, h, gl=st["gain"][k], ceiling=m.ceiling, **GAIN) for k, x in enumerate(xs)]
    return xs, [o.cpu().numpy() for o in out], st, refs


def launch(x, tab, n_signals, max_len, total, m, a, h, *, pcm=True, pad=0, fill=-777.0):
    """The two entry points on a caller's table: (out with `pad` extra elements, pcm, stats, limited), every buffer filled with a sentinel."""
    lib = L.load()
    dtab = torch.from_numpy(np.ascontiguousarray(tab, np.int32).reshape(-1)).cuda()
    ws = torch.empty(max(1, lib.ds_master_ws_bytes(n_signals, max_len) // 8 + 1), dtype=torch.float64, device="cuda")
    stats = torch.full((n_signals, MS["DS_MS_NS"]), fill, dtype=torch.float32, device="cuda")
    limited = torch.full((n_signals,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((total + pad,), fill, dtype=torch.float32, device="cuda")
    pc = torch.full((total + pad,), -7, dtype=torch.int16, device="cuda") if pcm else None
    st = L.current_stream()
    target = 0.0 if m.target_rms is None else float(F32(m.target_rms))
    L.call("ds_master_gain", x.data_ptr(), dtab.data_ptr(), n_signals, max_len, total, target, float(F32(m.max_gain)), ws.data_ptr(), stats.data_ptr(),
           limited.data_ptr(), st)
    L.call("ds_master_limit", x.data_ptr(), dtab.data_ptr(), n_signals, max_len, total, float(F32(m.ceiling)), a, h, stats.data_ptr(), limited.data_ptr(),
           out.data_ptr(), L.ptr(pc), st)
    return out.cpu().numpy(), None if pc is None else pc.cpu().numpy(), stats.cpu().numpy(), limited.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- 1. gain
def test_gain_rms_and_peak_to_one_ulp():
    xs, _, st, refs = batch(80, 800)
    rng = np.random.default_rng(5)
    big = (0.3 * rng.standard_normal(2 ** 20 + 3001)).astype(F32)                  # more than DS_MS_MAX_PARTS chunks: the clamped partial count
    _, bs = A.master(cuda([big, xs[-1]]), mastering(80, 800), sample_rate=SR, return_stats=True)
    bs = host(bs)
    rows = [(x, st["gain"][k], st["rms"][k], st["peak"][k]) for k, x in enumerate(xs)] + [(big, bs["gain"][0], bs["rms"][0], bs["peak"][0])]
    for x, g, rms, peak in rows:
        _, g64, rms64, peak_ref = M.gain(x, **GAIN)
        ug, ur = M.ulps(g, g64), M.ulps(rms, rms64)
        print(f"N = {len(x)}: gain {g} ({ug:.3f} ulp of {g64!r}), rms {rms} ({ur:.3f} ulp), peak {peak}")
        assert ug <= 1.0 and ur <= 1.0 and peak == peak_ref and g.dtype == F32
    assert bs["gain"][1] == st["gain"][-1] and bs["rms"][1] == st["rms"][-1]      # the same bits beside another neighbour


# ---------------------------------------------------------------------------------------------------- 2. limiter
@pytest.mark.parametrize("a,h", CASES, ids=[f"A{a}_R{h}" for a, h in CASES])
def test_limiter_equals_the_restatement_bit_for_bit(a, h):
    xs, outs, st, refs = batch(a, h)
    for k, (x, y, ref) in enumerate(zip(xs, outs, refs)):
        assert np.abs(ref["u"]).max() <= 2 ** 10 * float(ref["c"]) and st["gain"][k] <= 2.0          # inside the exactness range
        assert M.ulps(st["gain"][k], ref["gain64"]) <= 1.0
        bad = np.flatnonzero(y.view(np.uint32) != ref["y"].view(np.uint32))
        print(f"A={a} R={h} N={len(x)}: gL {st['gain'][k]}, limited {st['limited'][k]} / {ref['limited']}, min g {st['min_gain'][k]} / {ref['min_gain']}, "
              f"{len(bad)} samples differ" + (f", first at {bad[0]}: {y[bad[0]]!r} / {ref['y'][bad[0]]!r}" if len(bad) else ""))
        assert y.dtype == F32 and np.array_equal(y, ref["y"])
        assert st["min_gain"][k] == ref["min_gain"] and st["limited"][k] == ref["limited"] and st["limited"].dtype == np.int32
        assert np.abs(y).max() <= ref["c"]
    # the case is not vacuous: samples were limited, and below the caps (whose reach R + 3 A + 1 = 11 265 samples spans every gap between the
    # spikes of these lengths) some were left alone
    assert sum(r["limited"] for r in refs) > 0 and (a == 1024 or any(r["limited"] < len(r["x"]) for r in refs))


# ---------------------------------------------------------------------------------------------------- 3. each signal is its own
def test_a_signal_alone_equals_the_signal_in_the_batch():
    a, h = 80, 800
    xs, outs, st, _ = batch(a, h)
    for k, x in enumerate(xs):
        y, s = A.master(cuda([x])[0], mastering(a, h), sample_rate=SR, return_stats=True)
        s = host(s)
        assert y.shape == (len(x),) and np.array_equal(y.cpu().numpy(), outs[k])
        for f in s:
            assert s[f].shape == (1,) and s[f][0] == st[f][k], (k, f)


def test_a_spike_does_not_reach_the_next_signal():
    a, h = 80, 800
    m = mastering(a, h)
    loud = M.signal(T + 300, a, h, seed=3, tile=T)                                 # ends on a spike of 384 c
    t = np.arange(3000)
    quiet = (0.3 * np.sin(2 * np.pi * 440.0 * t / SR)).astype(F32)                 # gain 2 (the cap): 0.6, below the ceiling
    out, stats = A.master(cuda([loud, quiet, loud[::-1].copy()]), m, sample_rate=SR, return_stats=True)
    st = host(stats)
    assert st["gain"][1] == F32(2.0) and st["limited"][1] == 0 and st["min_gain"][1] == F32(1.0)
    assert np.array_equal(out[1].cpu().numpy(), (F32(2.0) * quiet).astype(F32))
    assert st["limited"][0] > 0 and st["limited"][2] > 0


# ---------------------------------------------------------------------------------------------------- 4. identity
def test_no_gain_and_nothing_over_the_ceiling_is_the_identity():
    t = torch.arange(2 * T + 77, device="cuda", dtype=torch.float32)
    x = 0.8 * torch.sin(2 * np.pi * 55.0 * t / SR)
    m = A.Mastering(target_rms=None)
    out, st = A.master(x, m, return_stats=True)
    assert out.dtype == torch.float32 and out.data_ptr() != x.data_ptr() and torch.equal(out, x)
    assert st.limited.tolist() == [0] and st.min_gain.tolist() == [1.0] and st.gain.tolist() == [1.0] and st.limited.dtype == torch.int32
    assert st.peak.item() == x.abs().max().item()
    both = torch.stack([x, -x])                                                   # a (B, L) tensor keeps its shape, a list its lengths
    out2 = A.master(both, m)
    assert out2.shape == both.shape and torch.equal(out2, both)
    outs = A.master([x, x[:100]], m)
    assert isinstance(outs, list) and torch.equal(outs[0], x) and torch.equal(outs[1], x[:100])
    assert torch.equal(A.master(x.double(), m), x)                                # other dtypes are taken as fp32, like pitch_shift


# ---------------------------------------------------------------------------------------------------- 5. degenerate inputs
def test_max_gain_caps_a_quiet_signal_and_silence_stays_silence():
    t = np.arange(5000)
    quiet = (1e-4 * np.sin(2 * np.pi * 55.0 * t / SR)).astype(F32)
    out, st = A.master(cuda([quiet, np.zeros(T + 9, F32)]), A.Mastering(), return_stats=True)
    st = host(st)
    assert st["gain"].tolist() == [10.0, 10.0] and st["limited"].tolist() == [0, 0] and st["min_gain"].tolist() == [1.0, 1.0]
    assert np.array_equal(out[0].cpu().numpy(), (F32(10.0) * quiet).astype(F32))
    z = out[1].cpu().numpy()
    assert not np.isnan(z).any() and not z.any() and st["rms"][1] == 0.0 and st["peak"][1] == 0.0 and np.isfinite(st["rms"]).all()


# ---------------------------------------------------------------------------------------------------- 6. PCM
def test_pcm_is_the_rounding_of_the_same_calls_float_output():
    a, h = 80, 800
    m = mastering(a, h, ceiling=1.0)                                               # the largest ceiling: +-32767 is reached
    xs = [M.signal(n, a, h, ceiling=1.0, seed=k, tile=T) for k, n in enumerate((161, T + 1, 2 * T + 40))]
    lens = [len(x) for x in xs]
    x = torch.cat(cuda(xs))
    y, pcm, _, _ = launch(x, A._flat_table(lens), len(xs), max(lens), x.numel(), m, a, h)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, np.rint(y * F32(32767)).astype(np.int16))
    assert np.abs(pcm.astype(np.int32)).max() == 32767
    got = A.master(cuda(xs), m, sample_rate=SR, pcm16=True)                        # the public call: the same samples, the same container
    assert [g.dtype for g in got] == [torch.int16] * 3 and np.array_equal(torch.cat(got).cpu().numpy(), pcm)
    assert np.array_equal(torch.cat(A.master(cuda(xs), m, sample_rate=SR)).cpu().numpy(), y)


# ---------------------------------------------------------------------------------------------------- 7. bounds
def test_nothing_is_written_outside_the_fitting_signals():
    a, h = 80, 800
    m = mastering(a, h)
    xs = [M.signal(T + 1, a, h, seed=1, tile=T), M.signal(700, a, h, seed=2)]
    n0, n2 = len(xs[0]), len(xs[1])
    total = n0 + n2
    x = torch.cat(cuda(xs))
    want_y, want_pcm, want_st, want_lim = launch(x, A._flat_table([n0, n2]), 2, n0, total, m, a, h)
    tab = np.zeros((3, PV["DS_PV_NI"]), np.int32)
    tab[:, PV["DS_PV_XOFF"]] = (0, total - 10, n0)
    tab[:, PV["DS_PV_LEN"]] = (n0, 100, n2)                                        # the middle row ends 90 samples behind the buffer
    y, pcm, st, lim = launch(x, tab, 3, n0, total, m, a, h, pad=128)
    assert np.array_equal(y[:total], want_y) and np.array_equal(pcm[:total], want_pcm)
    assert (y[total:] == F32(-777.0)).all() and (pcm[total:] == -7).all() and len(y) == total + 128
    assert np.array_equal(st[[0, 2]], want_st) and np.array_equal(lim[[0, 2]], want_lim)
    assert (st[1] == F32(-777.0)).all() and lim[1] == -7                           # the row that does not fit wrote nothing at all


# ---------------------------------------------------------------------------------------------------- 8. wiring
def _tracks(max_notes=6):
    g = load_golden("arranger")
    name = "Ode_to_Joy_Easy_variation"
    msgs = [R.messages(g[f"{name}.t{k}.msgs"]) for k in range(2)]
    tmap = A.tempo_map_of(msgs)
    return [A.Track(t, int(g[name + ".tpb"]), max_notes, pairing="midi", tempo_map=tmap) for t in msgs]


def _notes(tracks, names, perform=None):
    return {(name, s[1]): torch.from_numpy(R.synthetic_note(s[1])).cuda() for name, t in zip(names, tracks) for s in t.schedule(perform=perform)}


def test_render_and_arrange_master_the_mix_once():
    tracks, names = _tracks(), ["organ", "string"]
    mst = A.Mastering()
    fn = lambda v, d: R.synthetic_note(d)                                          # noqa: E731
    t = tracks[0]
    plain = t.render(fn)
    assert t.last_master is None and torch.equal(t.render(fn, master=None), plain)
    got = t.render(fn, master=mst)
    want, stats = A.master(plain, mst, return_stats=True)
    assert torch.equal(got, want) and not torch.equal(got, plain)
    assert isinstance(t.last_master, A.MasterStats) and torch.equal(t.last_master.gain, stats.gain) and torch.equal(t.last_master.limited, stats.limited)
    for perform in (None, A.Performance()):
        notes = _notes(tracks, names, perform)
        ds = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi", perform=perform)
        base = ds.arrange(tracks, names, notes)
        assert ds.last_master is None and torch.equal(ds.arrange(tracks, names, notes, master=None), base)
        got = ds.arrange(tracks, names, notes, master=mst)
        want, stats = A.master(base, mst, return_stats=True)
        assert torch.equal(got, want) and not torch.equal(got, base) and got.abs().max().item() <= F32(mst.ceiling)
        assert all(torch.equal(p, q) for p, q in zip(ds.last_master, stats))
        pcm = ds.arrange(tracks, names, notes, master=mst, pcm16=True)
        assert pcm.dtype == torch.int16 and torch.equal(pcm, A.master(base, mst, pcm16=True))
        # the constructor's master holds for every call; the keyword of arrange overrides it for one
        other = A.Mastering(target_rms=None, ceiling=0.5)
        dm = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi", perform=perform, master=mst)
        assert torch.equal(dm.arrange(tracks, names, notes), got) and dm.last_master is not None
        assert torch.equal(dm.arrange(tracks, names, notes, master=other), A.master(base, other))
        assert torch.equal(dm.arrange(tracks, names, notes, master=None), base) and dm.last_master is None
