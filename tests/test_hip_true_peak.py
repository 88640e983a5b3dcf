"""The true-peak meter and the limiter with its envelope as detector on the GPU: ds_true_peak bit for bit against the float64 restatement
(tests/true_peak_ref.py) on one ragged launch that crosses every tile boundary, every signal its own, the meter alone, bounds;
master(true_peak=True) bit for bit against the restatement at the device's gain, TruePeak, the LUFS path and the order of the launches,
the untouched default, and the wiring through Track.render and DiffSynth.arrange.

No tolerance anywhere behind the gain: every product of the interpolator is exact in float64, the sum has one order and one rounding per
add on both sides, a maximum has no order and the rounding to fp32 is monotone.  The gain is held to one fp32 ulp as in
tests/test_hip_master.py (the order of its float64 sum is the device's own)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import arranger_ref as AR
import master_ref as M
import true_peak_ref as R
import diffusynth_amd
from conftest import load_golden
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

TM = importlib.import_module("diffusynth_amd.true_peak")         # (the package's attribute `true_peak` is the function)
pytestmark = pytest.mark.gpu
MS, PV, TP = L.MS, L.PV, L.TP
T, TMS, SR, F32 = TP["DS_TP_TILE"], MS["DS_MS_TILE"], 16000, np.float32
LENGTHS = [1, 2, 5, 6, 7, 11, 12, 13, T - 1, T, T + 1, 2 * T + 13, 2 ** 20 + 3001]
GAIN = dict(target_rms=3.0, max_gain=2.0)        # as tests/test_hip_master.py: with the test signal's spikes the detector stays far inside 2^18 c
CASES = [(0, 0), (1, 1), (80, 800), (1024, 8192)]
BOUND_DB = 0.01                                  # DESIGN §7r's condition on the output's true peak at the defaults


def cuda(xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def host(stats):
    return {k: getattr(stats, k).cpu().numpy() for k in stats._fields}


def meter_signal(n, seed):
    """Noise with spikes at the first sample, the last sample and on both sides of every tile boundary (alternating signs, different sizes:
    a tile that read its neighbour's halo wrongly moves the envelope there)."""
    rng = np.random.default_rng(100 + seed)
    x = (0.3 * rng.standard_normal(n)).astype(F32)
    for k in range(1, (n - 1) // T + 1):
        x[k * T - 1] = 3.0 + 0.01 * (k % 7)
        x[k * T] = -(2.0 + 0.01 * (k % 5))
    x[-1] = -4.5
    x[0] = 5.25
    return x


def launch(x, tab, n_signals, max_len, total, *, env=True, pad=0, fill=-777.0):
    """ds_true_peak on a caller's table: (env with `pad` extra elements or None, tp with one extra element), every buffer filled with a sentinel."""
    lib = L.load()
    dtab = torch.from_numpy(np.ascontiguousarray(tab, np.int32).reshape(-1)).cuda()
    ws = torch.full((max(1, lib.ds_true_peak_ws_bytes(n_signals, max_len) // 4),), fill, dtype=torch.float32, device="cuda")
    tp = torch.full((n_signals + 1,), fill, dtype=torch.float32, device="cuda")
    e = torch.full((total + pad,), fill, dtype=torch.float32, device="cuda") if env else None
    L.call("ds_true_peak", x.data_ptr(), dtab.data_ptr(), n_signals, max_len, total, TM.true_peak_coefficients().ctypes.data, L.ptr(e), ws.data_ptr(), tp.data_ptr(),
           L.current_stream())
    return None if e is None else e.cpu().numpy(), tp.cpu().numpy()


@functools.lru_cache(maxsize=None)
def ragged():
    """One ragged launch shared by the tests below: (signals, flat device tensor, table, env, tp, the restatement's envelopes)."""
    xs = [meter_signal(n, k) for k, n in enumerate(LENGTHS)]
    x = torch.cat(cuda(xs))
    tab = A._flat_table(LENGTHS)
    env, tp = launch(x, tab, len(xs), max(LENGTHS), x.numel(), pad=64)
    return xs, x, tab, env, tp, [R.envelope(v) for v in xs]


# ---------------------------------------------------------------------------------------------------- 1. the meter
def test_envelope_and_true_peak_equal_the_restatement_bit_for_bit():
    xs, x, tab, env, tp, refs = ragged()
    total = x.numel()
    assert len(env) == total + 64 and (env[total:] == F32(-777.0)).all() and tp[len(xs)] == F32(-777.0)      # the sentinels behind env and tp
    off = 0
    for k, (v, ref) in enumerate(zip(xs, refs)):
        got = env[off:off + len(v)]
        bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
        print(f"N = {len(v)}: true peak {tp[k]!r} / {ref.max()!r} (sample peak {np.abs(v).max()!r}), {len(bad)} envelope samples differ" +
              (f", first at {bad[0]}: {got[bad[0]]!r} / {ref[bad[0]]!r}" if len(bad) else ""))
        assert got.dtype == F32 and np.array_equal(got, ref) and tp[k] == ref.max() and (got >= np.abs(v)).all()
        off += len(v)
    assert any(r.max() > np.abs(v).max() for v, r in zip(xs, refs))                                   # the true peak is not the sample peak


def test_public_call_every_container_and_a_signal_alone():
    xs, x, tab, env, tp, refs = ragged()
    got_tp, got_env = diffusynth_amd.true_peak(cuda(xs), return_envelope=True)
    assert isinstance(got_env, list) and got_tp.dtype == torch.float32 and got_tp.shape == (len(xs),) and got_tp.is_cuda
    assert np.array_equal(got_tp.cpu().numpy(), tp[:len(xs)]) and np.array_equal(torch.cat(got_env).cpu().numpy(), env[:x.numel()])
    assert torch.equal(diffusynth_amd.true_peak(cuda(xs)), got_tp)
    for k, v in enumerate(xs):                                                     # each signal alone: the same bits as in the batch
        t1, e1 = diffusynth_amd.true_peak(cuda([v])[0], return_envelope=True)
        assert t1.shape == (1,) and e1.shape == (len(v),) and t1.item() == tp[k] and np.array_equal(e1.cpu().numpy(), refs[k]), k
    both = torch.stack(cuda([xs[9], -xs[9]]))                                      # a (B, L) tensor keeps its shape
    t2, e2 = diffusynth_amd.true_peak(both, return_envelope=True)
    assert e2.shape == both.shape and t2.tolist() == [tp[9], tp[9]] and torch.equal(e2[0], e2[1])
    assert torch.equal(diffusynth_amd.true_peak(both.double()), t2)                # other dtypes are taken as fp32, like master()


def test_meter_alone_gives_the_same_true_peak():
    xs, x, tab, env, tp, _ = ragged()
    none, tp2 = launch(x, tab, len(xs), max(LENGTHS), x.numel(), env=False)
    assert none is None and np.array_equal(tp2, tp)


def test_nothing_is_written_outside_the_fitting_signals():
    xs = [meter_signal(T + 1, 1), meter_signal(700, 2)]
    n0, n2 = len(xs[0]), len(xs[1])
    total = n0 + n2
    x = torch.cat(cuda(xs))
    want_env, want_tp = launch(x, A._flat_table([n0, n2]), 2, n0, total)
    tab = np.zeros((5, PV["DS_PV_NI"]), np.int32)
    tab[:, PV["DS_PV_XOFF"]] = (0, total - 10, n0, 0, -1)
    tab[:, PV["DS_PV_LEN"]] = (n0, 100, n2, n0 + 1, 5)             # row 1 ends 90 samples behind the buffer, row 3 is longer than max_len, row 4 starts before it
    env, tp = launch(x, tab, 5, n0, total, pad=128)
    assert np.array_equal(env[:total], want_env) and (env[total:] == F32(-777.0)).all() and len(env) == total + 128
    assert np.array_equal(tp[[0, 2]], want_tp[:2]) and (tp[[1, 3, 4, 5]] == F32(-777.0)).all()       # the rows that do not fit wrote nothing at all
    assert np.array_equal(want_env, np.concatenate([R.envelope(v) for v in xs]))


# ---------------------------------------------------------------------------------------------------- 2. the limiter
def mastering(a, h, **kw):
    m = A.Mastering(lookahead=(a + 0.5) / SR, hold=(h + 0.5) / SR, true_peak=True, **{**GAIN, **kw})
    assert m.samples(SR) == (a, h)
    return m


def lengths_of(a, h):
    return [1, TMS + 1, 2 * TMS + h + 3 * a + 5] if a == 1024 else [1, 2, 80, 161, TMS - 1, TMS, TMS + 1, 2 * TMS + h + 3 * a + 5]


def limiter_signal(n, a, h, seed):
    """master_ref's test signal plus an fs/4 burst at 45 degrees over its second quarter: there the waveform peaks between the samples,
    so the envelope and the samples disagree about what the limiter has to do."""
    x = M.signal(n, a, h, seed=seed, tile=TMS).astype(np.float64)
    t = np.arange(n)
    x += np.where((t >= n // 4) & (t < n // 2), 1.5, 0.0) * np.sin(2 * np.pi * t / 4.0 + np.pi / 4.0)
    return x.astype(F32)


@functools.lru_cache(maxsize=None)
def batch(a, h):
    xs = [limiter_signal(n, a, h, k) for k, n in enumerate(lengths_of(a, h))]
    m = mastering(a, h)
    out, stats, peaks = A.master(cuda(xs), m, sample_rate=SR, return_stats=True, return_true_peak=True)
    st = host(stats)
    refs = [R.master(x, a, h, gl=st["gain"][k], ceiling=m.ceiling, **GAIN) for k, x in enumerate(xs)]
    return xs, [o.cpu().numpy() for o in out], st, refs, peaks


@pytest.mark.parametrize("a,h", CASES, ids=[f"A{a}_R{h}" for a, h in CASES])
def test_limiter_equals_the_restatement_bit_for_bit(a, h):
    xs, outs, st, refs, peaks = batch(a, h)
    tp_in, tp_out = peaks.input.cpu().numpy(), peaks.output.cpu().numpy()
    assert isinstance(peaks, A.TruePeak) and peaks.input.dtype == torch.float32 and peaks.output.shape == (len(xs),)
    differ = 0
    for k, (x, y, ref) in enumerate(zip(xs, outs, refs)):
        d = (ref["gain"] * ref["env"]).astype(F32)
        assert d.max() <= 2 ** 18 * float(ref["c"]) and st["gain"][k] <= 2.0                          # inside the exactness range of the float64 sum
        assert M.ulps(st["gain"][k], ref["gain64"]) <= 1.0
        bad = np.flatnonzero(y.view(np.uint32) != ref["y"].view(np.uint32))
        plain = M.master(x, a, h, gl=st["gain"][k], ceiling=mastering(a, h).ceiling, **GAIN)
        differ += int(np.count_nonzero(plain["y"] != ref["y"]))
        print(f"A={a} R={h} N={len(x)}: gL {st['gain'][k]}, limited {st['limited'][k]} / {ref['limited']}, min g {st['min_gain'][k]} / {ref['min_gain']}, "
              f"true peak {tp_in[k]!r} -> {tp_out[k]!r} ({tp_out[k] / float(ref['c']):.6f} c), {len(bad)} samples differ" +
              (f", first at {bad[0]}: {y[bad[0]]!r} / {ref['y'][bad[0]]!r}" if len(bad) else ""))
        assert y.dtype == F32 and np.array_equal(y, ref["y"])
        assert st["min_gain"][k] == ref["min_gain"] and st["limited"][k] == ref["limited"] and st["limited"].dtype == np.int32
        assert np.abs(y).max() <= ref["c"]
        assert tp_in[k] == ref["tp_in"] and tp_out[k] == ref["tp_out"] == R.true_peak(y)              # TruePeak, bit for bit
    # not vacuous: samples were limited, and the envelope asked for something else than the samples would have
    assert sum(r["limited"] for r in refs) > 0 and differ > 0


def test_true_peak_of_the_output_is_inside_the_condition_at_the_defaults():
    fx = R.fixtures()
    m = A.Mastering(target_rms=None, true_peak=True)
    assert m.samples(SR) == (80, 800)
    c = F32(m.ceiling)
    out, stats, peaks = A.master(cuda(list(fx.values())), m, sample_rate=SR, return_stats=True, return_true_peak=True)
    sp = A.master(cuda(list(fx.values())), A.Mastering(target_rms=None), sample_rate=SR, return_true_peak=True)[1]
    for k, (name, x) in enumerate(fx.items()):
        ref = R.master(x, 80, 800, target_rms=None, ceiling=m.ceiling)
        y = out[k].cpu().numpy()
        over, over_sp = R.db(peaks.output[k].item() / float(c)), R.db(sp.output[k].item() / float(c))
        print(f"{name}: true peak {peaks.input[k].item():.4f} -> {peaks.output[k].item() / float(c):.6f} c = {over:+.5f} dB; sample-peak limiter {over_sp:+.3f} dB")
        assert np.array_equal(y, ref["y"]) and peaks.output[k].item() == ref["tp_out"] and peaks.input[k].item() == ref["tp_in"] and stats.gain[k].item() == 1.0
        assert np.abs(y).max() <= c and over <= BOUND_DB and over_sp > 0.1
        assert sp.input[k].item() == ref["tp_in"]                                  # measured for the report where the Mastering made no envelope


def test_pcm_and_true_peak_of_the_float_result():
    a, h = 80, 800
    xs = [limiter_signal(n, a, h, k) for k, n in enumerate((161, TMS + 1))]
    m = mastering(a, h)
    y, peaks = A.master(cuda(xs), m, sample_rate=SR, return_true_peak=True)
    pcm, peaks16 = A.master(cuda(xs), m, sample_rate=SR, pcm16=True, return_true_peak=True)
    assert [p.dtype for p in pcm] == [torch.int16] * 2 and torch.equal(peaks.output, peaks16.output) and torch.equal(peaks.input, peaks16.input)
    for p, v in zip(pcm, y):
        assert np.array_equal(p.cpu().numpy(), M.pcm16(v.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------- 3. with a LUFS target; the launches
def test_lufs_target_then_envelope_then_limiter(monkeypatch):
    import loudness_ref as LR
    x = LR.gating_fixture(SR)[:3 * SR].astype(np.float64)
    t = np.arange(len(x))
    x = (x + np.where((t >= SR) & (t < SR + 4000), 0.6, 0.0) * np.sin(2 * np.pi * t / 4.0 + np.pi / 4.0)).astype(F32)
    names = []
    call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    m = A.Mastering(target_rms=None, target_lufs=-6.0, true_peak=True)
    y, st, loud, peaks = A.master(cuda([x])[0], m, return_stats=True, return_loudness=True, return_true_peak=True)
    assert names == ["ds_master_gain", "ds_loudness", "ds_loudness_gain", "ds_true_peak", "ds_master_limit_tp", "ds_true_peak"]
    del names[:]
    y0, st0 = A.master(cuda([x])[0], A.Mastering(target_rms=None, target_lufs=-6.0), return_stats=True)
    assert names == ["ds_master_gain", "ds_loudness", "ds_loudness_gain", "ds_master_limit"]
    del names[:]
    A.master(cuda([x])[0], A.Mastering(true_peak=True))
    assert names == ["ds_master_gain", "ds_true_peak", "ds_master_limit_tp"]
    del names[:]
    A.master(cuda([x])[0], A.Mastering(), return_true_peak=True)
    assert names == ["ds_master_gain", "ds_master_limit", "ds_true_peak", "ds_true_peak"]
    g = st.gain.cpu().numpy()[0]
    assert g == st0.gain.cpu().numpy()[0] and g != 1.0 and g < 10.0                # the LUFS gain, whatever the detector
    a, r = m.samples(SR)
    ref = R.master(x, a, r, gl=g, target_rms=None, ceiling=m.ceiling)
    plain = M.master(x, a, r, gl=g, target_rms=None, ceiling=m.ceiling)
    print(f"gain {g!r}, limited {st.limited.item()} / {ref['limited']} (sample detector {plain['limited']}), true peak {peaks.input.item()!r} -> {peaks.output.item()!r}")
    assert np.array_equal(y.cpu().numpy(), ref["y"]) and st.limited.item() == ref["limited"] and st.min_gain.item() == ref["min_gain"]
    assert np.array_equal(y0.cpu().numpy(), plain["y"]) and ref["limited"] > plain["limited"] > 0
    assert peaks.input.item() == ref["tp_in"] and peaks.output.item() == ref["tp_out"]


# ---------------------------------------------------------------------------------------------------- 4. the default is untouched
def test_true_peak_false_is_the_call_that_never_heard_of_it():
    a, h = 80, 800
    xs = [limiter_signal(n, a, h, k) for k, n in enumerate((161, TMS + 1, 2 * TMS + 40))]
    kw = dict(lookahead=(a + 0.5) / SR, hold=(h + 0.5) / SR, **GAIN)
    y0, s0 = A.master(cuda(xs), A.Mastering(**kw), sample_rate=SR, return_stats=True)
    y1, s1 = A.master(cuda(xs), A.Mastering(true_peak=False, **kw), sample_rate=SR, return_stats=True)
    y2, s2, peaks = A.master(cuda(xs), A.Mastering(true_peak=False, **kw), sample_rate=SR, return_stats=True, return_true_peak=True)
    for k, x in enumerate(xs):
        ref = M.master(x, a, h, gl=s0.gain[k].item(), ceiling=A.Mastering().ceiling, **GAIN)      # ... and that is master_ref's: the old definition
        assert np.array_equal(y0[k].cpu().numpy(), ref["y"])
        assert torch.equal(y0[k], y1[k]) and torch.equal(y0[k], y2[k])
        assert peaks.input[k].item() == R.true_peak(x) and peaks.output[k].item() == R.true_peak(ref["y"])
    assert all(torch.equal(p, q) for p, q in zip(s0, s1)) and all(torch.equal(p, q) for p, q in zip(s0, s2)) and len(s0) == 5
    yt = A.master(cuda(xs), A.Mastering(true_peak=True, **kw), sample_rate=SR)
    assert not all(torch.equal(p, q) for p, q in zip(y0, yt))


# ---------------------------------------------------------------------------------------------------- 5. wiring
def test_render_and_arrange_master_to_a_true_peak_ceiling_once():
    g = load_golden("arranger")
    name = "Ode_to_Joy_Easy_variation"
    msgs = [AR.messages(g[f"{name}.t{k}.msgs"]) for k in range(2)]
    tmap = A.tempo_map_of(msgs)
    tracks = [A.Track(t, int(g[name + ".tpb"]), 6, pairing="midi", tempo_map=tmap) for t in msgs]
    names = ["organ", "string"]
    mst = A.Mastering(true_peak=True)
    fn = lambda v, d: AR.synthetic_note(d)                                         # noqa: E731
    t = tracks[0]
    plain = t.render(fn)
    assert t.last_true_peak is None
    got = t.render(fn, master=mst)
    want, stats, peaks = A.master(plain, mst, return_stats=True, return_true_peak=True)
    assert torch.equal(got, want) and not torch.equal(got, plain)
    assert isinstance(t.last_true_peak, A.TruePeak) and all(torch.equal(p, q) for p, q in zip(t.last_true_peak, peaks)) and torch.equal(t.last_master.gain, stats.gain)
    assert t.last_loudness is None and peaks.output.item() == R.true_peak(want.cpu().numpy()) and peaks.input.item() == R.true_peak(plain.cpu().numpy())
    t.render(fn, master=A.Mastering())
    assert t.last_true_peak is None and t.last_master is not None                  # a sample-peak master: no true peak was measured
    notes = {(nm, s[1]): torch.from_numpy(AR.synthetic_note(s[1])).cuda() for nm, tr in zip(names, tracks) for s in tr.schedule()}
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi")
    base = ds.arrange(tracks, names, notes)
    assert ds.last_true_peak is None
    got = ds.arrange(tracks, names, notes, master=mst)
    want, stats, peaks = A.master(base, mst, return_stats=True, return_true_peak=True)
    assert torch.equal(got, want) and all(torch.equal(p, q) for p, q in zip(ds.last_master, stats)) and all(torch.equal(p, q) for p, q in zip(ds.last_true_peak, peaks))
    assert got.abs().max().item() <= F32(mst.ceiling)
    pcm = ds.arrange(tracks, names, notes, master=mst, pcm16=True)
    assert pcm.dtype == torch.int16 and torch.equal(pcm, A.master(base, mst, pcm16=True)) and torch.equal(ds.last_true_peak.output, peaks.output)
    both = A.Mastering(target_rms=None, target_lufs=-18.0, true_peak=True)
    got = ds.arrange(tracks, names, notes, master=both)
    assert torch.equal(got, A.master(base, both)) and ds.last_loudness is not None and ds.last_true_peak is not None
    dm = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi", master=mst)
    assert torch.equal(dm.arrange(tracks, names, notes), want) and dm.last_true_peak is not None
    assert torch.equal(dm.arrange(tracks, names, notes, master=None), base) and dm.last_true_peak is None
