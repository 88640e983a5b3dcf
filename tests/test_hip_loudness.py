"""The loudness meter on the GPU (ds_loudness, ds_loudness_gain) against the sequential restatement (tests/loudness_ref.py):
exact counts, block energies and the gated energy to a tolerance of float64 rounding order, the logarithms, every signal its own, bounds,
and Mastering(target_lufs=) through master(), Track.render and DiffSynth.arrange.

The tolerances.  The device and the restatement compute the same float64 recursion in another order (chunks from zero state plus carried
states against one pass), so they differ by rounding alone.  Measured on these fixtures (printed by the tests): block energies and Z within
Z_MEASURED = 1.6e-10 (relative) of the restatement: the blocks of the gating fixture's -80 dB stretch, whose outputs are 2000 times smaller
than the DC offset the high-pass holds in its state (elsewhere 4e-14 at 16 kHz, 2.4e-12 at 44.1 and 48 kHz, where the poles lie closer to
the unit circle); Z itself 2.3e-12 at the most.  Z_TOL is four times that, below the 1e-9 above which the carry itself would be wrong.
After a LUFS gain with an idle limiter the output's loudness is within LU_MEASURED = 1.3e-7 LU of the target (the gain is rounded to fp32
once, which alone can cost 5e-7 LU, and the output sample by sample); LU_TOL is four times that."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import loudness_ref as R
import master_ref as M
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

LM = importlib.import_module("diffusynth_amd.loudness")
pytestmark = pytest.mark.gpu
LU, PV, MS, F32 = L.LU, L.PV, L.MS, np.float32
Z_MEASURED, LU_MEASURED = 1.6e-10, 1.3e-7
Z_TOL, LU_TOL = 4 * Z_MEASURED, 4 * LU_MEASURED
assert Z_TOL <= 1e-9 and LU_TOL <= 1e-3


def cuda(xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def lengths_of(fs):
    h = R.hop(fs)
    lc, _, _ = LM.chunking(h)
    if fs != 16000:
        return [4 * h, 6 * h + 11, 9 * h + 3 * lc + 7]
    return [1, 4 * h - 1, 4 * h, 4 * h + 1, 5 * h - 1, 5 * h, lc - 1, lc, lc + 1, 3 * lc + 7, 6 * h + lc + 1, 9 * h + 3 * lc + 7, 2 ** 20 + 3001]


def launch(xs, fs, *, tab=None, total=None, pad=0, blocks=True, total_blocks=None):
    """ds_loudness on a caller's table -> (lu, cnt, block energies with `pad` more entries, offsets, counts), sentinels in every output."""
    lens = [len(x) for x in xs]
    x = torch.cat(cuda(xs))
    h = R.hop(fs)
    if tab is None:
        tab = A._flat_table(lens)
        LM.layout(tab, lens, h)
    n = len(tab)
    lens = tab[:, PV["DS_PV_LEN"]].tolist()
    nbs = [max(0, m // h - 3) for m in lens]
    total = x.numel() if total is None else total
    tb = max(1, sum(nbs)) if total_blocks is None else total_blocks
    dtab = torch.from_numpy(np.ascontiguousarray(tab, np.int32).reshape(-1)).cuda()
    lib = L.load()
    ws = torch.full((max(1, lib.ds_loudness_ws_bytes(n, max(lens), h) // 8),), math.nan, dtype=torch.float64, device="cuda")
    lu = torch.full((n + 1, LU["DS_LU_NS"]), -777.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((n + 1, 3), -7, dtype=torch.int32, device="cuda")
    bl = torch.full((tb + pad,), -777.0, dtype=torch.float64, device="cuda") if blocks else None
    L.call("ds_loudness", x.data_ptr(), dtab.data_ptr(), n, max(lens), total, LM._coefficients(fs).ctypes.data, h, LM.Z_ABS, ws.data_ptr(), lu.data_ptr(), cnt.data_ptr(),
           L.ptr(bl), tb if blocks else 0, L.current_stream())
    return lu.cpu().numpy(), cnt.cpu().numpy(), None if bl is None else bl.cpu().numpy(), tab[:, LU["DS_LU_TAB_BOFF"]].tolist(), nbs


@functools.lru_cache(maxsize=None)
def signals(fs):
    xs = [R.noise(n, k, fs=fs) for k, n in enumerate(lengths_of(fs))]
    if fs == 16000:
        xs.insert(5, R.gating_fixture())
    return xs


@functools.lru_cache(maxsize=None)
def batch(fs):
    """One ragged launch per rate, shared by the tests below: (signals, lu, cnt, block energies per signal, the restatement of every signal)."""
    xs = signals(fs)
    lu, cnt, bl, boffs, nbs = launch(xs, fs)
    return xs, lu, cnt, [bl[o:o + m] for o, m in zip(boffs, nbs)], [R.loudness(x, fs) for x in xs]


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else (0.0 if a == 0 else math.inf)


# ---------------------------------------------------------------------------------------------------- 1. energies and counts
@pytest.mark.parametrize("fs", [16000, 11025, 44100, 48000])
def test_counts_are_exact_and_energies_equal_the_restatement(fs):
    xs, lu, cnt, bls, refs = batch(fs)
    worst = 0.0
    for k, (x, r) in enumerate(zip(xs, refs)):
        z = bls[k]
        ez = float(np.max(np.abs(z / r["z"] - 1.0))) if r["nb"] else 0.0
        eZ = rel(lu[k, LU["DS_LU_ENERGY"]], r["Z"])
        near = min([abs(v / t - 1.0) for v in r["z"] for t in (R.Z_ABS, r["z_rel"]) if t > 0], default=math.inf)
        print(f"{fs} Hz N = {len(x)}: blocks {cnt[k].tolist()} / {[r['nb'], r['n1'], r['n2']]}, z_j off {ez:.2e}, Z off {eZ:.2e}, L {lu[k, LU['DS_LU_INTEGRATED']]:.6f}, "
              f"nearest block {near:.1e} from a gate")
        assert near > 1e-6                                                         # the fixture's condition: the decisions cannot differ
        assert cnt[k].tolist() == [r["nb"], r["n1"], r["n2"]] and len(z) == r["nb"] and cnt.dtype == np.int32
        assert ez <= Z_TOL and eZ <= Z_TOL
        worst = max(worst, ez, eZ)
    print(f"{fs} Hz: worst relative difference {worst:.2e} (tolerance {Z_TOL:.1e})")
    assert (lu[-1] == -777.0).all() and (cnt[-1] == -7).all()                      # nothing behind the last row
    if fs == 16000:                                                                # the cases are not vacuous
        assert [r["nb"] for r in refs[:5]] == [0, 0, 1, 1, 1] and refs[5]["nb"] - refs[5]["n1"] >= 1 and refs[5]["n1"] - refs[5]["n2"] >= 1
        assert refs[-1]["nb"] == (2 ** 20 + 3001) // 1600 - 3


def test_loudness_threshold_and_momentary_maximum_follow_the_device_energies():
    for fs in (16000, 48000):
        xs, lu, cnt, bls, refs = batch(fs)
        for k, z in enumerate(bls):
            Z = lu[k, LU["DS_LU_ENERGY"]]
            j1 = [v for v in z.tolist() if v > R.Z_ABS]
            want = (R.lufs(Z), max([R.lufs(v) for v in z.tolist()], default=-math.inf), R.lufs(0.1 * R.mean(j1)))
            got = (lu[k, LU["DS_LU_INTEGRATED"]], lu[k, LU["DS_LU_MOMENTARY_MAX"]], lu[k, LU["DS_LU_THRESHOLD"]])
            for g, w in zip(got, want):
                assert (g == w) if math.isinf(w) else abs(g - w) <= 1e-8, (fs, k, got, want)


# ---------------------------------------------------------------------------------------------------- 2. each signal is its own
def test_a_signal_alone_equals_the_signal_in_the_batch():
    xs, lu, cnt, bls, _ = batch(16000)
    for k, x in enumerate(xs):
        lu1, cnt1, bl1, _, nbs = launch([x], 16000)
        assert np.array_equal(lu1[0], lu[k]) and np.array_equal(cnt1[0], cnt[k]) and np.array_equal(bl1[:nbs[0]], bls[k]), k
    # the public call: the same values, as device tensors, and the momentary curve
    res, curves = LM.loudness(cuda(xs[4:7]), 16000, return_blocks=True)
    assert isinstance(res, LM.Loudness) and res.integrated.dtype == torch.float64 and res.blocks.dtype == torch.int32 and res.integrated.is_cuda
    assert torch.equal(res.integrated.cpu(), torch.from_numpy(lu[4:7, LU["DS_LU_INTEGRATED"]].copy()))
    assert torch.equal(res.momentary_max.cpu(), torch.from_numpy(lu[4:7, LU["DS_LU_MOMENTARY_MAX"]].copy()))
    assert torch.equal(res.threshold.cpu(), torch.from_numpy(lu[4:7, LU["DS_LU_THRESHOLD"]].copy()))
    assert res.blocks.tolist() == cnt[4:7, 0].tolist() and res.gated.tolist() == cnt[4:7, 2].tolist()
    for c, z in zip(curves, bls[4:7]):
        assert c.dtype == torch.float64 and c.shape == (len(z),)
        np.testing.assert_allclose(c.cpu().numpy(), -0.691 + 10.0 * np.log10(z), rtol=0, atol=1e-9)
    one = LM.loudness(cuda([xs[5]])[0], 16000)
    assert one.integrated.shape == (1,) and one.integrated.item() == lu[5, LU["DS_LU_INTEGRATED"]]
    two = LM.loudness(torch.stack(cuda([xs[5], -xs[5]])))                          # a (B, L) tensor; a sign changes nothing
    assert two.integrated.tolist() == [lu[5, LU["DS_LU_INTEGRATED"]]] * 2


def test_a_signal_without_a_block_reads_minus_infinity_and_keeps_its_gain():
    xs, lu, cnt, _, _ = batch(16000)
    for k in (0, 1, 7, 8, 9, 10):
        assert cnt[k].tolist() == [0, 0, 0] and lu[k, LU["DS_LU_ENERGY"]] == 0.0
        assert lu[k, LU["DS_LU_INTEGRATED"]] == -math.inf and lu[k, LU["DS_LU_MOMENTARY_MAX"]] == -math.inf and lu[k, LU["DS_LU_THRESHOLD"]] == -math.inf
    m = A.Mastering(target_rms=None, target_lufs=-14.0, ceiling=1.0)
    silent = np.zeros(8 * 1600, F32)                                               # blocks, none above the absolute gate
    short = (0.5 * xs[1]).astype(F32)                                              # 4 h - 1 samples, |x| < 1
    out, st, loud = A.master(cuda([short, silent, xs[5]]), m, return_stats=True, return_loudness=True)
    assert st.gain.tolist()[:2] == [1.0, 1.0] and st.gain.tolist()[2] != 1.0
    assert loud.integrated.tolist()[:2] == [-math.inf, -math.inf] and loud.blocks.tolist() == [0, 5, len(xs[5]) // 1600 - 3] and loud.gated.tolist()[:2] == [0, 0]
    assert np.array_equal(out[0].cpu().numpy(), short) and not out[1].any().item()  # |x| < 1 = the ceiling: a gain of 1 is the identity


# ---------------------------------------------------------------------------------------------------- 3. bounds
def test_nothing_is_written_outside_the_fitting_signals():
    xs = [signals(16000)[k] for k in (5, 11)]
    n0, n2 = len(xs[0]), len(xs[1])
    total = n0 + n2
    want_lu, want_cnt, want_bl, _, nbs = launch(xs, 16000)
    tab = np.zeros((4, PV["DS_PV_NI"]), np.int32)
    tab[:, PV["DS_PV_XOFF"]] = (0, total - 10, n0, 0)
    tab[:, PV["DS_PV_LEN"]] = (n0, 8000, n2, n0)                                   # row 1 ends behind the samples, row 3's blocks behind theirs
    tab[:, LU["DS_LU_TAB_BOFF"]] = (0, 0, nbs[0], nbs[0] + nbs[1] - 3)
    lu, cnt, bl, _, _ = launch(xs, 16000, tab=tab, total=total, pad=64, total_blocks=nbs[0] + nbs[1])
    assert np.array_equal(lu[[0, 2]], want_lu[:2]) and np.array_equal(cnt[[0, 2]], want_cnt[:2])
    assert np.array_equal(bl[:nbs[0] + nbs[1]], want_bl[:nbs[0] + nbs[1]]) and (bl[nbs[0] + nbs[1]:] == -777.0).all() and len(bl) == nbs[0] + nbs[1] + 64
    assert (lu[[1, 3, 4]] == -777.0).all() and (cnt[[1, 3, 4]] == -7).all()          # the rows that do not fit wrote nothing at all
    lu2, cnt2, none, _, _ = launch(xs, 16000, blocks=False)                         # without the block energies: the same results
    assert none is None and np.array_equal(lu2, want_lu) and np.array_equal(cnt2, want_cnt)


# ---------------------------------------------------------------------------------------------------- 4. master() to a LUFS target
def device_energy(x, fs=16000):
    lu, _, _, _, _ = launch([x], fs, blocks=False)
    return float(lu[0, LU["DS_LU_ENERGY"]])


def test_master_applies_the_exact_gain_and_the_limiter_of_the_restatement():
    x = signals(16000)[5]                                                          # the gating fixture: about -12.6 LUFS, peaks near 0.9
    for target, max_gain, capped in ((-16.0, 10.0, False), (-3.0, 2.0, True), (-9.0, 10.0, False)):
        m = A.Mastering(target_rms=None, target_lufs=target, max_gain=max_gain)
        a, r = m.samples(16000)
        y, st, loud = A.master(cuda([x])[0], m, return_stats=True, return_loudness=True)
        g = st.gain.cpu().numpy()[0]
        Z = device_energy(x)
        want_g = R.gain(Z, target, max_gain)
        ref = M.master(x, a, r, gl=g, target_rms=None, max_gain=max_gain, ceiling=m.ceiling)
        print(f"target {target} LUFS, max_gain {max_gain}: gain {g!r} / {want_g!r}, limited {st.limited.item()} / {ref['limited']}, input {loud.integrated.item():.4f} LUFS")
        assert g.dtype == F32 and g == want_g and (g == F32(max_gain)) == capped
        assert np.array_equal(y.cpu().numpy(), ref["y"]) and st.limited.item() == ref["limited"] and st.min_gain.item() == ref["min_gain"]
        assert st.peak.item() == ref["peak"] and M.ulps(st.rms.item(), ref["rms"]) <= 1.0
        assert loud.integrated.item() == R.lufs(Z) or abs(loud.integrated.item() - R.lufs(Z)) <= 1e-8
    assert ref["limited"] > 0                                                      # -9 LUFS from -12.6: the peaks cross the ceiling


def test_master_reaches_the_target_where_the_limiter_is_idle():
    worst = 0.0
    for k, target in ((5, -20.0), (11, -23.0), (13, -18.0)):
        x = signals(16000)[k]
        m = A.Mastering(target_rms=None, target_lufs=target, max_gain=10.0)
        y, st = A.master(cuda([x])[0], m, return_stats=True)
        assert st.limited.item() == 0 and st.gain.item() < 10.0
        got = LM.loudness(y, 16000).integrated.item()
        print(f"N = {len(x)}: target {target} LUFS, gain {st.gain.item()!r}, output {got:.7f} LUFS, off {abs(got - target):.2e} LU")
        worst = max(worst, abs(got - target))
        assert abs(got - target) <= LU_TOL
    print(f"worst distance from the target {worst:.2e} LU (tolerance {LU_TOL:.1e})")


def test_master_without_a_target_lufs_is_unchanged_and_can_still_report_the_loudness():
    x = cuda([signals(16000)[5]])[0]
    m = A.Mastering()
    y0, s0 = A.master(x, m, return_stats=True)
    y1, s1, loud = A.master(x, m, return_stats=True, return_loudness=True)
    assert torch.equal(y0, y1) and all(torch.equal(p, q) for p, q in zip(s0, s1))
    assert torch.equal(loud.integrated, LM.loudness(x).integrated)
    y2, loud2 = A.master(x, m, return_loudness=True)
    assert torch.equal(y2, y0) and torch.equal(loud2.integrated, loud.integrated)


# ---------------------------------------------------------------------------------------------------- 5. wiring
def test_render_and_arrange_master_to_the_target_once():
    import arranger_ref as AR
    from conftest import load_golden
    g = load_golden("arranger")
    name = "Ode_to_Joy_Easy_variation"
    msgs = [AR.messages(g[f"{name}.t{k}.msgs"]) for k in range(2)]
    tmap = A.tempo_map_of(msgs)
    tracks = [A.Track(t, int(g[name + ".tpb"]), 6, pairing="midi", tempo_map=tmap) for t in msgs]
    names = ["organ", "string"]
    mst = A.Mastering(target_rms=None, target_lufs=-18.0)
    fn = lambda v, d: AR.synthetic_note(d)                                         # noqa: E731
    t = tracks[0]
    plain = t.render(fn)
    assert t.last_loudness is None
    got = t.render(fn, master=mst)
    want, stats, loud = A.master(plain, mst, return_stats=True, return_loudness=True)
    assert torch.equal(got, want) and not torch.equal(got, plain)
    assert isinstance(t.last_loudness, LM.Loudness) and torch.equal(t.last_loudness.integrated, loud.integrated) and torch.equal(t.last_master.gain, stats.gain)
    assert math.isfinite(loud.integrated.item())
    t.render(fn, master=A.Mastering())
    assert t.last_loudness is None and t.last_master is not None                   # an RMS master: no loudness was measured
    notes = {(nm, s[1]): torch.from_numpy(AR.synthetic_note(s[1])).cuda() for nm, tr in zip(names, tracks) for s in tr.schedule()}
    ds = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi")
    base = ds.arrange(tracks, names, notes)
    assert ds.last_loudness is None
    got = ds.arrange(tracks, names, notes, master=mst)
    want, stats, loud = A.master(base, mst, return_stats=True, return_loudness=True)
    assert torch.equal(got, want) and all(torch.equal(p, q) for p, q in zip(ds.last_master, stats)) and all(torch.equal(p, q) for p, q in zip(ds.last_loudness, loud))
    pcm = ds.arrange(tracks, names, notes, master=mst, pcm16=True)
    assert pcm.dtype == torch.int16 and torch.equal(pcm, A.master(base, mst, pcm16=True))
    dm = A.DiffSynth({}, None, None, None, None, None, "cuda", pairing="midi", master=mst)
    assert torch.equal(dm.arrange(tracks, names, notes), got) and dm.last_loudness is not None
    assert torch.equal(dm.arrange(tracks, names, notes, master=None), base) and dm.last_loudness is None
