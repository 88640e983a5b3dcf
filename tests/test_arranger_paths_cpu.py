"""What tests/test_hip_arranger_paths.py rests on, shown without a GPU (tests/arranger_paths_ref.py):

  the table builder restates arranger._Plan, the mixer's lists restate arranger.mix_lists, the restatements on a caller's tables equal
  tests/arranger_ref.py on ordinary tables;
  the case list reaches every path the issue names (the geometry restatement says which path a shortened list would leave dark);
  8 x the float32 twin stays below the rule's cap of 1e-3 in every case, so the cap never decides;
  each deliberate fault, applied to the float64 restatement's output, exceeds the bound of its measure at least ten times: the tests can
  fail.  For the two faults in the upper half of the spectrum the whole-tensor measure of tests/test_hip_arranger.py on probe_signal is
  recorded beside the new one."""
import numpy as np
import pytest

import arranger_paths_ref as P
import arranger_ref as R
from conftest import rel_errs
from diffusynth_amd import arranger as A

MARGIN = 10.0


# ------------------------------------------------------------------------------------------------- builder, lists, restatements
@pytest.mark.parametrize("lengths,steps", [(P.STFT_LENGTHS, P.VOC_STEPS), tuple(zip(*P.ISTFT_CASES)), tuple(zip(*[c for c in P.RS_CASES if c != (1, -12)])),       # (the plan refuses a stretched length of 0; the kernel takes it)
                                           ((28416, 77568, 30001, 4097), (1, 2, -3, 0.5))], ids=["stft", "istft", "resample", "workload"])
def test_the_builder_restates_the_plan(lengths, steps):
    t, p = P.build(lengths, steps, gap=0), A._Plan(list(lengths), list(steps))
    assert np.array_equal(P.packed(t), p.host) and P.packed(t).dtype == p.host.dtype
    for f in ("n", "total_samples", "total_frames", "total_out", "total_stretched", "max_len", "max_frames", "max_out", "max_stretched"):
        assert getattr(t, f) == getattr(p, f), f
    g = P.build(lengths, steps)                                                  # the gaps move XOFF and SOFF, nothing else
    for f in P.FIELDS:
        if f not in ("XOFF", "SOFF"):
            assert P.col(g, f) == P.col(t, f), f
    assert P.col(g, "XOFF") == [o + P.GAP * s for s, o in enumerate(P.col(t, "XOFF"))]
    assert P.col(g, "SOFF") == [o + P.GAP * s for s, o in enumerate(P.col(t, "SOFF"))]
    assert g.total_samples == t.total_samples + P.GAP * (t.n - 1) and g.total_stretched == t.total_stretched + P.GAP * (t.n - 1)


def test_the_builder_lets_the_caller_change_a_field():
    def fix(s, row):
        if s == 1:
            row["SLEN"] = P.coverage_end(row["NOUT"]) + 300
    t, u = P.build((2048, 3072, 1024), (4, 4, 4)), P.build((2048, 3072, 1024), (4, 4, 4), fix=fix)
    grow = P.col(u, "SLEN")[1] - P.col(t, "SLEN")[1]
    assert grow > 300 and P.col(u, "SOFF")[2] == P.col(t, "SOFF")[2] + grow and u.total_stretched == t.total_stretched + grow
    assert u.max_stretched == P.col(u, "SLEN")[1]


@pytest.mark.parametrize("track_len", P.MIX_TRACKS)
def test_the_mixer_lists_restate_mix_lists_and_the_walk_is_numpy(track_len):
    notes, events = P.mix_case(track_len)
    flat, ev, ptr, lst = P.mix_tables(notes, events, track_len)
    ptr2, lst2 = A.mix_lists(ev[:, 0].tolist(), ev[:, 2].tolist(), track_len)
    assert np.array_equal(ptr, ptr2) and np.array_equal(lst, lst2)
    assert all(s >= 0 and s + len(notes[i]) <= track_len for s, i in events)
    want = P.mix_numpy(notes, events, track_len)
    got, touched = P.mix_walk(flat, ev, ptr, lst, len(lst), track_len)
    assert np.array_equal(got, want) and not touched
    zero, _ = P.mix_walk(flat, ev, ptr, lst, 0, track_len)
    assert not zero.any()


def test_mix_cases_hold_what_the_issue_lists():
    starts, ends, ones, depth = set(), set(), 0, 0
    for n in P.MIX_TRACKS:
        notes, events = P.mix_case(n)
        cover = np.zeros(n, int)
        for s, i in events:
            starts.add(s)
            ends.add((s + len(notes[i]) == n))
            ones += len(notes[i]) == 1
            cover[s:s + len(notes[i])] += 1
        depth = max(depth, cover.max())
    assert {0, 1023, 1024} <= starts and True in ends and ones > 0 and depth >= 3


def test_restatements_on_ordinary_tables_equal_arranger_ref():
    c = P.voc_case()
    for s in (0, 4, 8):
        nf = c.specs[s].shape[0]
        i0, al = R.time_steps(nf, c.t.rates[s])
        for dt in (np.float64, np.float32):
            assert np.array_equal(P.vocode(c.specs[s], i0, al, dt), R.phase_vocoder(c.specs[s], c.t.rates[s], dt) if dt == np.float32 else
                                  R.phase_vocoder(c.specs[s].astype(np.complex128), c.t.rates[s]))
    k = P.istft_case()
    for s in range(k.t.n):
        v = k.vocs[s].astype(np.complex128)
        got = P.overlap_add(P.synthesis_frames(v), len(k.want[s]))
        assert np.abs(got - k.want[s]).max() <= 1e-12 * np.abs(k.want[s]).max()
    y = P.noise(300, 1)
    assert np.array_equal(P.resample_left(y, 0.8, 200, np.zeros(80)), R.resample(y, 0.8, 200))


# ------------------------------------------------------------------------------------------------- the case list reaches every path
def test_stft_cases_reach_every_path():
    t = P.stft_case().t
    assert P.col(t, "NF") == [1, 1, 2, 2, 2, 3, 4, 5, 6]
    blocks = P.frame_blocks(t, "stft")
    assert {two for _, _, why, two in blocks if why is None} == {True, False}              # both halves of the two-frame trick
    assert any(why == "past the signal's frames" for _, _, why, _ in blocks)              # blocks of short signals exit
    assert {nf % 2 for nf in P.col(t, "NF")} == {0, 1}
    assert any(s < t.n - 1 for s in range(t.n)) and P.col(t, "XOFF")[1] == 1 + P.GAP        # a gap behind every signal but the last
    assert P.col(t, "XOFF")[-1] + P.col(t, "LEN")[-1] == t.total_samples                   # the last ends at the slab's guard


def test_vocode_cases_reach_every_path():
    t = P.voc_case().t
    rows = P.vocode_rows(t)
    assert all(why is None for _, why, _ in rows) and {m for _, _, m in rows} == {0, 1, 2, 3}, "nout % PV_U"
    assert set(t.steps) == {4, -3, 0.5, 1}
    assert max(P.col(t, "NOUT")) > P.PV_U                                                  # more than one trip of the unrolled loop
    c = P.voc_case()
    assert any((w == 0).any() for w in c.want) and all(np.isfinite(w).all() for w in c.want)
    idx = P.caller_steps(6, 8)
    assert {-2, -1, 5, 6, 11} <= set(idx.tolist())
    for s in c.specs:                                                                      # the scale test: nothing leaves the normal range
        a = np.abs(np.concatenate([s.real.ravel(), s.imag.ravel()])).astype(np.float64)
        a = a[a > 0]
        assert a.max() * 2.0 ** 100 < 2.0 ** 127 and a.min() * 2.0 ** -100 >= P.TINY32 and a.max() ** 2 * 2.0 ** 200 > 3.5e38


def test_istft_cases_reach_every_path():
    t = P.istft_case().t
    assert P.col(t, "NOUT") == [1, 2, 3, 4, 5, 6, 7, 8]
    blocks = P.frame_blocks(t, "istft")
    assert {two for _, _, why, two in blocks if why is None} == {True, False} and any(why for _, _, why, _ in blocks)
    counts = set()
    for nout, slen in zip(P.col(t, "NOUT"), P.col(t, "SLEN")):
        assert slen <= P.coverage_end(nout)
        counts |= set(P.ola_counts(nout, slen)[0].tolist())
    assert counts == {1, 2, 3, 4}
    long = P.ola_counts(3, P.coverage_end(3) + 300)[0]                                    # the caller's table: 300 samples no frame covers
    assert (long[-300:] == 0).all() and (long[:-300] > 0).all()
    assert any(ex for _, _, ex in P.ola_blocks(t)) and not all(ex for _, _, ex in P.ola_blocks(t))


def test_resample_cases_reach_every_path():
    t = P.rs_case().t
    assert len(P.RS_CASES) == 48 and sorted(set(P.col(t, "LEN"))) == list(P.RS_LENGTHS)
    assert any(r < 1 for r in t.rates) and any(r > 1 for r in t.rates) and any(r == 1.0 for r in t.rates)
    ks, left, right, natural = set(), False, False, []
    for s, (ln, slen, nres, rate) in enumerate(zip(P.col(t, "LEN"), P.col(t, "SLEN"), P.col(t, "NRES"), t.rates)):
        le, ri, tail, K = P.resample_edges(ln, slen, nres, rate)
        ks.add(K)
        left, right = left or le.any(), right or ri.any()
        assert tail.any() == (nres < ln)
        if nres < ln:
            natural.append(P.RS_CASES[s])
        assert P.resample_edges(ln, slen, ln - 7, rate)[2].sum() == min(7, ln)            # the caller's tables: a zero tail in every row
    # the plan's own zero tails, all at rate 2: round() goes to the even neighbour, so round(257 / 2) * 2 = 256 (1025, 2049 alike; 1 -> 0)
    assert natural == [(1, -12), (257, -12), (1025, -12), (2049, -12)]
    assert P.col(t, "SLEN")[P.RS_CASES.index((1, -12))] == 0                               # a stretched length of 0: every tap dropped
    assert ks == {35, 37, 44, 69} and left and right                                        # 69 taps a side at rate 1 / 2, 35 at rates >= 1
    blocks = P.resample_blocks(t)
    assert any(why == "past the signal" for _, _, why in blocks) and any(why is None and bx > 0 for _, bx, why in blocks)


def test_peak_cases_reach_every_path():
    assert [P.peak_blocks(n) for n in (1, 4096, 4097, 64 * 4096, 64 * 4096 + 1, max(P.PEAK_LENGTHS))] == [1, 1, 2, 64, 64, 64]
    nb = P.peak_blocks(max(P.PEAK_LENGTHS))
    assert (max(P.PEAK_LENGTHS) + 4095) // 4096 > nb == P.PN_NB_MAX                          # the clamp decides
    assert all(p is not None for p in P.peak_positions(max(P.PEAK_LENGTHS), nb))            # the long signal has all six places
    assert max(P.PEAK_LENGTHS) > 2 * nb * 256                                              # a third trip of the strided loop
    for v in range(6):
        for x in P.peak_batch(v):
            assert np.abs(x).max() == P.PEAK_SPIKE and (np.abs(x) == P.PEAK_SPIKE).sum() == 1
    assert P.peak_batch(0)[2].min() == -P.PEAK_SPIKE


# ------------------------------------------------------------------------------------------------- the cap never decides
def _twin_figures():
    c, v, k, r = P.stft_case(), P.voc_case(), P.istft_case(), P.rs_case()
    yield "stft", max(P.pair_errors(t, w).max() for t, w in zip(c.twin, c.want))
    yield "vocode", max(P.bin_errors(t, w).max() for t, w in zip(v.twin, v.want))
    yield "istft", max(P.signal_error(t, w) for t, w in zip(k.twin, k.want))
    yield "resample", max(P.signal_error(t, w) for t, w in zip(r.twin, r.want))


def test_eight_times_the_twin_stays_below_the_cap():
    for what, fig in _twin_figures():
        print(f"{what}: twin {fig:.2e}, 8 x twin {8 * fig:.2e}")
        assert 0 < 8 * fig < 1e-3, what
    v = P.voc_case()
    assert all(P.zeros_match(t, w) for t, w in zip(v.twin, v.want))


# ------------------------------------------------------------------------------------------------- the tests can fail
def _old_measure(fault):
    """What the whole-tensor measure of tests/test_hip_arranger.py gives for the same fault on probe_signal."""
    want = R.stft(R.probe_signal(5121, seed=10))
    return max(rel_errs(P.pairs(fault(want.copy())), P.pairs(want)))


def _nyquist_from_2047(S):
    S[:, 2048] = S[:, 2047]
    return S


def _odd_from_even_above_1024(S):
    for t in range(1, S.shape[0], 2):
        S[t, 1025:] = S[t - 1, 1025:]
    return S


@pytest.mark.parametrize("fault", [_nyquist_from_2047, _odd_from_even_above_1024], ids=["nyquist_from_2047", "odd_from_even_above_1024"])
def test_stft_faults_exceed_the_bound(fault):
    c = P.stft_case()
    seen = 0
    for s, (want, twin) in enumerate(zip(c.want, c.twin)):
        bad = fault(want.copy())
        if np.array_equal(bad, want):
            continue                                                                       # one frame: no odd frame to replace
        tol = P.bound(P.pair_errors(twin, want).max())
        err = P.pair_errors(bad, want).max()
        assert err > MARGIN * tol, (s, err, tol)
        seen += 1
    assert seen >= 7
    old = _old_measure(fault)
    print(f"{fault.__name__}: per-pair measure on noise {err:.2e} (bound {tol:.2e}); whole-tensor measure on probe_signal {old:.2e}")
    assert old < 0.1 * err                                                                 # the sentence that justifies the file


def test_vocoder_tail_fault_exceeds_the_bound():
    c = P.voc_case()
    seen = 0
    for want, twin in zip(c.want, c.twin):
        nout = want.shape[0]
        if nout % P.PV_U == 0 or nout < P.PV_U:
            continue
        bad = want.copy()
        bad[nout - nout % P.PV_U:] = want[nout - nout % P.PV_U - 1]
        tol, err = P.bound(P.bin_errors(twin, want).max()), P.bin_errors(bad, want).max()
        assert err > MARGIN * tol, (nout, err, tol)
        seen += 1
    assert seen >= 2


def test_istft_faults_exceed_the_bound():
    k = P.istft_case()
    rng = np.random.default_rng(7)
    for s in range(k.t.n):
        v = k.vocs[s].astype(np.complex128)
        nout, slen = v.shape[0], len(k.want[s])
        tol = P.bound(P.signal_error(k.twin[s], k.want[s]))
        bad = P.overlap_add(P.synthesis_frames(v), slen, t_lo_shift=1)                     # t_lo one too large
        assert P.signal_error(bad, k.want[s]) > MARGIN * tol, ("t_lo", s)
        if nout >= 2:                                                                      # DC / Nyquist imaginary parts not cleared
            w = v.copy()
            w[:, 0] += 1j * rng.standard_normal(nout) * np.abs(v).max()
            w[:, -1] += 1j * rng.standard_normal(nout) * np.abs(v).max()
            assert np.array_equal(R.istft(w, slen), k.want[s])                             # the semantics ignore them
            bad = P.overlap_add(P.synthesis_frames(w, dc_leak=True), slen)
            assert P.signal_error(bad, k.want[s]) > MARGIN * tol, ("dc", s)


def test_resampler_left_edge_fault_exceeds_the_bound():
    r = P.rs_case()
    seen = 0
    for s, (ys, rate, ln, nres) in enumerate(zip(r.ys, r.t.rates, P.col(r.t, "LEN"), P.col(r.t, "NRES"))):
        k = min(ln, nres)
        if k == 0:
            continue
        bad = P.resample_left(ys, rate, k, P.noise(80, 900 + s))
        tol = P.bound(P.signal_error(r.twin[s], r.want[s]))
        assert P.signal_error(bad, r.want[s][:k]) > MARGIN * tol, s
        seen += 1
    assert seen == 47


def test_peak_over_the_first_trip_only_changes_the_bits():
    nb = P.peak_blocks(max(P.PEAK_LENGTHS))
    for variant in (4, 5):                                                                 # the spike at nb * 256 and at the last sample
        x = P.peak_batch(variant)[-1]
        bad = x / np.max(np.abs(x[:nb * 256]))
        assert not np.array_equal(bad, P.peak_want(x)) and np.abs(P.peak_want(x)).max() == 1.0
    with np.errstate(all="ignore"):
        z = P.peak_want(np.zeros(5, np.float32))
    assert np.isnan(z).all()                                                               # numpy's 0 / 0: what the all-zero signal is pinned to
