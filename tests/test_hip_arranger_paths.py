"""The six original kernels of csrc/arranger.hip through the C ABI, on every path their launchers take: ds_pv_stft, ds_pv_vocode, ds_pv_istft
(frames and overlap-add), ds_resample_sinc, ds_peak_normalize and ds_mix_notes.  tests/test_hip_arranger.py drives them at the workload's
lengths on tables arranger._Plan builds; here are the smallest shapes, a caller's tables, rows that do not fit, and the refusals.  Cases,
table builder, geometry and error measures: tests/arranger_paths_ref.py; tests/test_arranger_paths_cpu.py shows without a GPU that the cases
reach every path named below and that each measure fails on a deliberate fault.

Every device buffer is a support_ref.slab (inputs, tables) or nan_slab (outputs, workspace); check_guards runs on all of them after every
launch.  The signals lie in the flat sample buffer with a gap of 64 NaN words behind every signal but the last, which ends at the slab's NaN
guard: a read past a signal's end that is not zeroed (ld_zero: the range check of a raw buffer load) shows as NaN in the spectrum.

Which case reaches which path:
  ds_pv_stft         lengths 1 .. 5121: nf 1 .. 6 (both parities: the `two == false` half of the two-frame transform), blocks of short signals
                     that exit; per frame pair against float64; imag == 0 at DC and Nyquist; no NaN; alone == in the batch
  ds_pv_vocode       nout % PV_U = 0, 1, 2, 3; zero bins; per bin against float64; spectra x 2^+-100 give the result x 2^+-100 bit for bit
                     (unit_mag's prescale); a caller's step_idx of -1, -2, nf - 1, nf, nf + 5 (the okl / okr guards)
  ds_pv_istft        nout 1 .. 8; per signal against float64; the imaginary parts of DC and Nyquist (finite, NaN) change no bit; a stretched
                     length 300 past what the frames cover (t_lo > t_hi: exact zeros); the gaps of y keep their NaN; the workspace size
  ds_resample_sinc   len 1 .. 2049 x rates 0.5 .. 2 (K 35 .. 69, a stretched length of 0); nres = len - 7 and nres = 0; rate 0, < 0, NaN
  ds_peak_normalize  len 1 .. 64 x 4096 + 4096 + 1 (the clamped partial count), the peak at each place of the strided loop; x 2^40; 0 / 0
  ds_mix_notes       track_len 1 .. 2053 on the test's own lists; ids and blk_ptr entries outside their ranges; n_blk_ev = 0
  rows that do not fit, host-side refusals: the last two tests.

Tolerance: the rule of tests/test_hip_arranger.py — 8 x the float32 twin's figure against float64 in the same measure, never below 2e-6, never
above 1e-3 — applied per signal in the finer measures of tests/arranger_paths_ref.py.  Everything else is bit for bit.  Every check prints
device, twin and bound, and appends them to $DS_ARRANGER_PARITY_LOG when that is set (profiles/arranger_paths_parity.txt keeps one green run's)."""
import os
import types

import numpy as np
import pytest
import torch

import arranger_paths_ref as P
import arranger_ref as R
import support_ref as S
from diffusynth_amd import _lib as L
from diffusynth_amd import arranger as A

pytestmark = pytest.mark.gpu
NB, W = P.NB, 2 * P.NB                           # bins, floats per frame of a spectrum


def note(line):
    print(line)
    path = os.environ.get("DS_ARRANGER_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def rule(what, dev, twin):
    tol = P.bound(twin)
    note(f"{what}: device {dev:.2e}, twin {twin:.2e}, bound {tol:.2e}")
    assert dev < tol, (what, dev, twin, tol)


def up(a):
    """A host array as a slab: float32 and int32 as they are, float64 as pairs of int32 words (8-byte aligned: the view starts 64 words in)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        a = a.view(np.int32)
    assert a.dtype in (np.float32, np.int32) and a.size > 0
    v = S.slab(torch.from_numpy(a.copy()))
    v.host_bits = a.view(np.uint32).copy()
    return v


def host(v):
    torch.cuda.synchronize()
    return v.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def settle(*views):
    """After a launch: the guards of every slab are intact, every input still holds its bits."""
    torch.cuda.synchronize()
    S.check_guards(*views)
    for v in views:
        if hasattr(v, "host_bits"):
            assert np.array_equal(v.cpu().numpy().view(np.uint32).reshape(-1), v.host_bits.reshape(-1)), "an input was written"


def tables(t):
    return types.SimpleNamespace(tab=up(t.tab.reshape(-1)), rates=up(t.rates), idx=up(t.idx), alpha=up(t.alpha))


def variant(t, **kw):
    return types.SimpleNamespace(**{**vars(t), **kw})


def rows_of(t, keep):
    """The launch of some rows of t on t's buffers: the same offsets and totals."""
    keep = list(keep)
    return variant(t, n=len(keep), tab=t.tab[keep].copy(), rates=t.rates[keep].copy())


# ------------------------------------------------------------------------------------------------- launches
def run_stft(t, x_flat):
    d, x, spec = tables(t), up(x_flat), S.nan_slab((t.total_frames * W,))
    L.call("ds_pv_stft", x.data_ptr(), d.tab.data_ptr(), t.n, t.max_frames, t.total_samples, t.total_frames, spec.data_ptr(), L.current_stream())
    settle(x, spec, d.tab)
    return host(spec)


def run_vocode(t, spec_flat):
    d, spec, voc = tables(t), up(spec_flat), S.nan_slab((t.total_out * W,))
    L.call("ds_pv_vocode", spec.data_ptr(), d.tab.data_ptr(), d.idx.data_ptr(), d.alpha.data_ptr(), t.n, t.total_frames, t.total_out, voc.data_ptr(),
           L.current_stream())
    settle(spec, voc, d.tab, d.idx, d.alpha)
    return host(voc)


def run_istft(t, voc_flat):
    d, voc = tables(t), up(voc_flat)
    nws = L.load().ds_pv_istft_ws_bytes(t.total_out)
    assert nws == t.total_out * 4096 * 4
    ws, y = S.nan_slab((nws // 4,)), S.nan_slab((t.total_stretched,))
    L.call("ds_pv_istft", voc.data_ptr(), d.tab.data_ptr(), t.n, t.max_out, t.max_stretched, t.total_out, t.total_stretched, ws.data_ptr(), y.data_ptr(),
           L.current_stream())
    settle(voc, ws, y, d.tab)
    return host(y)


def run_resample(t, ys_flat):
    d, ys, out = tables(t), up(ys_flat), S.nan_slab((t.total_samples,))
    L.call("ds_resample_sinc", ys.data_ptr(), d.tab.data_ptr(), d.rates.data_ptr(), t.n, t.max_len, t.total_stretched, t.total_samples, out.data_ptr(),
           L.current_stream())
    settle(ys, out, d.tab, d.rates)
    return host(out)


def run_peak(x_flat, tab, n, max_len, total):
    lib = L.load()
    nws = lib.ds_peak_normalize_ws_bytes(n, max_len)
    assert nws == n * P.peak_blocks(max_len) * 4
    x, dtab, ws, out = up(x_flat), up(np.asarray(tab, np.int32).reshape(-1)), S.nan_slab((nws // 4,)), S.nan_slab((total,))
    L.call("ds_peak_normalize", x.data_ptr(), dtab.data_ptr(), n, max_len, total, ws.data_ptr(), out.data_ptr(), L.current_stream())
    settle(x, dtab, ws, out)
    return host(out)


def peak_of(xs):
    lens = [len(x) for x in xs]
    tab = A._flat_table(lens)
    flat = run_peak(np.concatenate(xs), tab, len(xs), max(lens), sum(lens))
    return [flat[o:o + n] for o, n in zip(tab[:, P.COL["XOFF"]].tolist(), lens)]


def run_mix(flat, ev, ptr, lst, n_blk_ev, track_len):
    notes, dev, dptr = up(flat), up(ev.reshape(-1)), up(ptr)
    dlst = up(lst if len(lst) else np.zeros(1, np.int32))
    track = S.nan_slab((track_len,))
    L.call("ds_mix_notes", notes.data_ptr(), len(flat), dev.data_ptr(), len(ev), dptr.data_ptr(), dlst.data_ptr(), n_blk_ev, track.data_ptr(), track_len,
           L.current_stream())
    settle(notes, dev, dptr, dlst, track)
    return host(track)


def spectra(t, flat, off, cnt):
    return [P.cplx(g.reshape(-1, NB, 2)) for g in P.split(t, flat, off, cnt, W)]


def gaps_are_nan(t, flat, off, cnt):
    o, n = P.col(t, off), P.col(t, cnt)
    return all(np.isnan(flat[o[s] + n[s]:o[s + 1]]).all() and o[s + 1] - o[s] - n[s] == P.GAP for s in range(t.n - 1))


# ------------------------------------------------------------------------------------------------- ds_pv_stft
def test_stft_on_the_smallest_shapes():
    c = P.stft_case()
    t = c.t
    flat = run_stft(t, P.place(t, c.sigs))
    assert not np.isnan(flat).any(), "a read past a signal's end reached the spectrum"
    got = spectra(t, flat, "FOFF", "NF")
    for s, (g, want, twin) in enumerate(zip(got, c.want, c.twin)):
        assert g.shape == want.shape
        assert (g[:, 0].imag == 0).all() and (g[:, NB - 1].imag == 0).all(), s           # DC and Nyquist have no imaginary part
        rule(f"ds_pv_stft len {t.lengths[s]} (nf {want.shape[0]}), worst frame pair", P.pair_errors(g, want).max(), P.pair_errors(twin, want).max())
    rows = P.split(t, flat, "FOFF", "NF", W)
    for s, x in enumerate(c.sigs):                                                       # alone == in the batch, bit for bit
        assert same_bits(run_stft(P.build([len(x)], [t.steps[s]], gap=0), x), rows[s]), s


# ------------------------------------------------------------------------------------------------- ds_pv_vocode
def _spec_flat(t, specs):
    return P.place(t, [P.pairs(s) for s in specs], off="FOFF", total=t.total_frames, width=W)


def test_vocode_on_the_smallest_shapes_and_at_both_ends_of_the_exponent_range():
    c = P.voc_case()
    t = c.t
    base = _spec_flat(t, c.specs)
    flat = run_vocode(t, base)
    assert np.isfinite(flat).all()
    for s, (g, want, twin) in enumerate(zip(spectra(t, flat, "TOFF", "NOUT"), c.want, c.twin)):
        assert g.shape == want.shape and P.zeros_match(g, want), s                        # zero bins give exact zeros
        rule(f"ds_pv_vocode len {t.lengths[s]} n_steps {t.steps[s]} (nout {want.shape[0]}), worst bin", P.bin_errors(g, want).max(),
             P.bin_errors(twin, want).max())
    tiny = np.float32(P.TINY32)
    for e in (100, -100):                                                                # unit_mag: the squares neither overflow nor underflow
        scaled = np.ldexp(base, e).astype(np.float32)
        assert np.isfinite(scaled).all() and ((np.abs(scaled) >= tiny) | (scaled == 0)).all(), "a scaled input left the normal range"
        assert np.array_equal(np.ldexp(scaled.astype(np.float64), -e), base.astype(np.float64))
        with np.errstate(over="ignore", under="ignore"):
            sq = scaled * scaled                                                         # what |v|^2 without the prescale would be
        assert np.isinf(sq).any() if e > 0 else ((sq == 0) & (scaled != 0)).any()
        # the expected words: the first result times 2^e, exact wherever that is zero or normal.  A component that is tiny beside its
        # partner (a phase of almost 0: the accumulator behind a zero frame is u conj(u)) falls below the normal range at 2^-100: there
        # the scaled result is whatever rounding or flushing leaves, at most the smallest normal number
        exact = np.ldexp(flat.astype(np.float64), e)
        normal = (np.abs(exact) >= P.TINY32) | (exact == 0)
        assert np.abs(exact).max() < 2.0 ** 127 and normal.mean() > 0.98 and (e < 0 or normal.all())
        got = run_vocode(t, scaled)
        assert same_bits(got[normal], exact.astype(np.float32)[normal]), e
        assert (np.abs(got[~normal]) <= tiny).all(), e
        note(f"ds_pv_vocode: spectra x 2^{e} give the result x 2^{e} bit for bit ({(~normal).sum()} of {normal.size} words below the normal range)")


def test_vocode_with_a_callers_step_indices():
    n, st = 5121, 4
    t = P.build([n], [st], gap=0)
    nf, nout = t.max_frames, t.max_out
    spec = R.stft(P.noise(n, 210)).astype(np.complex64)
    t.idx = P.caller_steps(nf, nout)
    flat = run_vocode(t, _spec_flat(t, [spec]))
    assert np.isfinite(flat).all()
    g = spectra(t, flat, "TOFF", "NOUT")[0]
    want, twin = P.vocode(spec, t.idx, t.alpha), P.vocode(spec, t.idx, t.alpha, np.float32)
    assert P.zeros_match(g, want) and (want[[2, 4, 5]] == 0).all() and (want[[1, 3]] != 0).all()        # -2, nf, nf + 5 read nothing; -1 and nf - 1 one frame
    rule("ds_pv_vocode step_idx -1, -2, nf - 1, nf, nf + 5, worst bin", P.bin_errors(g, want).max(), P.bin_errors(twin, want).max())


# ------------------------------------------------------------------------------------------------- ds_pv_istft
def _voc_flat(t, vocs):
    return P.place(t, [P.pairs(v) for v in vocs], off="TOFF", total=t.total_out, width=W)


def test_istft_on_the_smallest_shapes():
    lib = L.load()
    assert lib.ds_pv_istft_ws_bytes(0) == 0 and lib.ds_pv_istft_ws_bytes(-3) == 0 and lib.ds_pv_istft_ws_bytes(7) == 7 * 4096 * 4
    c = P.istft_case()
    t = c.t
    base = _voc_flat(t, c.vocs)
    y = run_istft(t, base)
    assert gaps_are_nan(t, y, "SOFF", "SLEN")                                              # between one signal's slen and the next soff
    for s, (g, want, twin) in enumerate(zip(P.split(t, y, "SOFF", "SLEN"), c.want, c.twin)):
        assert g.shape == want.shape and np.isfinite(g).all()
        rule(f"ds_pv_istft len {t.lengths[s]} n_steps {t.steps[s]} (nout {c.vocs[s].shape[0]}) -> {len(want)}", P.signal_error(g, want),
             P.signal_error(twin, want))
    # the imaginary parts of DC and Nyquist do not exist for a real signal: whatever stands there changes no bit
    rng = np.random.default_rng(11)
    other = base.reshape(-1, NB, 2).copy()
    other[:, 0, 1] = 50.0 * rng.standard_normal(len(other))
    other[:, NB - 1, 1] = 50.0 * rng.standard_normal(len(other))
    other[::3, 0, 1] = np.nan
    other[1::3, NB - 1, 1] = np.nan
    assert same_bits(run_istft(t, other.reshape(-1)), y)
    # a caller's stretched length 300 samples past what the synthesis frames cover: t_lo > t_hi, exact zeros
    long = {2: P.coverage_end(3) + 300, 7: P.coverage_end(8) + 300}

    def fix(s, row):
        row["SLEN"] = long.get(s, row["SLEN"])
    u = P.build(t.lengths, t.steps, fix=fix)
    assert u.total_out == t.total_out and P.col(u, "TOFF") == P.col(t, "TOFF")
    yl = run_istft(u, base)
    assert gaps_are_nan(u, yl, "SOFF", "SLEN")
    for s, (g, ref) in enumerate(zip(P.split(u, yl, "SOFF", "SLEN"), P.split(t, y, "SOFF", "SLEN"))):
        assert same_bits(g[:len(ref)], ref) and np.isfinite(g).all(), s
        if s in long:
            counts = P.ola_counts(c.vocs[s].shape[0], long[s])[0]
            assert (counts[-300:] == 0).all() and (counts[:-300] > 0).all() and same_bits(g[-300:], np.zeros(300, np.float32)), s
    note("ds_pv_istft: DC / Nyquist imaginary parts (finite, NaN) change no bit; 300 samples no frame covers are +0")


# ------------------------------------------------------------------------------------------------- ds_resample_sinc
def test_resample_on_the_smallest_shapes():
    c = P.rs_case()
    t = c.t
    ys = P.place(t, c.ys, off="SOFF", total=t.total_stretched)
    out = run_resample(t, ys)
    assert gaps_are_nan(t, out, "XOFF", "LEN")
    got = P.split(t, out, "XOFF", "LEN")
    for s, (g, want, twin) in enumerate(zip(got, c.want, c.twin)):
        nres = P.col(t, "NRES")[s]
        assert g.shape == want.shape and np.isfinite(g).all() and not g[max(nres, 0):].any()
        rule(f"ds_resample_sinc len {t.lengths[s]} n_steps {t.steps[s]} (slen {P.col(t, 'SLEN')[s]})", P.signal_error(g, want), P.signal_error(twin, want))
    for what in ("len - 7", "0"):                                                        # a caller's nres: exact zeros from nres on
        u = variant(t, tab=t.tab.copy())
        u.tab[:, P.COL["NRES"]] = [n - 7 if what == "len - 7" else 0 for n in t.lengths]
        cut = P.split(u, run_resample(u, ys), "XOFF", "LEN")
        for s, (g, ref) in enumerate(zip(cut, got)):
            k = max(0, min(P.col(u, "NRES")[s], P.col(t, "NRES")[s]))
            assert same_bits(g[:k], ref[:k]) and same_bits(g[k:], np.zeros(len(g) - k, np.float32)), (what, s)
    note("ds_resample_sinc: nres = len - 7 and nres = 0 give +0 from nres on, the bits of the full row before it")


def test_resample_rows_without_a_positive_rate_write_nothing():
    t = P.build([257] * 4, [4, 1, -3, 0])
    ys = P.place(t, [P.noise(n, 450 + s) for s, n in enumerate(P.col(t, "SLEN"))], off="SOFF", total=t.total_stretched)
    good = P.split(t, run_resample(t, ys), "XOFF", "LEN")
    u = variant(t, rates=t.rates.copy())
    u.rates[1:] = (0.0, -1.0, np.nan)
    got = P.split(u, run_resample(u, ys), "XOFF", "LEN")
    assert same_bits(got[0], good[0]) and np.isfinite(good[0]).all()
    assert all(np.isnan(g).all() for g in got[1:])


# ------------------------------------------------------------------------------------------------- ds_peak_normalize
def test_peak_normalize_is_numpys_quotient_wherever_the_peak_lies():
    nb = P.peak_blocks(max(P.PEAK_LENGTHS))
    assert nb == P.PN_NB_MAX and L.load().ds_peak_normalize_ws_bytes(len(P.PEAK_LENGTHS), max(P.PEAK_LENGTHS)) == len(P.PEAK_LENGTHS) * 64 * 4
    assert L.load().ds_peak_normalize_ws_bytes(0, 5) == 0 and L.load().ds_peak_normalize_ws_bytes(3, 0) == 0
    last = None
    for v in range(6):
        xs = P.peak_batch(v)
        got = peak_of(xs)
        for s, (g, x) in enumerate(zip(got, xs)):
            assert same_bits(g, P.peak_want(x)), (v, s)
        last = (xs, got)
    note(f"ds_peak_normalize: lengths {P.PEAK_LENGTHS}, nb {nb}, the peak at 0, 255, 256, nb * 256 - 1, nb * 256, len - 1: numpy's fp32 quotient bit for bit")
    xs, got = last
    for s, g in enumerate(peak_of(P.peak_batch(5, scale=40))):                            # a power of two changes no bit of the quotient
        assert same_bits(g, got[s]), s
    for s, x in enumerate(xs):                                                           # alone (its own partial count) == in the batch
        assert same_bits(peak_of([x])[0], got[s]), s


def test_peak_normalize_of_silence_is_numpys_nan_and_leaves_the_neighbour_alone():
    x = P.peak_signal(257, 77, 100)
    got = peak_of([np.zeros(300, np.float32), x])
    assert np.isnan(got[0]).all() and np.array_equal(got[0], P.peak_want(np.zeros(300, np.float32)), equal_nan=True)      # 0 / 0
    assert same_bits(got[1], P.peak_want(x)) and same_bits(got[1], peak_of([x])[0])


# ------------------------------------------------------------------------------------------------- ds_mix_notes
@pytest.mark.parametrize("track_len", P.MIX_TRACKS)
def test_mix_notes_on_the_tests_own_lists(track_len):
    notes, events = P.mix_case(track_len)
    flat, ev, ptr, lst = P.mix_tables(notes, events, track_len)
    want = P.mix_numpy(notes, events, track_len)
    got = run_mix(flat, ev, ptr, lst, len(lst), track_len)
    assert same_bits(got, want)                                                          # numpy's float32 += float64 in event order
    # entries only a caller can build: an id of -1, an id of n_ev, an event whose (offset, length) leaves `notes`, blk_ptr entries -3 and
    # above n_blk_ev
    ev2 = np.concatenate([ev, np.array([[0, len(flat), 1]], np.int32)])
    head = np.array([-1, len(ev2), len(ev2) - 1], np.int32)
    lst2 = np.concatenate([head, lst])
    ptr2 = ptr.copy()
    ptr2[1:] += len(head)
    ptr2[0], ptr2[-1] = -3, len(lst2) + 7
    walk, touched = P.mix_walk(flat, ev2, ptr2, lst2, len(lst2), track_len)
    got2 = run_mix(flat, ev2, ptr2, lst2, len(lst2), track_len)
    assert not np.isnan(got2).any() and touched == {0, len(ptr) - 2}
    assert same_bits(got2, walk) and same_bits(got2, want)                                # left out: the touched blocks too keep their bits
    zeros = run_mix(flat, ev, ptr, lst, 0, track_len)                                    # n_blk_ev = 0 with events present
    assert same_bits(zeros, np.zeros(track_len, np.float32))


# ------------------------------------------------------------------------------------------------- rows that do not fit
def _misfits(t, fields):
    """For each (field, value): the three-row launch with the middle row's field set to it."""
    for f, v in fields:
        u = variant(t, tab=t.tab.copy())
        u.tab[1, P.COL[f]] = v
        yield f"{f} = {v}", u


def test_a_row_that_does_not_fit_reads_and_writes_nothing():
    """Three rows, the middle one with one field that leaves the totals the caller states, a negative offset or a negative count: the whole
    output equals, bit for bit, that of the launch of the two outer rows on the same buffers — the middle row's words keep their NaN."""
    lengths, steps = (1025, 2048, 300), (4, -3, 1)
    t = P.build(lengths, steps)
    r = {f: P.col(t, f)[1] for f in P.FIELDS}
    sigs = [P.noise(n, 600 + s) for s, n in enumerate(lengths)]
    specs = [R.stft(x).astype(np.complex64) for x in sigs]
    vocs = [R.phase_vocoder(sp, rate).astype(np.complex64) for sp, rate in zip(specs, t.rates)]
    ys = [P.noise(n, 610 + s) for s, n in enumerate(P.col(t, "SLEN"))]
    x_flat, spec_flat, voc_flat = P.place(t, sigs), _spec_flat(t, specs), _voc_flat(t, vocs)
    ys_flat = P.place(t, ys, off="SOFF", total=t.total_stretched)
    outer = rows_of(t, (0, 2))
    plans = (
        ("ds_pv_stft", lambda u: run_stft(u, x_flat), ("FOFF", "NF", W),
         [("XOFF", t.total_samples - r["LEN"] + 1), ("LEN", t.total_samples - r["XOFF"] + 1), ("FOFF", t.total_frames - r["NF"] + 1), ("XOFF", -1), ("FOFF", -1),
          ("LEN", -5)]),
        ("ds_pv_vocode", lambda u: run_vocode(u, spec_flat), ("TOFF", "NOUT", W),
         [("FOFF", t.total_frames - r["NF"] + 1), ("TOFF", t.total_out - r["NOUT"] + 1), ("NOUT", t.total_out - r["TOFF"] + 1), ("FOFF", -1), ("TOFF", -1),
          ("NOUT", -2), ("NF", -1)]),
        ("ds_pv_istft", lambda u: run_istft(u, voc_flat), ("SOFF", "SLEN", 1),
         [("TOFF", t.total_out - r["NOUT"] + 1), ("SOFF", t.total_stretched - r["SLEN"] + 1), ("SLEN", t.total_stretched - r["SOFF"] + 1), ("TOFF", -1),
          ("SOFF", -1), ("NOUT", -2), ("SLEN", -4)]),
        ("ds_resample_sinc", lambda u: run_resample(u, ys_flat), ("XOFF", "LEN", 1),
         [("XOFF", t.total_samples - r["LEN"] + 1), ("SOFF", t.total_stretched - r["SLEN"] + 1), ("SLEN", t.total_stretched - r["SOFF"] + 1), ("XOFF", -1),
          ("SOFF", -1), ("SLEN", -4), ("LEN", -5)]),
        ("ds_peak_normalize", lambda u: run_peak(x_flat, u.tab, u.n, u.max_len, u.total_samples), ("XOFF", "LEN", 1),
         [("XOFF", t.total_samples - r["LEN"] + 1), ("LEN", t.total_samples - r["XOFF"] + 1), ("XOFF", -1), ("LEN", -5)]),
    )
    for name, run, (off, cnt, width), fields in plans:
        want = run(outer)
        o, n = P.col(t, off)[1] * width, P.col(t, cnt)[1] * width
        full = run(t)
        assert np.isnan(want[o:o + n]).all() and n > 0 and np.isfinite(full[o:o + n]).all(), name        # the middle row has words of its own
        keep = np.ones(len(want), bool)
        keep[o:o + n] = False
        assert same_bits(full[keep], want[keep]), name                                   # the outer rows: the same bits beside any neighbour
        for what, u in _misfits(t, fields):
            assert same_bits(run(u), want), (name, what)
        note(f"{name}: a middle row with {', '.join(f + ' = ' + str(v) for f, v in fields)} writes nothing; the outer rows keep their bits")


# ------------------------------------------------------------------------------------------------- host-side refusals
def test_host_side_refusals():
    """Each call returns the library's error before anything is launched: the NaN-filled outputs stay untouched.  No buffer of the refused
    sizes exists."""
    lib, st = L.load(), L.current_stream()
    t = P.build([1024], [4], gap=0)
    d = tables(t)
    x, spec, voc = up(P.noise(1024, 1)), S.nan_slab((t.total_frames * W,)), S.nan_slab((t.total_out * W,))
    ws, y, out = S.nan_slab((t.total_out * 4096,)), S.nan_slab((t.total_stretched,)), S.nan_slab((1024,))
    pws, track = S.nan_slab((4,)), S.nan_slab((1024,))
    ev, ptr, lst = up(np.array([0, 0, 1024], np.int32)), up(np.array([0, 1], np.int32)), up(np.zeros(1, np.int32))
    p = lambda v: v.data_ptr()                                                            # noqa: E731
    BIG = 2 ** 31                                                                        # one more than an int32 offset reaches
    null, bad, most, align = "bad args", "bad args", "at most", "aligned"
    calls = {
        "ds_pv_stft": ([p(x), p(d.tab), 1, t.max_frames, 1024, t.total_frames, p(spec), st],
                       [(0, None, null), (1, None, null), (6, None, null), (2, 0, bad), (2, 65536, most), (3, 0, bad), (4, 0, bad), (5, 0, bad), (4, BIG, most),
                        (5, (BIG - 1) // NB + 1, most), (4, 2 ** 30, r"2\^30"), (4, 2 ** 30 - 2047, r"2\^30"), (6, p(spec) + 4, align), (0, p(x) + 2, align),
                        (1, p(d.tab) + 2, align)]),
        "ds_pv_vocode": ([p(spec), p(d.tab), p(d.idx), p(d.alpha), 1, t.total_frames, t.total_out, p(voc), st],
                         [(0, None, null), (1, None, null), (2, None, null), (3, None, null), (7, None, null), (4, 0, bad), (4, 65536, most), (5, 0, bad), (6, 0, bad),
                          (5, (BIG - 1) // NB + 1, most), (6, (BIG - 1) // NB + 1, most), (0, p(spec) + 4, align), (7, p(voc) + 4, align), (2, p(d.idx) + 2, align)]),
        "ds_pv_istft": ([p(voc), p(d.tab), 1, t.max_out, t.max_stretched, t.total_out, t.total_stretched, p(ws), p(y), st],
                        [(0, None, null), (1, None, null), (7, None, null), (8, None, null), (2, 0, bad), (2, 65536, most), (3, 0, bad), (4, 0, bad), (5, 0, bad),
                         (6, 0, bad), (5, BIG // 4096, most), (6, BIG, most), (0, p(voc) + 4, align), (8, p(y) + 2, align), (7, p(ws) + 2, align)]),
        "ds_resample_sinc": ([p(y), p(d.tab), p(d.rates), 1, 1024, t.total_stretched, 1024, p(out), st],
                             [(0, None, null), (1, None, null), (2, None, null), (7, None, null), (3, 0, bad), (3, 65536, most), (4, 0, bad), (5, 0, bad), (6, 0, bad),
                              (5, BIG, most), (6, BIG, most), (2, p(d.rates) + 4, align), (7, p(out) + 2, align), (0, p(y) + 2, align)]),
        "ds_peak_normalize": ([p(x), p(d.tab), 1, 1024, 1024, p(pws), p(out), st],
                              [(0, None, null), (1, None, null), (5, None, null), (6, None, null), (2, 0, bad), (2, 65536, most), (3, 0, bad), (4, 0, bad),
                               (4, BIG, most), (0, p(x) + 2, align), (6, p(out) + 2, align)]),
        "ds_mix_notes": ([p(x), 1024, p(ev), 1, p(ptr), p(lst), 1, p(track), 1024, st],
                         [(0, None, null), (2, None, null), (4, None, null), (5, None, null), (7, None, null), (1, 0, bad), (3, 0, bad), (6, -1, bad), (8, 0, bad),
                          (1, BIG, most), (0, p(x) + 2, align), (7, p(track) + 2, align)]),
    }
    n = 0
    for name, (good, refused) in calls.items():
        for pos, val, word in refused:
            args = list(good)
            args[pos] = val
            assert getattr(lib, name)(*args) != 0, (name, pos, val)
            with pytest.raises(L.DsError, match=word):
                L.call(name, *args)
            n += 1
    torch.cuda.synchronize()
    for v in (spec, voc, ws, y, out, pws, track):
        assert bool(torch.isnan(v).all())
    S.check_guards(x, spec, voc, ws, y, out, pws, track, ev, ptr, lst, d.tab, d.rates, d.idx, d.alpha)
    note(f"host-side refusals: {n} calls of the six entry points refused before any launch")
