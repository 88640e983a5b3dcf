"""Plain CPU helpers of tests/test_hip_arranger_paths.py and tests/test_arranger_paths_cpu.py: the six original kernels of csrc/arranger.hip
(ds_pv_stft, ds_pv_vocode, ds_pv_istft, ds_resample_sinc, ds_peak_normalize, ds_mix_notes) on every path their launchers take.

Four kinds of thing live here:
  cases          the smallest lengths at which each path exists, white noise throughout (every bin and every sample at one scale);
  table builder  arranger._Plan's arithmetic RESTATED (tests/test_arranger_paths_cpu.py asserts the equality), with a gap of GAP NaN words
                 behind every signal but the last in the sample buffers, and single fields open to the caller;
  geometry       host arithmetic that says which path a block, a frame or a sample takes in each kernel: the CPU test asserts that the
                 case list reaches every path, so a shortened list says which path went dark;
  restatements   the float64 semantics are tests/arranger_ref.py's; here are the forms that take a CALLER's tables (step indices outside
                 the spectrum, stretched lengths no frame covers), the mixer's list walk, and the error measures.

Error measures: finer than the whole-tensor norms of tests/test_hip_arranger.py.  STFT: per frame PAIR (2t, 2t + 1) as the kernel transforms
them, max |got - want| over the pair's largest |want| (the two-for-one separation couples a frame's error to its partner's scale: the measure
says so).  Vocoder: per bin, |got - want| / |want|.  iSTFT, resampler: per signal, max-norm over the signal's largest |want|.  The rule
is that of tests/test_hip_arranger.py: 8 x the float32 twin's figure in the same measure, inside [2e-6, 1e-3]."""
import functools
import math
import types

import numpy as np

import arranger_ref as R
from diffusynth_amd import _lib as L

N_FFT, HOP, NB = R.N_FFT, R.HOP, R.N_FFT // 2 + 1
PV_U = 4                    # synthesis frames per trip of pv_vocode_kernel
SPB = 1024                  # samples per block: resampler, normaliser's divide, mixer
PN_CHUNK, PN_NB_MAX = 4096, 64
GAP = 64                    # NaN words behind every signal but the last
PV = L.PV
NI = PV["DS_PV_NI"]
FIELDS = ("XOFF", "LEN", "FOFF", "NF", "TOFF", "NOUT", "SOFF", "SLEN", "NRES")
COL = {f: PV["DS_PV_" + f] for f in FIELDS}
TINY32 = R.TINY32

# ------------------------------------------------------------------------------------------------- cases
STFT_LENGTHS = (1, 1023, 1024, 1025, 2047, 2048, 3072, 4097, 5121)            # nf 1, 1, 2, 2, 2, 3, 4, 5, 6
VOC_STEPS = (-3, 0.5, 1, -3, 4, 4, 0.5, 4, 4)                                 # nout 1, 2, 3, 2, 3, 4, 5, 7, 8
ISTFT_CASES = ((1, -3), (1023, 4), (1024, 0.5), (2048, 4), (3072, 1), (3072, 4), (4097, 4), (5121, 4))      # nout 1 .. 8
RS_LENGTHS = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
RS_STEPS = (4, 1, -3, -12, 0, 12)             # rates 0.79, 0.94, 1.19, 2, 1 and 1 / 2: K = ceil(32 / (0.95 min(1, rate))) + 1 = 44, 37, 35, 35, 35, 69
RS_CASES = tuple((n, st) for n in RS_LENGTHS for st in RS_STEPS)
PEAK_LENGTHS = (1, 255, 256, 257, 4096, 4097, PN_NB_MAX * PN_CHUNK + PN_CHUNK + 1)
PEAK_SPIKE = 3.5
MIX_TRACKS = (1, 1023, 1025, 2048 + 5)


def noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def cplx(a):
    """(..., 2) floats -> complex128."""
    a = np.asarray(a, np.float64)
    return a[..., 0] + 1j * a[..., 1]


def pairs(a):
    """complex -> (..., 2) float32, the device's layout."""
    a = np.asarray(a)
    return np.stack([a.real, a.imag], axis=-1).astype(np.float32)


# ------------------------------------------------------------------------------------------------- table builder
def build(lengths, steps, gap=GAP, fix=None):
    """The DS_PV_NI table, rates, step_idx and step_alpha of one batched pitch_shift as host arrays, as arranger._Plan forms them (gap = 0:
    the same numbers).  gap: that many words are skipped behind every signal but the last in the sample buffer (XOFF) and in the stretched
    buffer (SOFF); the totals count them.  fix(s, row): may change a row (a dict over FIELDS) before the offsets move on, e.g. a longer SLEN."""
    n = len(lengths)
    tab = np.zeros((n, NI), np.int32)
    rates = np.zeros(n, np.float64)
    idx, alpha = [], []
    xoff = foff = toff = soff = 0
    for s, (ln, st) in enumerate(zip(lengths, steps)):
        rate = 2.0 ** (-float(st) / 12.0)
        nf = 1 + ln // HOP
        ts = np.arange(0, nf, rate, dtype=np.float64)
        slen = int(round(ln / rate))
        row = dict(XOFF=xoff, LEN=ln, FOFF=foff, NF=nf, TOFF=toff, NOUT=len(ts), SOFF=soff, SLEN=slen, NRES=int(math.ceil(slen * rate)))
        if fix is not None:
            fix(s, row)
        for f in FIELDS:
            tab[s, COL[f]] = row[f]
        rates[s] = rate
        idx.append(np.floor(ts).astype(np.int32))
        alpha.append(np.mod(ts, 1.0).astype(np.float32))
        g = gap if s < n - 1 else 0
        xoff, foff, toff, soff = xoff + row["LEN"] + g, foff + nf, toff + len(ts), soff + row["SLEN"] + g
    return types.SimpleNamespace(n=n, tab=tab, rates=rates, idx=np.concatenate(idx), alpha=np.concatenate(alpha), lengths=list(lengths), steps=list(steps),
                                 total_samples=xoff, total_frames=foff, total_out=toff, total_stretched=soff,
                                 max_len=int(tab[:, COL["LEN"]].max()), max_frames=int(tab[:, COL["NF"]].max()),
                                 max_out=int(tab[:, COL["NOUT"]].max()), max_stretched=int(tab[:, COL["SLEN"]].max()))


def col(t, f):
    return t.tab[:, COL[f]].tolist()


def packed(t):
    """[rates | tab | step_idx | step_alpha] as arranger._Plan.host packs them."""
    return np.concatenate([t.rates.view(np.int32), t.tab.reshape(-1), t.idx, t.alpha.view(np.int32)])


def place(t, arrays, off="XOFF", total=None, dtype=np.float32, width=1):
    """The signals' arrays in one flat buffer at their offsets, NaN in the gaps."""
    flat = np.full((t.total_samples if total is None else total) * width, np.nan, dtype)
    for a, o in zip(arrays, col(t, off)):
        a = np.asarray(a, dtype).reshape(-1)
        flat[o * width:o * width + a.size] = a
    return flat


def split(t, flat, off, cnt, width=1):
    flat = np.asarray(flat)
    return [flat[o * width:(o + n) * width] for o, n in zip(col(t, off), col(t, cnt))]


def coverage_end(nout):
    """The first stretched sample no synthesis frame covers."""
    return N_FFT // 2 + HOP * (nout - 1)


# ------------------------------------------------------------------------------------------------- geometry
def fits(off, n, total):
    return off >= 0 and n >= 0 and off + n <= total


def _rows(t):
    for s in range(t.n):
        yield s, {f: int(t.tab[s, COL[f]]) for f in FIELDS}


def frame_blocks(t, kernel):
    """Blocks of the three two-frames-per-transform launches ("stft", "istft"): (signal, block, why it exits or None, two)."""
    out = []
    for s, r in _rows(t):
        cnt, grid = (r["NF"], t.max_frames) if kernel == "stft" else (r["NOUT"], t.max_out)
        for bx in range((grid + 1) // 2):
            t0 = 2 * bx
            if t0 >= cnt:
                why = "past the signal's frames"
            elif kernel == "stft" and not fits(r["XOFF"], r["LEN"], t.total_samples):
                why = "xoff + len"
            elif kernel == "stft" and not fits(r["FOFF"], r["NF"], t.total_frames):
                why = "foff + nf"
            elif kernel == "istft" and not fits(r["TOFF"], r["NOUT"], t.total_out):
                why = "toff + nout"
            else:
                why = None
            out.append((s, bx, why, None if why else t0 + 1 < cnt))
    return out


def vocode_rows(t):
    """(signal, why the row's threads exit or None, nout % PV_U)."""
    out = []
    for s, r in _rows(t):
        why = "nf <= 0" if r["NF"] <= 0 else "foff + nf" if not fits(r["FOFF"], r["NF"], t.total_frames) else \
            "toff + nout" if not fits(r["TOFF"], r["NOUT"], t.total_out) else None
        out.append((s, why, r["NOUT"] % PV_U if r["NOUT"] > 0 else None))
    return out


def ola_counts(nout, slen):
    """Per stretched sample the frames pv_ola_kernel sums: t_hi - t_lo + 1, 0 where t_lo > t_hi."""
    pos = np.arange(slen) + N_FFT // 2
    t_hi = np.minimum(pos // HOP, nout - 1)
    t_lo = np.where(pos < N_FFT, 0, (pos - N_FFT) // HOP + 1)
    return np.maximum(t_hi - t_lo + 1, 0), t_lo, t_hi


def ola_blocks(t):
    """(signal, block of 256, exits whole) of the overlap-add launch."""
    return [(s, bx, bx * 256 >= r["SLEN"]) for s, r in _rows(t) for bx in range((t.max_stretched + 255) // 256)]


def resample_blocks(t):
    """(signal, block of SPB, why it exits or None)."""
    out = []
    for s, r in _rows(t):
        for bx in range((t.max_len + SPB - 1) // SPB):
            why = "past the signal" if bx * SPB >= r["LEN"] else "xoff + len" if not fits(r["XOFF"], r["LEN"], t.total_samples) else \
                "soff + slen" if not fits(r["SOFF"], r["SLEN"], t.total_stretched) else "rate" if not t.rates[s] > 0.0 else None
            out.append((s, bx, why))
    return out


def resample_edges(ln, slen, nres, rate):
    """Per output sample: taps dropped on the left (n < 0), on the right (n >= slen), and m >= nres (the zero tail); and K."""
    fc = R.RS_FC * min(1.0, rate)
    half = R.RS_Z / fc
    K = int(math.ceil(half)) + 1
    p = np.arange(ln, dtype=np.float64) / rate
    base = np.floor(p).astype(np.int64)
    frac = p - base
    left = np.zeros(ln, bool)
    right = np.zeros(ln, bool)
    for j in range(-K, K + 1):
        live = np.abs(frac - j) <= half
        left |= live & (base + j < 0)
        right |= live & (base + j >= slen)
    tail = np.arange(ln) >= nres
    return left & ~tail, right & ~tail, tail, K


def peak_blocks(max_len):
    nb = (max_len + PN_CHUNK - 1) // PN_CHUNK
    return min(max(nb, 1), PN_NB_MAX)


# ------------------------------------------------------------------------------------------------- restatements on a caller's tables
def vocode(D, i0, alpha, dtype=np.float64):
    """arranger_ref.phase_vocoder (phasor form) on given step tables: frame i0 on the left and i0 + 1 on the right, a frame outside
    [0, n_frames) a zero frame (librosa's two appended zero frames are the ordinary case)."""
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    D = np.asarray(D).astype(ctype)
    nf, zero = D.shape[0], np.zeros(D.shape[1], ctype)
    fr = lambda i: D[i] if 0 <= i < nf else zero                                    # noqa: E731
    out = np.zeros((len(i0), D.shape[1]), ctype)
    _, acc = R._unit(D[0], dtype)
    acc = acc.astype(ctype)
    for t in range(len(i0)):
        ml, ul = R._unit(fr(int(i0[t])), dtype)
        mr, ur = R._unit(fr(int(i0[t]) + 1), dtype)
        a = dtype(alpha[t])
        out[t] = ((dtype(1.0) - a) * ml + a * mr) * acc
        acc = (acc * (ur * np.conj(ul)).astype(ctype)).astype(ctype)
        acc = (acc / np.abs(acc).astype(dtype)).astype(ctype)
    return out


def synthesis_frames(S, dtype=np.float64, dc_leak=False):
    """The windowed inverse transforms pv_istft_frames_kernel leaves in its workspace.  dc_leak: the fault of NOT clearing the imaginary
    parts of DC and Nyquist: with Z = A + i B, Im A[0] lands in frame t + 1 as a constant and Im B[0] in frame t (Nyquist: alternating)."""
    S = np.asarray(S)
    fr = np.fft.irfft(S, n=N_FFT, axis=1).astype(dtype)
    if dc_leak:
        alt = (-1.0) ** np.arange(N_FFT)
        for t in range(0, S.shape[0] - 1, 2):
            fr[t + 1] += (S[t, 0].imag + S[t, -1].imag * alt) / N_FFT
            fr[t] -= (S[t + 1, 0].imag + S[t + 1, -1].imag * alt) / N_FFT
    return fr * R.hann(dtype)[None, :]


def overlap_add(fr, slen, dtype=np.float64, t_lo_shift=0):
    """pv_ola_kernel's gather: sample s sums frames t_lo .. t_hi in frame order and divides by its window-sum-square where that exceeds
    tiny; a sample no frame covers is 0.  t_lo_shift = 1 is the fault "t_lo one too large"."""
    nout = fr.shape[0]
    _, t_lo, t_hi = ola_counts(nout, slen)
    t_lo = t_lo + t_lo_shift
    pos = np.arange(slen) + N_FFT // 2
    w2 = R.hann(dtype) ** 2
    v, wss = np.zeros(slen, dtype), np.zeros(slen, dtype)
    for t in range(nout):
        live = (t >= t_lo) & (t <= t_hi)
        n = np.clip(pos - t * HOP, 0, N_FFT - 1)
        v = v + np.where(live, fr[t][n], 0).astype(dtype)
        wss = wss + np.where(live, w2[n], 0).astype(dtype)
    nz = wss > TINY32
    v[nz] = v[nz] / wss[nz]
    return v


def resample_left(x, rate, n_out, left):
    """arranger_ref.resample in float64 with the taps at n < 0 NOT dropped: they read `left` (left[-1] is the word in front of x)."""
    x = np.asarray(x, np.float64)
    pad = len(left)
    fc = R.RS_FC * min(1.0, rate)
    half = R.RS_Z / fc
    pos = np.arange(n_out, dtype=np.float64) / rate
    base = np.floor(pos).astype(np.int64)
    frac = pos - base
    K = int(math.ceil(half)) + 1
    assert pad >= K
    xe = np.concatenate([np.asarray(left, np.float64), x])
    out = np.zeros(n_out)
    for j in range(-K, K + 1):
        n = base + j
        t = frac - j
        inside = (np.abs(t) <= half) & (n < len(x))
        h = fc * np.sinc(fc * t) * R.kaiser(t / half)
        out = out + np.where(inside, h * xe[np.clip(n + pad, 0, len(xe) - 1)], 0)
    return out


def resample_want(ys, rate, ln, nres, dtype=np.float64):
    """What ds_resample_sinc stores for one row: nres samples through the filter, zeros up to len (fix_length)."""
    out = np.zeros(ln, dtype)
    k = max(0, min(nres, ln))
    if k:
        out[:k] = R.resample(ys, rate, k, dtype)
    return out


# ------------------------------------------------------------------------------------------------- error measures, the rule
def pair_errors(got, want):
    """Per frame pair (2t, 2t + 1): max |got - want| over the pair / the pair's largest |want|."""
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    return np.array([np.abs(got[t:t + 2] - want[t:t + 2]).max() / np.abs(want[t:t + 2]).max() for t in range(0, want.shape[0], 2)])


def bin_errors(got, want):
    """|got - want| / |want| at every (t, k) with want != 0 (0 elsewhere: those must be equal to 0 exactly, zeros_match)."""
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    nz = want != 0
    e = np.zeros(want.shape)
    e[nz] = np.abs(got - want)[nz] / np.abs(want)[nz]
    return e


def zeros_match(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return bool((got[want == 0] == 0).all())


def signal_error(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not want.any():                                       # (a stretched length of 0: the result is zeros, and only zeros are right)
        return 0.0 if not got.any() else float("inf")
    return float(np.abs(got - want).max() / np.abs(want).max())


def bound(twin):
    """8 x the twin's figure, inside [2e-6, 1e-3]."""
    return min(max(8.0 * float(twin), 2e-6), 1e-3)


# ------------------------------------------------------------------------------------------------- peak normalisation
def peak_positions(ln, nb):
    """The indices a spike is placed at in turn, where they exist in a signal of ln samples."""
    want = (0, 255, 256, nb * 256 - 1, nb * 256, ln - 1)
    return [p if p < ln else None for p in want]


def peak_signal(ln, seed, at, negative=False):
    """White noise scaled below 1 with one sample of magnitude PEAK_SPIKE at index `at` (None: at the last sample)."""
    x = noise(ln, seed)
    x = (x * np.float32(0.9 / max(np.abs(x).max(), 1e-30))).astype(np.float32)
    assert np.abs(x).max() < 1.0
    x[ln - 1 if at is None else at] = -PEAK_SPIKE if negative else PEAK_SPIKE
    return x


def peak_want(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.max(np.abs(x))


# ------------------------------------------------------------------------------------------------- mixer
def mix_case(track_len, seed=0):
    """(notes, events [(start, note)]) for one track length: events at 0, 1023 and 1024 where they fit, one that ends on the last sample,
    one of length 1, three deep overlaps.  Every event fits the track."""
    lens = [n for n in (1, 7, 300, 1024, 1030) if n <= track_len]
    notes = [noise(n, seed + 10 * track_len + i) for i, n in enumerate(lens)]
    ev = []
    for start in (0, 1023, 1024):
        for i, n in enumerate(lens):
            if start + n <= track_len:
                ev.append((start, i))
    ev.append((track_len - lens[-1], len(lens) - 1))        # ends on the last sample
    ev.append((track_len - 1, 0))                           # one sample, the last
    ev += [(0, 0)] * 3                                      # three deep at sample 0
    if track_len > 300:
        ev += [(track_len - 300 - k, lens.index(300)) for k in (0, 1, 2)]
    return notes, ev


def mix_tables(notes, events, track_len):
    """(flat notes, ev [n][3] = start, offset, length; blk_ptr; blk_ev): the per-block lists arranger.mix_lists builds, restated."""
    offs = np.concatenate([[0], np.cumsum([len(x) for x in notes])]).astype(np.int64)
    ev = np.array([(s, offs[i], len(notes[i])) for s, i in events], np.int32).reshape(-1, 3)
    nblk = (track_len + SPB - 1) // SPB
    per = [[e for e, (s, _, n) in enumerate(ev.tolist()) if n > 0 and s < (b + 1) * SPB and s + n > b * SPB] for b in range(nblk)]
    ptr = np.zeros(nblk + 1, np.int32)
    ptr[1:] = np.cumsum([len(p) for p in per])
    return np.concatenate(notes).astype(np.float32), ev, ptr, np.array([e for p in per for e in p], np.int32)


def mix_numpy(notes, events, track_len):
    """numpy's float32 += float64 in event order: what ds_mix_notes equals bit for bit."""
    want = np.zeros(track_len, np.float32)
    for start, i in events:
        want[start:start + len(notes[i])] += notes[i].astype(np.float64)
    return want


def mix_walk(flat, ev, ptr, lst, n_blk_ev, track_len):
    """mix_notes_kernel<false>'s walk on a caller's lists: block b adds events lst[max(ptr[b], 0) : min(ptr[b + 1], n_blk_ev)] in list order,
    skipping ids outside [0, n_ev) and events whose (offset, length) leaves `flat`.  Returns (track, blocks that met such an entry)."""
    track = np.zeros(track_len, np.float32)
    touched = set()
    nblk = (track_len + SPB - 1) // SPB
    for b in range(nblk):
        if ptr[b] < 0 or ptr[b + 1] > n_blk_ev:
            touched.add(b)
        lo, hi = b * SPB, min((b + 1) * SPB, track_len)
        for e in range(max(int(ptr[b]), 0), min(int(ptr[b + 1]), n_blk_ev)):
            i = int(lst[e])
            if i < 0 or i >= len(ev):
                touched.add(b)
                continue
            start, off, n = (int(v) for v in ev[i])
            if not fits(off, n, len(flat)):
                touched.add(b)
                continue
            a, z = max(lo, start), min(hi, start + n)
            if a < z:
                track[a:z] += flat[off + a - start:off + z - start].astype(np.float64)
    return track, touched


# ------------------------------------------------------------------------------------------------- case data (computed once, shared, never changed)
@functools.lru_cache(maxsize=None)
def stft_case():
    t = build(STFT_LENGTHS, VOC_STEPS)
    sigs = [noise(n, 100 + i) for i, n in enumerate(STFT_LENGTHS)]
    return types.SimpleNamespace(t=t, sigs=sigs, want=[R.stft(s) for s in sigs], twin=[R.stft(s, np.float32) for s in sigs])


ZERO_SIGNAL, ZERO_FRAMES, ZERO_BINS = 6, slice(1, 3), slice(50, 60)           # a block of zero bins in two consecutive frames: want == 0 exists


@functools.lru_cache(maxsize=None)
def voc_case():
    t = build(STFT_LENGTHS, VOC_STEPS)
    specs = [R.stft(noise(n, 200 + i)).astype(np.complex64) for i, n in enumerate(STFT_LENGTHS)]
    specs[ZERO_SIGNAL][ZERO_FRAMES, ZERO_BINS] = 0
    want = [R.phase_vocoder(s.astype(np.complex128), r) for s, r in zip(specs, t.rates)]
    twin = [R.phase_vocoder(s, r, np.float32) for s, r in zip(specs, t.rates)]
    return types.SimpleNamespace(t=t, specs=specs, want=want, twin=twin)


def caller_steps(nf, nout):
    """A caller's step_idx for one signal of nout >= 8 synthesis frames: -1 (right frame only), -2, nf - 1 (left frame only), nf, nf + 5
    (nothing), the rest inside."""
    assert nout >= 8 and nf >= 3
    return np.array([0, -1, -2, nf - 1, nf, nf + 5, 1, nf - 2] + [1] * (nout - 8), np.int32)


@functools.lru_cache(maxsize=None)
def istft_case():
    lengths, steps = [n for n, _ in ISTFT_CASES], [s for _, s in ISTFT_CASES]
    t = build(lengths, steps)
    vocs = [R.phase_vocoder(R.stft(noise(n, 300 + i)), r).astype(np.complex64) for i, (n, r) in enumerate(zip(lengths, t.rates))]
    slen = col(t, "SLEN")
    want = [R.istft(v.astype(np.complex128), n) for v, n in zip(vocs, slen)]
    twin = [R.istft(v, n, np.float32) for v, n in zip(vocs, slen)]
    return types.SimpleNamespace(t=t, vocs=vocs, want=want, twin=twin)


@functools.lru_cache(maxsize=None)
def rs_case():
    lengths, steps = [n for n, _ in RS_CASES], [s for _, s in RS_CASES]
    t = build(lengths, steps)
    ys = [noise(n, 400 + i) for i, n in enumerate(col(t, "SLEN"))]
    rows = list(zip(ys, t.rates, lengths, col(t, "NRES")))
    return types.SimpleNamespace(t=t, ys=ys, want=[resample_want(*r) for r in rows], twin=[resample_want(*r, np.float32) for r in rows])


def peak_batch(variant, scale=0):
    """The seven signals with the spike at position `variant` of peak_positions (the batch's nb; the last sample where that does not exist);
    signal 2's spike is negative.  scale: a power of two applied to everything."""
    nb = peak_blocks(max(PEAK_LENGTHS))
    xs = [peak_signal(n, 500 + i, peak_positions(n, nb)[variant], negative=i == 2) for i, n in enumerate(PEAK_LENGTHS)]
    return [np.ldexp(x, scale).astype(np.float32) for x in xs]
