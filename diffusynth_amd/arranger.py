"""The Arrangement tab's audio stage on the GPU: pitch shift, resample, mix-down, and the reference's Track / DiffSynth on top of it.

Replaces webUI/natural_language_guided_4/track_maker.py.  Per note event the reference normalises a sampled note (once per distinct
duration), runs ceil((note - 52) / 4) chained librosa.effects.pitch_shift calls on the host and adds the result into the track.  Here the
notes stay in HBM: ds_peak_normalize, then the chains as a shared-prefix tree (a note of `total` semitones shares its first i steps with
every note of the same duration and total' >= 4 i), level by level, every level ONE batched ds_pv_stft -> ds_pv_vocode -> ds_pv_istft ->
ds_resample_sinc sequence over all its nodes, then one ds_mix_notes per track.

Kept on purpose: the reference's rule for total <= 0 (range(ceil(total / 4)) is empty: notes at or below MIDI 52 are mixed unshifted).
Opt-in (`tune=`, off by default): shift every note to its event's pitch in BOTH directions, from a stated source pitch or from the one
pitch.estimate_pitch detects; signed chains through the same tree.
Opt-in (`pairing="midi"`, `perform=Performance(...)`, off by default): play the file as written — every close paired with the oldest
open note of its pitch, the tempo map integrated, velocity as level and the reference's own ADSR envelope (tools.adsr_envelope) gated at
the real note-off, both applied inside the mix (ds_mix_notes_shaped).
Opt-in (`master=Mastering(...)`, off by default): an RMS gain and a peak-hold look-ahead limiter behind the mix (ds_master_gain,
ds_master_limit; include/diffusynth_hip.h has the arithmetic), once per render, in arrange / get_music once on the sum of the tracks.
With Mastering(target_lufs=...) the gain is the one that takes the mix's K-weighted gated loudness (BS.1770) to the target instead
(ds_loudness, ds_loudness_gain between the two; diffusynth_amd/loudness.py).  With Mastering(true_peak=True) the ceiling is a true-peak
ceiling: the limiter's detector is the 4x interpolated envelope of the mix (ds_true_peak, ds_master_limit_tp; diffusynth_amd/true_peak.py).
Opt-in (`formant=Formant(...)`, off by default): every link of a chain keeps the note's spectral envelope where the source had it
(ds_pv_formant between ds_pv_vocode and ds_pv_istft: cepstral envelope, warped ratio, one more launch per level), so a note shifted two
octaves up is still the same instrument.  Beyond the reference; defined in include/diffusynth_hip.h.
Different on purpose: the resampler.  librosa's default (soxr_hq) is a closed third-party design; the windowed sinc of
include/diffusynth_hip.h (fc = 0.95 min(1, rate), 32 zero crossings, Kaiser beta 12) is this package's definition.

Everything that is floored or rounded — frame counts, the phase vocoder's time steps, round(len / rate), ceil(len * rate),
int(start_sec * sr) — is computed here on the host in float64 and handed to the kernels as integers and tables.  No CPU fallback.
"""
import bisect
import collections
import dataclasses
import itertools
import math

import numpy as np
import torch

from . import _lib as L
from .loudness import check_sample_rate as _lu_rate, energy_of as _lu_energy, measure as _lu_measure, result as _lu_result     # (the package's
# attribute `loudness` is the function of that name, not the module)
from .true_peak import TruePeak, measure as _tp_measure                                                                         # (likewise `true_peak`)

N_FFT, HOP = 4096, 1024
_NO_GPU = "diffusynth_amd arranger runs on MI355X only (%s); no CPU fallback"
_PV = L.PV
_MX = L.MX
_MS = L.MS


def _require_cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(_NO_GPU % what)


def rate_of(n_steps):
    return 2.0 ** (-float(n_steps) / 12.0)


def chain_steps(total, step_size=4):
    """The n_steps of the reference's chained calls (track_maker.py:37-45): empty for total <= 0."""
    return [min(step_size, total - i * step_size) for i in range(int(math.ceil(total / step_size)))]


def signed_chain(total, step_size=4, deadband=0.05):
    """The n_steps of a chain that shifts by any real `total` of either sign: [] inside the deadband (|total| < deadband semitones: 5 cents
    by default, below what is heard as mistuned), else sign * [step_size, ..., step_size, remainder].  chain_steps(total) for a positive integer."""
    if not abs(total) >= deadband:
        return []
    sign, a = (1 if total > 0 else -1), abs(total)
    n = int(math.ceil(a / step_size))
    return [sign * step_size] * (n - 1) + [sign * (a - (n - 1) * step_size)]


# ---------------------------------------------------------------------------------------------------- one batched pitch_shift
def _finite_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) and math.isfinite(v)


@dataclasses.dataclass(frozen=True, kw_only=True)
class Formant:
    """Formant-preserving pitch shifts (pitch_shift(formant=...), Track.render(formant=...), DiffSynth(formant=...)): every synthesis frame
    of the phase vocoder is multiplied, bin by bin, by the ratio of its own smoothed spectral envelope at the place the resampler will move
    the bin to and at the bin itself (ds_pv_formant; include/diffusynth_hip.h has the arithmetic), so the envelope stays where the source
    had it while the partials move.

    order: the lifter's cut-off in QUEFRENCY SAMPLES: the envelope keeps the cepstral coefficients up to it.  It must stay below the source's
    pitch period sample_rate / f0 (97 samples at MIDI 52 and 16 kHz), or the envelope follows the partials themselves; 1 .. DS_PV_ORDER_MAX.
    max_gain_db: the correction of a bin is held inside +- max_gain_db (0 < max_gain_db <= 60).
    track_pitch: a link of a chain entered at cumulative shift `lo` semitones gets max(4, floor(order min(1, 2^(-lo / 12)))): the period of
    its input has already shrunk by the shifts in front of it (a downward chain keeps `order`).  False: every link gets `order`."""
    order: int = 30
    max_gain_db: float = 24.0
    track_pitch: bool = True

    def __post_init__(self):
        if not isinstance(self.order, (int, np.integer)) or isinstance(self.order, (bool, np.bool_)) or not 1 <= self.order <= _PV["DS_PV_ORDER_MAX"]:
            raise ValueError(f"Formant: order must be an int in [1, {_PV['DS_PV_ORDER_MAX']}] (quefrency samples), not {self.order!r}")
        if not _finite_number(self.max_gain_db) or not 0 < self.max_gain_db <= _PV["DS_PV_GAIN_DB_MAX"]:
            raise ValueError(f"Formant: max_gain_db must be a number in (0, {_PV['DS_PV_GAIN_DB_MAX']}], not {self.max_gain_db!r}")
        if not isinstance(self.track_pitch, (bool, np.bool_)):
            raise ValueError(f"Formant: track_pitch must be a bool, not {self.track_pitch!r}")

    @property
    def limit(self):
        """max_gain_db in nepers, ln 10 / 20 per dB, as the fp32 value the kernel takes."""
        return float(np.float32(float(self.max_gain_db) * math.log(10.0) / 20.0))

    def node_order(self, lo):
        """The order of a link whose input sits `lo` semitones from the source."""
        if not self.track_pitch:
            return int(self.order)
        return max(4, int(math.floor(int(self.order) * min(1.0, 2.0 ** (-float(lo) / 12.0)))))


def _check_formant(formant):
    if formant is None or isinstance(formant, Formant):
        return formant
    raise ValueError(f"formant: None or a Formant, not {formant!r}")


class _Plan:
    """Host side of one batched pitch_shift: the signal table and the time-step tables (float64), packed for ONE upload.  orders (one per
    signal; only with a Formant) appends ds_pv_formant's order and warp = fl32(1 / rate) arrays; without it the buffer is what it always was."""

    def __init__(self, lengths, n_steps, orders=None):
        n = len(lengths)
        tab = np.zeros((n, _PV["DS_PV_NI"]), dtype=np.int32)
        rates = np.zeros(n, dtype=np.float64)
        idx, alpha = [], []
        xoff = foff = toff = soff = 0
        for s, (ln, st) in enumerate(zip(lengths, n_steps)):
            rate = rate_of(st)
            nf = 1 + ln // HOP
            steps = np.arange(0, nf, rate, dtype=np.float64)
            slen = int(round(ln / rate))
            if ln < 1 or slen < 1:
                raise ValueError(f"pitch_shift: a signal of {ln} samples is too short for n_steps={st}")
            tab[s] = (xoff, ln, foff, nf, toff, len(steps), soff, slen, int(math.ceil(slen * rate)))
            rates[s] = rate
            idx.append(np.floor(steps).astype(np.int32))
            alpha.append(np.mod(steps, 1.0).astype(np.float32))
            xoff, foff, toff, soff = xoff + ln, foff + nf, toff + len(steps), soff + slen
        self.n, self.total_samples, self.total_frames, self.total_out, self.total_stretched = n, xoff, foff, toff, soff
        self.max_len, self.max_frames = int(tab[:, _PV["DS_PV_LEN"]].max()), int(tab[:, _PV["DS_PV_NF"]].max())
        self.max_out, self.max_stretched = int(tab[:, _PV["DS_PV_NOUT"]].max()), int(tab[:, _PV["DS_PV_SLEN"]].max())
        self.offsets = tab[:, _PV["DS_PV_XOFF"]].tolist()
        # [rates (8-byte aligned) | tab | step_idx | step_alpha] as one int32 buffer
        self.host = np.concatenate([rates.view(np.int32), tab.reshape(-1), np.concatenate(idx), np.concatenate(alpha).view(np.int32)])
        self.o_tab, self.o_idx, self.o_alpha = 2 * n, 2 * n + tab.size, 2 * n + tab.size + toff
        if orders is not None:
            if len(orders) != n:
                raise ValueError(f"pitch_shift: {len(orders)} orders for {n} signals")
            self.o_order, self.o_warp = self.host.size, self.host.size + n
            warp = (1.0 / rates).astype(np.float32)              # the float64 quotient rounded once: the fp32 factor of q = fl32(k) * warp
            self.host = np.concatenate([self.host, np.asarray(orders, dtype=np.int32), warp.view(np.int32)])


def _shift_flat(x, lengths, n_steps, formant=None, orders=None):
    """x: the signals back to back (fp32, CUDA) -> (the shifted signals back to back, their offsets).  Four entry points, six launches; with
    a Formant (orders: one per signal, default its order) ds_pv_formant between vocode and iSTFT: five and seven."""
    if formant is not None and orders is None:
        orders = [formant.order] * len(lengths)
    p = _Plan(lengths, n_steps, orders if formant is not None else None)
    dev = x.device
    tables = torch.from_numpy(p.host).to(dev)
    base = tables.data_ptr()
    rates, tab, idx, alpha = base, base + 4 * p.o_tab, base + 4 * p.o_idx, base + 4 * p.o_alpha
    spec = torch.empty(p.total_frames * (N_FFT // 2 + 1) * 2, dtype=torch.float32, device=dev)
    voc = torch.empty(p.total_out * (N_FFT // 2 + 1) * 2, dtype=torch.float32, device=dev)
    ws = torch.empty(L.load().ds_pv_istft_ws_bytes(p.total_out) // 4, dtype=torch.float32, device=dev)
    ys = torch.empty(p.total_stretched, dtype=torch.float32, device=dev)
    out = torch.empty(p.total_samples, dtype=torch.float32, device=dev)
    st = L.current_stream()
    L.call("ds_pv_stft", x.data_ptr(), tab, p.n, p.max_frames, p.total_samples, p.total_frames, spec.data_ptr(), st)
    L.call("ds_pv_vocode", spec.data_ptr(), tab, idx, alpha, p.n, p.total_frames, p.total_out, voc.data_ptr(), st)
    if formant is not None:
        L.call("ds_pv_formant", voc.data_ptr(), tab, base + 4 * p.o_order, base + 4 * p.o_warp, formant.limit, p.n, p.max_out, p.total_out, st)
    L.call("ds_pv_istft", voc.data_ptr(), tab, p.n, p.max_out, p.max_stretched, p.total_out, p.total_stretched, ws.data_ptr(), ys.data_ptr(), st)
    L.call("ds_resample_sinc", ys.data_ptr(), tab, rates, p.n, p.max_len, p.total_stretched, p.total_samples, out.data_ptr(), st)
    return out, p.offsets


def _as_list(signals, what):
    """(B, L) tensor or list of 1-D tensors -> (list of contiguous fp32 1-D CUDA tensors, was_tensor)."""
    if isinstance(signals, torch.Tensor):
        _require_cuda(signals, what)
        if signals.dim() != 2:
            raise ValueError(f"{what}: expected a (B, L) tensor or a list of 1-D tensors")
        return [r for r in signals.detach().float().contiguous()], True
    sigs = list(signals)
    for s in sigs:
        _require_cuda(s, what)
        if s.dim() != 1:
            raise ValueError(f"{what}: expected a (B, L) tensor or a list of 1-D tensors")
    return [s.detach().float().contiguous() for s in sigs], False


def _per_signal(v, n, what):
    if isinstance(v, (int, float, np.integer, np.floating)):
        return [v] * n
    v = [x.item() if isinstance(x, (torch.Tensor, np.generic)) else x for x in v]
    if len(v) != n:
        raise ValueError(f"{what}: {len(v)} values for {n} signals")
    return v


@torch.no_grad()
def pitch_shift(signals, n_steps, sample_rate=16000, n_fft=4096, hop_length=None, *, formant=None):
    """librosa.effects.pitch_shift(y, sr, n_steps, n_fft=4096, hop_length=1024) for a batch: a (B, L) CUDA tensor or a list of 1-D CUDA
    tensors of different lengths, n_steps a number or one per signal (any real value of either sign) -> the same shapes, fp32.
    sample_rate does not enter the arithmetic (as in librosa: only the ratio does).  formant (a Formant; None: librosa's shift, today's
    bits) keeps every signal's spectral envelope in place, with the Formant's order for this one link."""
    formant = _check_formant(formant)
    if n_fft != N_FFT or (hop_length is not None and hop_length != HOP):
        raise ValueError(f"pitch_shift: n_fft {N_FFT} / hop_length {HOP} only (the reference's call)")
    sigs, was_tensor = _as_list(signals, "pitch_shift")
    if not sigs:
        return signals
    steps = _per_signal(n_steps, len(sigs), "pitch_shift")
    lengths = [s.numel() for s in sigs]
    out, offs = _shift_flat(sigs[0] if len(sigs) == 1 else torch.cat(sigs), lengths, steps, formant)
    if was_tensor:
        return out.view(len(sigs), lengths[0])
    return [out[o:o + n] for o, n in zip(offs, lengths)]


# ---------------------------------------------------------------------------------------------------- the shared-prefix tree
def shift_tree(requests, step_size=4):
    """requests: (signal key, total semitones) pairs -> levels; level i lists its nodes (key, parent cumulative, cumulative, n_steps), each
    (key, cumulative) once.  The chain of a request is the path (key, 0) -> (key, min(total, step_size)) -> ... -> (key, total)."""
    levels = []
    pending = sorted({(k, t) for k, t in requests if t > 0}, key=lambda kt: (str(kt[0]), kt[1]))
    i = 0
    while pending:
        lo = i * step_size
        nodes = []
        for k, t in pending:
            node = (k, lo, min(t, lo + step_size), min(step_size, t - lo))
            if node not in nodes:
                nodes.append(node)
        levels.append(nodes)
        pending = [(k, t) for k, t in pending if t > lo + step_size]
        i += 1
    return levels


def signed_tree(requests, step_size=4, deadband=0.05):
    """shift_tree for real totals of either sign (signed_chain's chains): the node behind i whole steps is (key, +-step_size * i), the last
    one (key, total) itself, so equal prefixes meet in one node by float equality and chains of opposite sign share only the root (key, 0).
    A cumulative names its level, its parent and its n_steps, so (key, cumulative) appears once."""
    levels, seen = [], set()
    for k, t in sorted({(k, t) for k, t in requests if signed_chain(t, step_size, deadband)}, key=lambda kt: (str(kt[0]), kt[1])):
        chain = signed_chain(t, step_size, deadband)
        sign, lo = (1 if t > 0 else -1), 0
        for i, st in enumerate(chain):
            cum = t if i == len(chain) - 1 else sign * step_size * (i + 1)
            if (k, cum) not in seen:
                seen.add((k, cum))
                while len(levels) <= i:
                    levels.append([])
                levels[i].append((k, lo, cum, st))
            lo = cum
    return levels


def _tree_arg(formant, *lead):
    """Trailing arguments of Track's calls of _run_tree / _run_levels: none without a Formant, so that the plain render calls the two
    exactly as it did before the mode existed (tests/test_pitch_cpu.py replaces them by two-argument stand-ins).  ONLY for those two
    internal calls: everything else, the public calls above all, hands `formant` on as it is — an explicit None must stay a None."""
    return () if formant is None else lead + (formant,)


def node_orders(nodes, formant):
    """The lifter order of every node of a level: Formant.node_order of the cumulative shift the node is entered at."""
    return [formant.node_order(lo) for _, lo, _, _ in nodes]


def _run_tree(sources, requests, step_size=4, formant=None):
    """sources {key: 1-D fp32 CUDA tensor}; -> {(key, cumulative): tensor} with (key, 0) = the source itself.  One batched launch sequence
    per level."""
    return _run_levels(sources, shift_tree(requests, step_size), formant)


def _run_levels(sources, levels, formant=None):
    """_run_tree on built levels (shift_tree's or signed_tree's).  With a Formant every node carries its own order; (key, cumulative) still
    names a node uniquely (its order follows from the cumulative of its parent), so the sharing is the same."""
    have = {(k, 0): v for k, v in sources.items()}
    for nodes in levels:
        parents = [have[(k, lo)] for k, lo, _, _ in nodes]
        lengths = [p.numel() for p in parents]
        out, offs = _shift_flat(parents[0] if len(parents) == 1 else torch.cat(parents), lengths, [st for _, _, _, st in nodes],
                                formant, None if formant is None else node_orders(nodes, formant))
        for (k, _, cum, _), o, n in zip(nodes, offs, lengths):
            have[(k, cum)] = out[o:o + n]
    return have


@torch.no_grad()
def pitch_shift_chain(signals, totals, step_size=4, *, signed=False, formant=None):
    """The reference's pitch_shift_librosa (track_maker.py:12-47) for a batch: ceil(total / step_size) chained shifts of at most step_size
    semitones; total <= 0 returns the input unchanged (the reference's loop is empty).  Signals that are the same tensor share the common
    prefix of their chains; the result is bit for bit what the chains run one by one give.  signed=True: real totals of either sign through
    signed_chain (a total inside its deadband returns the input).  formant (a Formant) keeps the envelope in place
    in every link, each with the order of the cumulative shift it is entered at."""
    formant = _check_formant(formant)
    if isinstance(signals, torch.Tensor) and signals.dim() == 2:
        _require_cuda(signals, "pitch_shift_chain")
        rows = list(signals)
    else:
        rows = list(signals)
        for s in rows:
            _require_cuda(s, "pitch_shift_chain")
    tot = _per_signal(totals, len(rows), "pitch_shift_chain")
    keys, sources = [], {}
    for s in rows:
        key = (s.data_ptr(), s.numel(), s.dtype)
        keys.append(key)
        if key not in sources:
            sources[key] = s.detach().float().contiguous()
    if signed:
        have = _run_levels(sources, signed_tree(list(zip(keys, tot)), step_size), formant)
        out = [have[(k, t)] if signed_chain(t, step_size) else s for s, k, t in zip(rows, keys, tot)]
    else:
        have = _run_tree(sources, [(k, t) for k, t in zip(keys, tot) if t > 0], step_size, formant)
        out = [s if t <= 0 else have[(k, t)] for s, k, t in zip(rows, keys, tot)]
    if isinstance(signals, torch.Tensor):
        return torch.stack([o.float() for o in out])
    return out


def pitch_shift_librosa(waveform, sample_rate, total_steps, step_size=4, n_fft=4096, hop_length=None, *, formant=None):
    """Drop-in for track_maker.pitch_shift_librosa on one CUDA waveform (formant: as in pitch_shift_chain)."""
    formant = _check_formant(formant)
    if n_fft != N_FFT or (hop_length is not None and hop_length != HOP):
        raise ValueError(f"pitch_shift_librosa: n_fft {N_FFT} / hop_length {HOP} only")
    _require_cuda(waveform, "pitch_shift_librosa")
    return pitch_shift_chain([waveform], [total_steps], step_size, formant=formant)[0]


# ---------------------------------------------------------------------------------------------------- peak normalisation, mix
def _flat_table(lengths):
    tab = np.zeros((len(lengths), _PV["DS_PV_NI"]), dtype=np.int32)
    tab[:, _PV["DS_PV_LEN"]] = lengths
    tab[1:, _PV["DS_PV_XOFF"]] = np.cumsum(lengths)[:-1]
    return tab


@torch.no_grad()
def peak_normalize(signals):
    """x / max|x| per signal (a true fp32 division, as numpy's): list of 1-D CUDA tensors -> list."""
    sigs, _ = _as_list(signals, "peak_normalize")
    lengths = [s.numel() for s in sigs]
    tab = _flat_table(lengths)
    x = sigs[0] if len(sigs) == 1 else torch.cat(sigs)
    dtab = torch.from_numpy(tab.reshape(-1)).to(x.device)
    ws = torch.empty(max(1, L.load().ds_peak_normalize_ws_bytes(len(sigs), max(lengths)) // 4), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    L.call("ds_peak_normalize", x.data_ptr(), dtab.data_ptr(), len(sigs), max(lengths), x.numel(), ws.data_ptr(), out.data_ptr(), L.current_stream())
    return [out[o:o + n] for o, n in zip(tab[:, _PV["DS_PV_XOFF"]].tolist(), lengths)]


def mix_lists(starts, lengths, track_len):
    """Per block of DS_MIX_BLOCK samples the ascending indices of the events that touch it: (blk_ptr, blk_ev) int32."""
    nblk = (track_len + L.MIX_BLOCK - 1) // L.MIX_BLOCK
    per = [[] for _ in range(nblk)]
    for e, (s, n) in enumerate(zip(starts, lengths)):
        if n > 0:
            for b in range(s // L.MIX_BLOCK, min(nblk - 1, (s + n - 1) // L.MIX_BLOCK) + 1):
                per[b].append(e)
    ptr = np.zeros(nblk + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(p) for p in per])
    return ptr, np.array([e for p in per for e in p], dtype=np.int32)


def _linspace_step(start, stop, n):
    """numpy.linspace's step in float64; 0 for a segment of 0 or 1 samples (its single element is `start`)."""
    return (float(stop) - float(start)) / (n - 1) if n > 1 else 0.0


def shaped_rows(starts, offsets, note_lengths, gains, envelopes):
    """The event table of ds_mix_notes_shaped, int32 (n, DS_MX_NI) with the five floats as fp32 bit patterns.  envelopes: one
    (n_a, n_d, n_s, n_r, sustain) per event, or None for the weight g over the whole note (one sustain segment at level 1).  LEN is the
    mixed length min(note, n_a + n_d + n_s + n_r); the steps and the gain are float64 here and fp32 in the table."""
    n = len(starts)
    gains = [1.0] * n if gains is None else [float(g) for g in _per_signal(gains, n, "mix_notes: gains")]
    if envelopes is None:
        envelopes = [(0, 0, ln, 0, 1.0) for ln in note_lengths]
    if len(envelopes) != n:
        raise ValueError(f"mix_notes: {len(envelopes)} envelopes for {n} events")
    ev = np.zeros((n, _MX["DS_MX_NI"]), dtype=np.int32)
    fv = ev.view(np.float32)
    for e, (g, (na, nd, ns, nr, sus)) in enumerate(zip(gains, envelopes)):
        seg = [int(v) for v in (na, nd, ns, nr)]
        if min(seg) < 0 or seg != [na, nd, ns, nr] or not math.isfinite(sus) or not math.isfinite(g):
            raise ValueError(f"mix_notes: event {e}: segment lengths must be integers >= 0, gain and sustain finite (got {(g, na, nd, ns, nr, sus)})")
        if sum(seg) > 2 ** 31 - 1:
            raise ValueError(f"mix_notes: event {e}: an envelope of {sum(seg)} samples (at most 2^31 - 1)")
        ev[e, :_MX["DS_MX_NI_PLAIN"]] = (starts[e], offsets[e], min(note_lengths[e], sum(seg)))
        ev[e, _MX["DS_MX_NA"]:_MX["DS_MX_NR"] + 1] = seg
        fv[e, _MX["DS_MX_GAIN"]], fv[e, _MX["DS_MX_SUSTAIN"]] = g, sus
        fv[e, _MX["DS_MX_STEP_A"]] = _linspace_step(0.0, 1.0, seg[0])
        fv[e, _MX["DS_MX_STEP_D"]] = _linspace_step(1.0, sus, seg[1])
        fv[e, _MX["DS_MX_STEP_R"]] = _linspace_step(sus, 0.0, seg[3])
    return ev


@torch.no_grad()
def mix_notes(notes, events, track_len, *, gains=None, envelopes=None):
    """notes: list of 1-D fp32 CUDA tensors; events: (start sample, note index) in mixing order -> the (track_len,) fp32 track, every sample
    the sum of the notes covering it in event order (ds_mix_notes).

    gains (one float per event) and / or envelopes (one (n_a, n_d, n_s, n_r, sustain) per event: the segment lengths of adsr_envelope in
    samples) select ds_mix_notes_shaped: every note sample is weighted by fl(g_e env_e(j)) as it is added, nothing per event is
    materialised.  envelopes=None weights the whole note by g_e.  An event then ends with its envelope (the mixed length
    min(len(note), n_a + n_d + n_s + n_r)), for the fit check and for the per-block lists alike."""
    sigs, _ = _as_list(notes, "mix_notes")
    lengths = [s.numel() for s in sigs]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    shaped = gains is not None or envelopes is not None
    events = list(events)
    mixed = [lengths[i] for _, i in events]              # the fit check first, on Python integers: nothing is narrowed to int32 before it
    if envelopes is not None:
        envelopes = list(envelopes)
        if len(envelopes) != len(events):
            raise ValueError(f"mix_notes: {len(envelopes)} envelopes for {len(events)} events")
        mixed = [min(m, sum(env[:4])) for m, env in zip(mixed, envelopes)]
    for (start, _), m in zip(events, mixed):
        if start < 0 or start + m > track_len:
            raise ValueError(f"mix_notes: a note of {m} samples at {start} does not fit a track of {track_len} samples")
    if shaped:
        ev = shaped_rows([s for s, _ in events], [offs[i] for _, i in events], [lengths[i] for _, i in events], gains, envelopes)
    else:
        ev = np.array([(s, offs[i], lengths[i]) for s, i in events], dtype=np.int32).reshape(-1, _MX["DS_MX_NI_PLAIN"])
    if not events or track_len == 0:
        return torch.zeros(track_len, dtype=torch.float32, device=sigs[0].device if sigs else "cuda")
    ptr, lst = mix_lists(ev[:, _MX["DS_MX_START"]].tolist(), ev[:, _MX["DS_MX_LEN"]].tolist(), track_len)
    flat = sigs[0] if len(sigs) == 1 else torch.cat(sigs)
    host = np.concatenate([ev.reshape(-1), ptr, lst, np.zeros(1, np.int32)])
    tables = torch.from_numpy(host).to(flat.device)
    base = tables.data_ptr()
    track = torch.empty(track_len, dtype=torch.float32, device=flat.device)
    L.call("ds_mix_notes_shaped" if shaped else "ds_mix_notes", flat.data_ptr(), flat.numel(), base, len(ev), base + 4 * ev.size,
           base + 4 * (ev.size + ptr.size), len(lst), track.data_ptr(), track_len, L.current_stream())
    return track


def _mix_nodes(have, placed, n, shape=None):
    """have {node: tensor}; placed: (node, start sample) per event in mixing order -> the track (every distinct node handed over once).
    shape: None or (gains, envelopes) per event for the shaped mix."""
    used, index = [], {}
    for node, _ in placed:
        if node not in index:
            index[node] = len(used)
            used.append(have[node])
    events = [(start, index[node]) for node, start in placed]
    if shape is None:
        return mix_notes(used, events, n)
    return mix_notes(used, events, n, gains=shape[0], envelopes=shape[1])


def _shape_arg(shape):
    """The plain mix is called exactly as before the shaped one existed."""
    return () if shape is None else (shape,)


# ---------------------------------------------------------------------------------------------------- performed mode: envelope, velocity
def adsr_segments(sample_rate, duration, attack_time, decay_time, sustain_level, release_time):
    """The segment lengths of the reference's tools.adsr_envelope (tools.py:280-288), its int(...) expressions: (n_a, n_d, n_s, n_r); the
    envelope is n_a + n_d + n_s + int(1.0 * sample_rate) samples long, zero behind the release."""
    if not release_time <= 1.0:
        raise ValueError("adsr_envelope: release_time > 1.0")
    n_a, n_d, n_r = int(attack_time * sample_rate), int(decay_time * sample_rate), int(release_time * sample_rate)
    return n_a, n_d, max(0, int(duration * sample_rate) - n_a - n_d), n_r


@torch.no_grad()
def adsr_envelope(signals, sample_rate, duration, attack_time, decay_time, sustain_level, release_time):
    """The reference's tools.adsr_envelope on the device for one 1-D CUDA signal, a (B, L) tensor or a ragged list; duration and the four
    envelope parameters a number or one per signal.  Per signal the result has n_a + n_d + n_s + int(1.0 * sample_rate) samples: the signal
    cut or zero-extended to that length, times attack / decay / sustain / release (numpy's linspace per segment) and zero behind the
    release.  One ds_mix_notes_shaped launch: one event per signal into the concatenated outputs.  fp32 in, fp32 out."""
    single = isinstance(signals, torch.Tensor) and signals.dim() == 1
    sigs, was_tensor = _as_list([signals] if single else signals, "adsr_envelope")
    if not sigs:
        return signals
    n = len(sigs)
    par = [_per_signal(v, n, "adsr_envelope") for v in (duration, attack_time, decay_time, sustain_level, release_time)]
    envs, outs = [], []
    for dur, at, dt, sus, rt in zip(*par):
        seg = adsr_segments(sample_rate, dur, at, dt, sus, rt)
        envs.append(seg + (float(sus),))
        outs.append(seg[0] + seg[1] + seg[2] + int(1.0 * sample_rate))
    if min(s.numel() for s in sigs) < 1 or sum(outs) < 1:
        raise ValueError("adsr_envelope: an empty signal or an empty result")
    starts = np.concatenate([[0], np.cumsum(outs)]).tolist()
    flat = mix_notes(sigs, [(starts[i], i) for i in range(n)], starts[-1], envelopes=envs)
    if single:
        return flat
    if was_tensor and len(set(outs)) == 1:
        return flat.view(n, outs[0])
    return [flat[o:o + m] for o, m in zip(starts, outs)]


@dataclasses.dataclass(frozen=True, kw_only=True)
class Performance:
    """How a `pairing="midi"` track is played (Track.render(perform=...)): velocity as level and the reference's ADSR envelope gated at
    the real note-off.  gain = (velocity / 127) ** velocity_exponent (2: General MIDI's 40 log10(v / 127) dB; 0: every note at full level);
    the envelope is adsr_envelope's with duration = the held time; a note is sampled for max(held, 0.75) rounded up to a multiple of
    duration_step seconds (0.0625 s = one latent column at 16 kHz, so notes of one latent width share one sampled note)."""
    velocity_exponent: float = 2.0
    attack_time: float = 0.0
    decay_time: float = 0.0
    sustain_level: float = 1.0
    release_time: float = 0.1
    duration_step: float = 0.0625

    def __post_init__(self):
        for f in dataclasses.fields(self):
            if not _finite_number(getattr(self, f.name)):
                raise ValueError(f"Performance: {f.name} must be a finite number, not {getattr(self, f.name)!r}")
        if self.velocity_exponent < 0 or self.attack_time < 0 or self.decay_time < 0 or self.release_time < 0:
            raise ValueError("Performance: velocity_exponent, attack_time, decay_time and release_time must not be negative")
        if not 0.0 <= self.sustain_level <= 1.0:
            raise ValueError(f"Performance: sustain_level {self.sustain_level} outside [0, 1]")
        if self.release_time > 1.0:
            raise ValueError(f"Performance: release_time {self.release_time} > 1 (the sampled note's tail is 1 s)")
        if not self.duration_step > 0:
            raise ValueError(f"Performance: duration_step {self.duration_step} must be positive")

    def gain(self, velocity):
        return (velocity / 127.0) ** self.velocity_exponent

    def sampled_duration(self, held):
        """max(held, 0.75) rounded up to a multiple of duration_step; within 1e-9 steps above a multiple counts as that multiple."""
        return math.ceil(max(held, 0.75) / self.duration_step - 1e-9) * self.duration_step

    def envelope(self, held, sample_rate):
        """mix_notes' envelope entry of a note held for `held` seconds."""
        return adsr_segments(sample_rate, held, self.attack_time, self.decay_time, self.sustain_level, self.release_time) + (float(self.sustain_level),)


def _check_perform(perform):
    if perform is None or isinstance(perform, Performance):
        return perform
    raise ValueError(f"perform: None or a Performance, not {perform!r}")


def tempo_map_of(tracks):
    """The file's tempo map: the set_tempo messages of ALL tracks as (absolute tick, tempo), ordered by tick (track order, then message
    order, within a tick: of several entries on one tick the last holds)."""
    out = []
    for track in tracks:
        now = 0
        for msg in track:
            now += msg.time
            if msg.type == "set_tempo":
                out.append((now, msg.tempo))
    return sorted(out, key=lambda tt: tt[0])


# ---------------------------------------------------------------------------------------------------- mastering: gain, limiter
@dataclasses.dataclass(frozen=True, kw_only=True)
class Mastering:
    """The stage behind a mix (master(), Track.render(master=...), DiffSynth(master=...)): a gain that takes the signal to target_rms (at
    most max_gain; None: no gain), then a limiter that keeps |y| <= ceiling: the gain a sample needs is held for `hold` seconds behind it,
    reached `lookahead` seconds ahead of it and smoothed by a moving average of 2 lookahead + 1 samples, so it never exceeds what any sample
    needs (include/diffusynth_hip.h).  Times are floored to samples as int(t * sample_rate).  The defaults are choices, not
    measurements: the reference's tools.rms_normalize default, 20 dB, -1 dBFS, 5 ms and 50 ms.

    target_lufs (in [-70, 0]; target_rms must then be None) makes the gain the one that takes the signal's K-weighted gated loudness
    (BS.1770: loudness()) to that many LUFS, at most max_gain; a signal with nothing to measure keeps a gain of 1.

    true_peak=True (only True or False) makes the ceiling a true-peak ceiling (dBTP): the limiter's detector becomes the envelope of the
    4x interpolated input (true_peak()) instead of the samples' magnitudes.  The sample peak is still held to the ceiling
    exactly.  The true peak of the result is not bounded exactly, because a gain that varies in time does not commute with the
    interpolator: it rests on the look-ahead, whose smoothing keeps the gain slow against the interpolator's 12 samples.  At the
    defaults the measured overshoot on the test signals of DESIGN §7r is below 0.01 dB; with lookahead=0 the gain steps from sample to
    sample and the bound does not hold (1.6 dB over on hard-clipped noise)."""
    target_rms: float | None = 0.1
    max_gain: float = 10.0
    ceiling: float = 10 ** (-1 / 20)
    lookahead: float = 0.005
    hold: float = 0.05
    target_lufs: float | None = None
    true_peak: bool = False

    def __post_init__(self):
        if not isinstance(self.true_peak, (bool, np.bool_)):
            raise ValueError(f"Mastering: true_peak must be True or False, not {self.true_peak!r}")
        for f in dataclasses.fields(self):
            if f.name == "true_peak":
                continue
            v = getattr(self, f.name)
            if not (_finite_number(v) or (f.name in ("target_rms", "target_lufs") and v is None)):
                raise ValueError(f"Mastering: {f.name} must be a finite number, not {v!r}")
        if self.target_lufs is not None:
            if self.target_rms is not None:
                raise ValueError(f"Mastering: target_lufs {self.target_lufs!r} and target_rms {self.target_rms!r} are both set: one gain, so target_rms must be None beside a target_lufs")
            if not -70.0 <= self.target_lufs <= 0.0:
                raise ValueError(f"Mastering: target_lufs {self.target_lufs!r} outside [-70, 0]")
        for name in ("target_rms", "max_gain"):                 # (the kernels take them as fp32)
            v = getattr(self, name)
            if v is not None and not (v > 0 and 0 < float(np.float32(v)) < math.inf):
                raise ValueError(f"Mastering: {name} must be positive (and a finite, non-zero fp32 value), not {v!r}")
        if not (0.0 < self.ceiling <= 1.0 and float(np.float32(self.ceiling)) > 0):
            raise ValueError(f"Mastering: ceiling {self.ceiling} outside (0, 1]")
        if self.lookahead < 0:
            raise ValueError(f"Mastering: lookahead {self.lookahead} must not be negative")
        if self.hold < self.lookahead:
            raise ValueError(f"Mastering: hold {self.hold} < lookahead {self.lookahead} (the hold covers the look-ahead: that is why the gain never exceeds what a sample needs)")

    def samples(self, sample_rate):
        """(A, R): lookahead and hold in samples, floored; ValueError above the kernels' caps."""
        if not isinstance(sample_rate, (int, np.integer)) or isinstance(sample_rate, (bool, np.bool_)) or sample_rate <= 0:
            raise ValueError(f"master: sample_rate must be a positive int, not {sample_rate!r}")
        if self.target_lufs is not None:
            _lu_rate(sample_rate, "master (target_lufs)")
        a, r = int(self.lookahead * int(sample_rate)), int(self.hold * int(sample_rate))
        if a > _MS["DS_MS_MAX_LOOKAHEAD"]:
            raise ValueError(f"master: lookahead {self.lookahead} s is {a} samples at {sample_rate} Hz (at most {_MS['DS_MS_MAX_LOOKAHEAD']})")
        if r > _MS["DS_MS_MAX_HOLD"]:
            raise ValueError(f"master: hold {self.hold} s is {r} samples at {sample_rate} Hz (at most {_MS['DS_MS_MAX_HOLD']})")
        return a, r


class MasterStats(collections.namedtuple("MasterStats", "gain rms peak min_gain limited")):
    """Per signal, as device tensors (reading them is the caller's copy): the gain applied, the input's RMS and peak (fp32), the smallest
    limiter gain and the number of samples whose limiter gain is below 1 (int32)."""
    __slots__ = ()


def _check_master(master):
    if master is None or isinstance(master, Mastering):
        return master
    raise ValueError(f"master: None or a Mastering, not {master!r}")


def _signals_of(signals, who):
    """(fp32 contiguous 1-D CUDA tensors, lengths, single, was_tensor) of a 1-D tensor, a (B, L) tensor or a list of 1-D tensors; every
    ValueError comes before the device is asked for."""
    single = isinstance(signals, torch.Tensor) and signals.dim() == 1
    was_tensor = isinstance(signals, torch.Tensor) and not single
    if was_tensor and signals.dim() != 2:
        raise ValueError(f"{who}: signals: expected a 1-D tensor, a (B, L) tensor or a list of 1-D tensors")
    try:
        sigs = [signals] if single else list(signals)
    except TypeError:
        raise ValueError(f"{who}: signals: expected a 1-D tensor, a (B, L) tensor or a list of 1-D tensors") from None
    if not sigs:
        raise ValueError(f"{who}: signals: no signals")
    for s in sigs:
        if not isinstance(s, torch.Tensor) or s.dim() != 1:
            raise ValueError(f"{who}: signals: expected a 1-D tensor, a (B, L) tensor or a list of 1-D tensors")
        if s.numel() < 1:
            raise ValueError(f"{who}: signals: an empty signal")
        if s.numel() > _MS["DS_MS_MAX_LEN"]:
            raise ValueError(f"{who}: signals: a signal of {s.numel()} samples (at most 2^24 = {_MS['DS_MS_MAX_LEN']})")
    for s in sigs:
        _require_cuda(s, who)
    sigs = [s.detach().float().contiguous() for s in sigs]
    return sigs, [s.numel() for s in sigs], single, was_tensor


@torch.no_grad()
def master(signals, mastering=Mastering(), *, sample_rate=16000, pcm16=False, return_stats=False, return_loudness=False, return_true_peak=False):
    """Gain and limiter (Mastering) for one 1-D CUDA tensor, a (B, L) tensor or a list of 1-D tensors of different lengths, each signal by
    itself -> the same container, fp32, or int16 = rint(y * 32767) with pcm16=True; with return_stats=True (result, MasterStats).
    One table upload, ds_master_gain and ds_master_limit, no device -> host copy.  A signal's result is the same bits alone and in a batch.
    With a target_lufs: ds_master_gain (no target: rms, peak), ds_loudness, ds_loudness_gain, ds_master_limit; MasterStats.gain is the
    gain applied.  return_loudness=True appends the Loudness of the INPUT to the return value (it is measured for that where the
    Mastering has no target_lufs).
    With true_peak=True: ds_master_gain, the LUFS pair where a target is set, ds_true_peak with the envelope of the input, then
    ds_master_limit_tp.  return_true_peak=True appends TruePeak(input, output) last, both fp32 device tensors: output from one more
    ds_true_peak on the result, input from one on x where the Mastering did not already make it.  With pcm16=True, output is the true
    peak of the fp32 result BEFORE it is quantised to int16 (the true peak of the int16 samples is not measured)."""
    if not isinstance(mastering, Mastering):
        raise ValueError(f"master: mastering must be a Mastering, not {mastering!r}")
    if not isinstance(return_true_peak, (bool, np.bool_)):
        raise ValueError(f"master: return_true_peak must be True or False, not {return_true_peak!r}")
    a, r = mastering.samples(sample_rate)
    lufs = mastering.target_lufs
    if return_loudness:
        _lu_rate(sample_rate, "master (return_loudness)")
    sigs, lengths, single, was_tensor = _signals_of(signals, "master")
    n, max_len = len(sigs), max(lengths)
    tab = _flat_table(lengths)
    x = sigs[0] if n == 1 else torch.cat(sigs)
    dev = x.device
    dtab = torch.from_numpy(tab.reshape(-1)).to(dev)
    ws = torch.empty(L.load().ds_master_ws_bytes(n, max_len) // 4, dtype=torch.float32, device=dev)      # (the allocator aligns far beyond 8 bytes)
    stats = torch.empty((n, _MS["DS_MS_NS"]), dtype=torch.float32, device=dev)
    limited = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty(x.numel(), dtype=torch.float32, device=dev)
    pcm = torch.empty(x.numel(), dtype=torch.int16, device=dev) if pcm16 else None
    target = 0.0 if mastering.target_rms is None else float(np.float32(mastering.target_rms))
    st = L.current_stream()
    L.call("ds_master_gain", x.data_ptr(), dtab.data_ptr(), n, max_len, x.numel(), target, float(np.float32(mastering.max_gain)), ws.data_ptr(),
           stats.data_ptr(), limited.data_ptr(), st)
    loud = None
    if lufs is not None or return_loudness:
        lu, cnt, _ = _lu_measure(x, dtab, lengths, int(sample_rate))
        loud = _lu_result(lu, cnt)
        if lufs is not None:
            L.call("ds_loudness_gain", lu.data_ptr(), n, _lu_energy(lufs), float(np.float32(mastering.max_gain)), stats.data_ptr(), st)
    tp_in = None
    if mastering.true_peak:
        tp_in, env = _tp_measure(x, dtab, lengths, True)
        L.call("ds_master_limit_tp", x.data_ptr(), env.data_ptr(), dtab.data_ptr(), n, max_len, x.numel(), float(np.float32(mastering.ceiling)), a, r,
               stats.data_ptr(), limited.data_ptr(), out.data_ptr(), L.ptr(pcm), st)
    else:
        L.call("ds_master_limit", x.data_ptr(), dtab.data_ptr(), n, max_len, x.numel(), float(np.float32(mastering.ceiling)), a, r, stats.data_ptr(),
               limited.data_ptr(), out.data_ptr(), L.ptr(pcm), st)
    peaks = None
    if return_true_peak:
        peaks = TruePeak(_tp_measure(x, dtab, lengths)[0] if tp_in is None else tp_in, _tp_measure(out, dtab, lengths)[0])
    res = pcm if pcm16 else out
    if was_tensor:
        res = res.view(n, lengths[0])
    elif not single:
        res = [res[o:o + m] for o, m in zip(tab[:, _PV["DS_PV_XOFF"]].tolist(), lengths)]
    ret = (res,)
    if return_stats:
        ret += (MasterStats(*(stats[:, _MS[k]] for k in ("DS_MS_GAIN", "DS_MS_RMS", "DS_MS_PEAK", "DS_MS_MIN_GAIN")), limited),)
    if return_loudness:
        ret += (loud,)
    if return_true_peak:
        ret += (peaks,)
    return ret[0] if len(ret) == 1 else ret


def _mastered(track, mastering, sample_rate, pcm16=False):
    """(track or its mastered form, MasterStats or None, Loudness or None, TruePeak or None); an empty track has nothing to master."""
    if mastering is None or track.numel() == 0:
        return (track.to(torch.int16) if pcm16 else track), None, None, None
    lufs, tp = mastering.target_lufs is not None, mastering.true_peak
    ret = master(track, mastering, sample_rate=sample_rate, pcm16=pcm16, return_stats=True, return_loudness=lufs, return_true_peak=tp)
    return ret[0], ret[1], (ret[2] if lufs else None), (ret[-1] if tp else None)


# ---------------------------------------------------------------------------------------------------- tuned mode
def _check_tune(tune):
    """None, "detect" or a finite real number (returned as float); anything else is a ValueError, before any other work."""
    if tune is None or (isinstance(tune, str) and tune == "detect"):
        return tune
    if isinstance(tune, (int, float, np.integer, np.floating)) and not isinstance(tune, (bool, np.bool_)) and math.isfinite(tune):
        return float(tune)
    raise ValueError(f"tune: None (the reference's rule), a MIDI pitch (a finite real number) or \"detect\", not {tune!r}")


def _source_pitches(tune, keys, normed, sample_rate):
    """{key: MIDI pitch of the normalised note}: the stated one, or ONE estimate_pitch call over all of them (nan = unpitched)."""
    if tune != "detect":
        return {k: tune for k in keys}
    from . import pitch
    est = pitch.estimate_pitch([normed[k] for k in keys], sample_rate=sample_rate)
    return dict(zip(keys, est.midi.tolist()))


# ---------------------------------------------------------------------------------------------------- Track (track_maker.py:50-187)
class NoteEvent:
    """A MIDI note event: note number, velocity, start time and duration in ticks."""

    def __init__(self, note, velocity, start_time, duration):
        self.note, self.velocity, self.start_time, self.duration = note, velocity, start_time, duration

    def __str__(self):
        return f"Note {self.note}, velocity {self.velocity}, start_time {self.start_time}, duration {self.duration}"


def tick2second(tick, ticks_per_beat, tempo):
    """mido.tick2second."""
    return tick * tempo * 1e-6 / ticks_per_beat


class Track:
    """The reference's Track for any iterable of mido-like messages (.type, .time, .is_meta, .note, .velocity, .tempo).

    pairing="reference" (the default) is the reference's reading of the file, bit for bit: a closing note_on closes the LAST opened note,
    velocities are the closing message's 0, meta deltas are dropped and a start is ticks x the tempo in force at the note.
    pairing="midi" reads the file as written: every message advances the clock; a note_on with velocity > 0 opens a note of its
    (channel, note) and a note_off or a note_on with velocity 0 closes the OLDEST open note of the same (channel, note) (an unmatched close is
    ignored, a note still open at the end closes at the track's last tick); events are ordered by note-on tick, then message order, and
    carry the opening velocity; seconds are the integral over tempo_map, a list of (absolute tick, tempo) (None: the track's own set_tempo
    messages; tempo_map_of(tracks) for a file), 500 000 us per beat before its first entry."""

    def __init__(self, track, ticks_per_beat, max_notes=100, *, pairing="reference", tempo_map=None):
        if pairing not in ("reference", "midi"):
            raise ValueError(f"Track: pairing \"reference\" or \"midi\", not {pairing!r}")
        if pairing == "reference" and tempo_map is not None:
            raise ValueError("Track: tempo_map needs pairing=\"midi\" (the reference pairing keeps the reference's tempo rule)")
        track = list(track)
        self._cum = None
        self.pairing = pairing
        self.tempo_events = self._parse_tempo_events(track)
        self.ticks_per_beat = ticks_per_beat
        self.max_notes = int(max_notes)
        if pairing == "midi":
            self.events = self._parse_midi_events(track)
            self._set_tempo_map(tempo_map_of([track]) if tempo_map is None else tempo_map)
        else:
            self.events = self._parse_note_events(track)

    @staticmethod
    def _parse_midi_events(track):
        now, held, done = 0, collections.defaultdict(collections.deque), []
        for order, msg in enumerate(track):
            now += msg.time
            if msg.type not in ("note_on", "note_off"):
                continue
            key = (getattr(msg, "channel", 0), msg.note)
            if msg.type == "note_on" and msg.velocity > 0:
                held[key].append((now, order, msg.velocity))
            elif held[key]:
                on, first, velocity = held[key].popleft()
                done.append((on, first, NoteEvent(msg.note, velocity, on, now - on)))
        for (_, note), queue in held.items():
            done.extend((on, first, NoteEvent(note, velocity, on, now - on)) for on, first, velocity in queue)
        return [e for _, _, e in sorted(done, key=lambda d: d[:2])]

    def _set_tempo_map(self, tempo_map):
        """Break points (tick, tempo, seconds at tick): the seconds summed segment by segment in float64."""
        ticks, tempi = [0], [500000]
        for tick, tempo in sorted(((int(t), int(u)) for t, u in tempo_map), key=lambda tt: tt[0]):
            if tick < 0 or tempo <= 0:
                raise ValueError(f"Track: tempo_map entry {(tick, tempo)}")
            if tick == ticks[-1]:
                tempi[-1] = tempo
            else:
                ticks.append(tick)
                tempi.append(tempo)
        secs = [0.0]
        for i in range(1, len(ticks)):
            secs.append(secs[-1] + tick2second(ticks[i] - ticks[i - 1], self.ticks_per_beat, tempi[i - 1]))
        self.tempo_map = list(zip(ticks, tempi))
        self._map = (ticks, tempi, secs)

    def seconds(self, tick):
        """pairing="midi": the time of an absolute tick, the integral of the tempo map."""
        ticks, tempi, secs = self._map
        i = bisect.bisect_right(ticks, tick) - 1
        return secs[i] + tick2second(tick - ticks[i], self.ticks_per_beat, tempi[i])

    def _parse_tempo_events(self, track):
        # as written in the reference: a non-meta message re-states the DEFAULT tempo, so a track without set_tempo plays at 500 000 us per beat
        out = []
        for msg in track:
            if msg.type == "set_tempo":
                out.append((msg.time, msg.tempo))
            elif not msg.is_meta:
                out.append((msg.time, 500000))
        return out

    def _parse_note_events(self, track):
        # a note_on with velocity 0 closes the LAST note_on with velocity > 0; note_off messages only advance the clock
        events, now, on = [], 0, None
        for msg in track:
            if not msg.is_meta:
                now += msg.time
                if msg.type == "note_on" and msg.velocity > 0:
                    on = now
                elif msg.type == "note_on" and msg.velocity == 0:
                    if on is None:
                        raise ValueError("Track: a closing note_on (velocity 0) before any note was opened")
                    events.append(NoteEvent(msg.note, msg.velocity, on, now - on))
        return events

    def _get_tempo_at(self, time_tick):
        # the reference walks tempo_events and returns the tempo in force when the elapsed ticks first exceed time_tick: a bisection over
        # the running sums (a preset track has thousands of entries, and _get_total_time asks once per event)
        ev = self.tempo_events
        if self._cum is None or self._cum[0] is not ev or len(self._cum[1]) != len(ev):
            self._cum = (ev, list(itertools.accumulate(dt for dt, _ in ev)))
        j = bisect.bisect_right(self._cum[1], time_tick)
        return ev[j - 1][1] if j > 0 else 500000

    def _get_total_time(self):
        total = 0
        for e in self.events:
            total += e.duration * tick2second(1, self.ticks_per_beat, self._get_tempo_at(e.start_time))
        return total + 10

    def schedule(self, sample_rate=16000, perform=None):
        """Host arithmetic of synthesize_track for the first max_notes events: (duration key, duration_sec, start_sample, note - 52) each.
        pairing="midi": start = int(seconds(on) * sample_rate), duration_sec = max(held, 0.75), with a Performance its sampled_duration."""
        perform = self._check_perform(perform)
        out = []
        if self.pairing == "midi":
            for e, held in zip(self.events, self.held()):
                dur = max(held, 0.75) if perform is None else perform.sampled_duration(held)
                out.append((str(dur), dur, int(self.seconds(e.start_time) * sample_rate), e.note - 52))
            return out
        for e in self.events[:self.max_notes]:
            spt = tick2second(1, self.ticks_per_beat, self._get_tempo_at(e.start_time))
            dur = max(e.duration * spt, 0.75)
            out.append((str(dur), dur, int(e.start_time * spt * sample_rate), e.note - 52))
        return out

    def _check_perform(self, perform):
        perform = _check_perform(perform)
        if perform is not None and self.pairing != "midi":
            raise ValueError("Track: perform needs pairing=\"midi\" (the reference pairing has no velocities: every one is the closing message's 0)")
        return perform

    def held(self):
        """pairing="midi": seconds from note-on to note-off (unfloored) of the first max_notes events."""
        return [self.seconds(e.start_time + e.duration) - self.seconds(e.start_time) for e in self.events[:self.max_notes]]

    def shape(self, sample_rate=16000, perform=None):
        """(gains, envelopes) of the played events for mix_notes: velocity as level, the envelope gated at the real note-off."""
        perform = self._check_perform(perform)
        if perform is None:
            return None
        return ([perform.gain(e.velocity) for e in self.events[:self.max_notes]], [perform.envelope(h, sample_rate) for h in self.held()])

    def mixed_lengths(self, note_lengths, sample_rate=16000, perform=None):
        """pairing="midi": samples each played event adds to the track: its note's length {duration key: samples}, cut where its envelope ends."""
        lens = [note_lengths[key] for key, _, _, _ in self.schedule(sample_rate, perform)]
        shape = self.shape(sample_rate, perform)
        return lens if shape is None else [min(n, sum(env[:4])) for n, env in zip(lens, shape[1])]

    def track_length(self, sample_rate=16000, note_lengths=None, perform=None):
        """pairing="reference": the reference's total time.  pairing="midi": the last sounding sample, max(start + mixed length) over the
        played events; note_lengths {duration key: samples} is needed there."""
        if self.pairing == "midi":
            if note_lengths is None:
                raise ValueError("Track.track_length: pairing=\"midi\" ends with its last sounding sample; give note_lengths {duration key: samples}")
            ends = [s[2] + m for s, m in zip(self.schedule(sample_rate, perform), self.mixed_lengths(note_lengths, sample_rate, perform))]
            return max(ends, default=0)
        if note_lengths is not None or perform is not None:
            raise ValueError("Track.track_length: note_lengths and perform need pairing=\"midi\"")
        return int(self._get_total_time() * sample_rate)

    last_pitches = None        # {duration key: MIDI pitch the note was taken to sit at, nan = unpitched} of the last tuned render

    last_master = None         # MasterStats of the last mastered render

    last_loudness = None       # Loudness of the last render's mix, where that render was mastered to a LUFS target (else None)
    last_true_peak = None      # TruePeak of the last render's mix, where that render's Mastering has true_peak=True (else None)

    @torch.no_grad()
    def render(self, note_fn, sample_rate=16000, return_tensor=True, notes=None, *, tune=None, perform=None, master=None, formant=None):
        """synthesize_track on the device.  note_fn(velocity, duration_sec) -> numpy array or tensor on either device, called once per distinct
        duration in event order (the reference's cache); notes: {duration key: tensor} sampled beforehand instead.  One peak normalisation,
        one tree of chains over the distinct (duration, note) pairs, one mix.

        tune=None: the reference's rule (shift by note - 52, nothing at or below 52).  tune=p (a real number): every source is taken to sit
        at MIDI p and each event is shifted by signed_chain(note - p), up or down; 52 is the reference's assumption without its <= 0 rule.
        tune="detect": one pitch.estimate_pitch call over the normalised notes; a pitched note of detected pitch p_k is shifted by
        signed_chain(note - p_k), an unpitched one (noise, percussion) follows the reference's rule.  The chains are planned on the host in
        float64, so "detect" costs exactly one extra device -> host copy per render (a period and a count per distinct note).
        last_pitches holds {duration key: p, p_k or nan} afterwards.

        perform (a Performance; pairing="midi" only) changes the last stage alone: the mix weights every event by its velocity's gain and
        by adsr_envelope's envelope of its held time (mix_notes(gains=, envelopes=)), and notes are sampled for the performed durations.
        Normalisation, the chains and tune= are the same and compose with it.

        master (a Mastering) adds one stage behind the mix: master(track, mastering, sample_rate=sample_rate), bit for bit; last_master
        holds its MasterStats, last_loudness the mix's Loudness where the Mastering has a target_lufs (else None), last_true_peak its
        TruePeak where the Mastering has true_peak=True (else None).  None (the default) is the render without it.

        formant (a Formant) changes the chains alone: every link keeps the note's spectral envelope in place (pitch_shift_chain(formant=)).
        It composes with tune, perform and master; None (the default) is the render without it."""
        formant = _check_formant(formant)
        tune = _check_tune(tune)
        perform = self._check_perform(perform)
        master = _check_master(master)
        if master is not None:
            master.samples(sample_rate)            # its refusals come before any device work
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU % "Track.render")
        sched, n, raw, shape = self._collect(note_fn, sample_rate, notes, perform)
        if not sched:
            track = torch.zeros(n, dtype=torch.float32, device="cuda")
        else:
            keys = list(raw)
            normed = dict(zip(keys, peak_normalize([raw[k] for k in keys])))
            if tune is None:
                track = self._mix_reference(sched, n, normed, shape, formant)
            else:
                track = self._mix_tuned(sched, n, normed, _source_pitches(tune, keys, normed, sample_rate), shape, formant)
        self.last_loudness = None
        self.last_true_peak = None
        if master is not None:
            track, self.last_master, self.last_loudness, self.last_true_peak = _mastered(track, master, sample_rate)
        return track if return_tensor else track.cpu().numpy()

    def _collect(self, note_fn, sample_rate, notes, perform=None):
        """(schedule, track length, {duration key: the raw 1-D fp32 CUDA note}, mix shape or None).  pairing="reference": with the fit
        check; pairing="midi": the track ends with its last sounding sample."""
        sched = self.schedule(sample_rate, perform)
        raw = {}
        for (key, dur, _, _), e in zip(sched, self.events):
            if key not in raw:
                s = notes[key] if notes is not None else note_fn(e.velocity, dur)
                s = torch.from_numpy(np.ascontiguousarray(s)) if isinstance(s, np.ndarray) else s
                raw[key] = s.detach().reshape(-1).float().cuda()
        if self.pairing == "midi":
            n = self.track_length(sample_rate, {key: s.numel() for key, s in raw.items()}, perform)
            return sched, n, raw, self.shape(sample_rate, perform)
        n = self.track_length(sample_rate)
        for key, _, start, _ in sched:
            if start + raw[key].numel() > n:
                raise ValueError(f"Track: a note of {raw[key].numel()} samples at sample {start} ends past the track's {n} samples")
        return sched, n, raw, None

    def _mix_reference(self, sched, n, normed, shape=None, formant=None):
        have = _run_tree(normed, [(key, total) for key, _, _, total in sched if total > 0], *_tree_arg(formant, 4))
        return _mix_nodes(have, [((key, max(total, 0)), start) for key, _, start, total in sched], n, *_shape_arg(shape))

    def _mix_tuned(self, sched, n, normed, pitches, shape=None, formant=None):
        """pitches {duration key: MIDI pitch of the normalised note, nan = unpitched}: the signed tree and the mix."""
        self.last_pitches = {key: float(pitches[key]) for key in normed}
        totals = []
        for key, _, _, total in sched:                                         # total = note - 52
            p = self.last_pitches[key]
            totals.append(max(total, 0) if math.isnan(p) else (total + 52) - p)
        have = _run_levels(normed, signed_tree([(key, t) for (key, _, _, _), t in zip(sched, totals)]), *_tree_arg(formant))
        return _mix_nodes(have, [((key, t if signed_chain(t) else 0), start) for (key, _, start, _), t in zip(sched, totals)], n, *_shape_arg(shape))

    def synthesize_track(self, diffSynthSampler, sample_rate=16000):
        """The reference's method: float32 numpy array."""
        return self.render(diffSynthSampler, sample_rate, return_tensor=False)


_UNSET = object()


# ---------------------------------------------------------------------------------------------------- DiffSynth (track_maker.py:190-322)
class DiffSynth:
    """The reference's DiffSynth: every distinct (instrument, duration) note of ALL tracks of a request is sampled through one
    SamplingBatcher (shared U-Net steps), decoded per width group, and arranged on the device; one device -> host copy of the music.

    The empty-prompt condition comes from text_encoder.get_text_features(**CLAP_tokenizer([""], ...)) when a text encoder is given (once per
    get_music: it is a constant) or from the keyword-only `condition` (a (1, D) tensor).  With text_encoder = a multi_modal_model over a
    clap_text.ClapTextTower (or the tower itself) that call runs on the device end to end; only the tokenizer stays outside.
    """

    def __init__(self, instruments_configs, noise_prediction_model, VAE_quantizer, VAE_decoder, text_encoder, CLAP_tokenizer, device,
                 model_sample_rate=16000, timesteps=1000, channels=4, freq_resolution=512, time_resolution=256, VAE_scale=4, squared=False, *,
                 condition=None, noise_device="philox", seed=None, tune=None, pairing="reference", perform=None, master=None, formant=None):
        self.noise_prediction_model, self.VAE_quantizer, self.VAE_decoder = noise_prediction_model, VAE_quantizer, VAE_decoder
        self.device, self.model_sample_rate, self.timesteps, self.channels = device, model_sample_rate, timesteps, channels
        self.freq_resolution, self.time_resolution, self.VAE_scale, self.squared = freq_resolution, time_resolution, VAE_scale, squared
        self.height = int(freq_resolution / VAE_scale)
        self.text_encoder, self.CLAP_tokenizer = text_encoder, CLAP_tokenizer
        self.instruments_configs = instruments_configs
        self.condition, self.noise_device, self.seed = condition, noise_device, seed
        self.tune = _check_tune(tune)                # Track.render's tune=, for every track of arrange / get_music
        if pairing not in ("reference", "midi"):
            raise ValueError(f"DiffSynth: pairing \"reference\" or \"midi\", not {pairing!r}")
        self.pairing = pairing                       # Track's pairing=, for every track get_music builds (with the file's tempo map for "midi")
        self.perform = _check_perform(perform)       # Track.render's perform=, for every track of arrange / get_music
        if self.perform is not None and pairing != "midi":
            raise ValueError("DiffSynth: perform needs pairing=\"midi\"")
        self.master = _check_master(master)          # master()'s stage behind the sum of the tracks of arrange / get_music
        self.formant = _check_formant(formant)       # Track.render's formant=, for every track of arrange / get_music
        self.last_master = None                      # MasterStats of the last mastered arrange (None: it was not mastered)
        self.last_loudness = None                    # Loudness of the last arrange's sum (None: it was not mastered to a LUFS target)
        self.last_true_peak = None                   # TruePeak of the last arrange's sum (None: its Mastering had no true_peak=True)
        self.last_batcher = None
        self.last_pitches = None                     # {(instrument name, duration_sec): MIDI pitch or nan} of the last tuned arrange

    def _condition(self):
        if self.text_encoder is not None:
            return self.text_encoder.get_text_features(**self.CLAP_tokenizer([""], padding=True, return_tensors="pt")).to(self.device)
        if self.condition is None:
            raise ValueError("DiffSynth: give a text_encoder / CLAP_tokenizer pair or the keyword `condition` (the empty prompt's embedding)")
        return self.condition.to(self.device)

    def note_width(self, duration_sec):
        return int(self.time_resolution * ((duration_sec + 1) / 4) / self.VAE_scale)

    def _submit(self, batcher, cfg, duration_sec, condition, seed):
        from .sampler import DiffSynthSampler
        width = self.note_width(duration_sec)
        s = DiffSynthSampler(self.timesteps, height=self.height, channels=self.channels, noise_strategy="repeat", mute=True, device=self.device,
                             max_batchsize=1, noise_device=self.noise_device)
        s.respace(list(np.linspace(0, self.timesteps - 1, cfg["sample_steps"], dtype=np.int32)))
        mask = torch.zeros((1, 1, self.height, width), dtype=torch.float32, device=self.device)
        mask[:, :, :, :int(self.time_resolution * (cfg["attack"] / 4) / self.VAE_scale)] = 1.0
        mask[:, :, :, -int(self.time_resolution * ((cfg["before_release"] + 1) / 4) / self.VAE_scale):] = 1.0
        kw = {} if seed is None else {"seed": seed}
        guide = torch.as_tensor(cfg["latent_representation"]).to(self.device)
        return batcher.submit(s, "inpaint_sample", (1, self.channels, self.height, width), cfg["noising_strength"],
                              guide, mask, return_tensor=True, condition=condition, sampler=cfg["sampler"],
                              use_dynamic_mask=True, end_noise_level_ratio=0.0, mask_flexivity=1.0, **kw)

    @torch.no_grad()
    def sample_notes(self, wanted):
        """wanted: (instrument name, duration_sec) pairs -> {pair: 1-D fp32 CUDA signal}.  One batcher for all of them; VQ, decoder and iSTFT
        once per latent width."""
        from .batching import SamplingBatcher
        from .vocoder import latents_to_audio
        wanted = list(dict.fromkeys(wanted))
        condition = self._condition()
        batcher = SamplingBatcher(self.noise_prediction_model)
        # the widest U-Net batch first: the engine's plans share one arena sized to the largest peak seen, and growing it drops the cached
        # plans — submitted in this order every (batch, width) plan is built once per request
        widths = [self.note_width(dur) for _, dur in wanted]
        rows = {w: widths.count(w) * w for w in widths}
        handles = [None] * len(wanted)
        for i in sorted(range(len(wanted)), key=lambda i: (-rows[widths[i]], widths.index(widths[i]), i)):
            name, dur = wanted[i]
            handles[i] = self._submit(batcher, self.instruments_configs[name], dur, condition, None if self.seed is None else self.seed + i)
        batcher.run()
        self.last_batcher = batcher
        latents = [h.result()[0][-1] for h in handles]
        out, groups = {}, {}
        for i, lat in enumerate(latents):
            groups.setdefault(lat.shape[-1], []).append(i)
        for idxs in groups.values():
            quantized = self.VAE_quantizer(torch.cat([latents[i] for i in idxs]))[0]
            audio = latents_to_audio(self.VAE_decoder, quantized)
            for j, i in enumerate(idxs):
                out[wanted[i]] = audio[j]
        return out

    @staticmethod
    def wanted_notes(tracks, instrument_names, sample_rate=16000, perform=None):
        """The (instrument name, duration_sec) pair of every event the tracks will mix, in track and event order (with a Performance: its
        sampled durations)."""
        return [(instrument_names[i], dur) for i, t in enumerate(tracks) for _, dur, _, _ in t.schedule(sample_rate, perform)]

    @torch.no_grad()
    def arrange(self, tracks, instrument_names, notes, sample_rate=16000, *, tune=_UNSET, perform=_UNSET, master=_UNSET, pcm16=False, formant=_UNSET):
        """The audio stage of get_music on sampled notes {(instrument name, duration_sec): signal}: normalise, chains and mix per track,
        then the sum of the zero-padded tracks (track_maker.py:316-322), all on the device.  tune (default: the constructor's) as in
        Track.render; with "detect" the distinct notes of ALL tracks are normalised in one launch and estimated in ONE estimate_pitch call
        (one extra device -> host copy per call), and each track is then what its own tuned render gives, bit for bit.  perform (default:
        the constructor's) as in Track.render, for tracks built with pairing="midi"; it composes with every form of tune.
        master (default: the constructor's; None: off) runs master()'s stage ONCE, on the sum of the tracks, which is then
        master(plain sum, mastering, sample_rate=sample_rate) bit for bit; pcm16=True returns its int16 form (it needs a master: the raw sum
        has no bound); last_master holds the MasterStats, or None (last_loudness, last_true_peak as in Track.render).  formant (default: the constructor's; None: off) as in Track.render, for
        the chains of every track."""
        formant = self.formant if formant is _UNSET else _check_formant(formant)
        tune = self.tune if tune is _UNSET else _check_tune(tune)
        perform = self.perform if perform is _UNSET else _check_perform(perform)
        master = self.master if master is _UNSET else _check_master(master)
        if master is None and pcm16:
            raise ValueError("DiffSynth: pcm16=True needs a master (the sum of the tracks has no bound: a 16-bit rounding of it would clip)")
        if master is not None:
            master.samples(sample_rate)            # its refusals come before any device work
        per_track = [{key: notes[(instrument_names[i], dur)] for key, dur, _, _ in t.schedule(sample_rate, perform)} for i, t in enumerate(tracks)]
        if tune == "detect":
            audios = self._arrange_detected(tracks, instrument_names, per_track, sample_rate, perform, formant)
        else:
            audios = [t.render(None, sample_rate, notes=per_track[i], tune=tune, perform=perform, formant=formant) for i, t in enumerate(tracks)]
            if tune is not None:
                self.last_pitches = {(instrument_names[i], dur): tune for i, t in enumerate(tracks) for _, dur, _, _ in t.schedule(sample_rate, perform)}
        full = torch.zeros(max(a.numel() for a in audios), dtype=torch.float32, device=audios[0].device)
        for a in audios:                           # the reference's order: full_audio += pad(audio), track by track
            full[:a.numel()] += a
        full, self.last_master, self.last_loudness, self.last_true_peak = _mastered(full, master, sample_rate, pcm16)
        return full

    def _arrange_detected(self, tracks, instrument_names, per_track, sample_rate, perform=None, formant=None):
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU % "DiffSynth.arrange")
        parts = [t._collect(None, sample_rate, per_track[i], perform) for i, t in enumerate(tracks)]
        ids, flat = {}, []                                                      # every distinct (instrument, duration) note once
        for i, (sched, _, raw, _) in enumerate(parts):
            for key, dur, _, _ in sched:
                if (instrument_names[i], dur) not in ids:
                    ids[(instrument_names[i], dur)] = len(flat)
                    flat.append(raw[key])
        audios = [torch.zeros(n, dtype=torch.float32, device="cuda") for _, n, _, _ in parts]
        if not flat:
            self.last_pitches = {}
            return audios
        normed = peak_normalize(flat)
        midi = _source_pitches("detect", list(range(len(flat))), normed, sample_rate)
        self.last_pitches = {name_dur: midi[j] for name_dur, j in ids.items()}
        for i, (sched, n, raw, shape) in enumerate(parts):
            if sched:
                own = {key: ids[(instrument_names[i], dur)] for key, dur, _, _ in sched}
                audios[i] = tracks[i]._mix_tuned(sched, n, {key: normed[j] for key, j in own.items()}, {key: midi[j] for key, j in own.items()},
                                                      shape, formant)
        return audios

    @torch.no_grad()
    def get_music(self, mid, instrument_names, sample_rate=16000, max_notes=100, return_tensor=False, *, pairing=_UNSET, perform=_UNSET,
                  master=_UNSET, pcm16=False, formant=_UNSET):
        """The reference's get_music.  pairing / perform (default: the constructor's): with pairing="midi" every track is built with the
        file's tempo map, tempo_map_of(mid.tracks), and the notes are sampled for the performed durations.  master / pcm16 as in arrange:
        the music is mastered on the device and still leaves it in one copy, of int16 samples (half the bytes) with pcm16=True.  formant as in arrange."""
        formant = self.formant if formant is _UNSET else _check_formant(formant)
        pairing = self.pairing if pairing is _UNSET else pairing
        perform = self.perform if perform is _UNSET else _check_perform(perform)
        master = self.master if master is _UNSET else _check_master(master)
        if master is None and pcm16:
            raise ValueError("DiffSynth.get_music: pcm16=True needs a master (the sum of the tracks has no bound: a 16-bit rounding of it would clip)")
        if perform is not None and pairing != "midi":
            raise ValueError("DiffSynth.get_music: perform needs pairing=\"midi\"")
        if pairing == "midi":
            tempo_map = tempo_map_of(mid.tracks)
            tracks = [Track(t, mid.ticks_per_beat, max_notes, pairing="midi", tempo_map=tempo_map) for t in mid.tracks]
        else:
            tracks = [Track(t, mid.ticks_per_beat, max_notes, pairing=pairing) for t in mid.tracks]
        assert len(tracks) <= len(
            instrument_names), f"len(tracks) = {len(tracks)} > {len(instrument_names)} = len(instrument_names)"
        assert sample_rate == self.model_sample_rate, "sample_rate != model_sample_rate"
        wanted = self.wanted_notes(tracks, instrument_names, sample_rate, perform)
        full = self.arrange(tracks, instrument_names, self.sample_notes(wanted) if wanted else {}, sample_rate, perform=perform, master=master, pcm16=pcm16,
                            formant=formant)
        return full if return_tensor else full.cpu().numpy()
