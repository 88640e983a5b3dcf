"""The Arrangement tab's audio stage on the GPU: pitch shift, resample, mix-down, and the reference's Track / DiffSynth on top of it.

Replaces webUI/natural_language_guided_4/track_maker.py.  Per note event the reference normalises a sampled note (once per distinct
duration), runs ceil((note - 52) / 4) chained librosa.effects.pitch_shift calls on the host and adds the result into the track.  Here the
notes stay in HBM: ds_peak_normalize, then the chains as a shared-prefix tree (a note of `total` semitones shares its first i steps with
every note of the same duration and total' >= 4 i), level by level, every level ONE batched ds_pv_stft -> ds_pv_vocode -> ds_pv_istft ->
ds_resample_sinc sequence over all its nodes, then one ds_mix_notes per track.

Kept on purpose: the reference's rule for total <= 0 (range(ceil(total / 4)) is empty: notes at or below MIDI 52 are mixed unshifted).
Opt-in (`tune=`, off by default): shift every note to its event's pitch in BOTH directions, from a stated source pitch or from the one
pitch.estimate_pitch detects; signed chains through the same tree.
Different on purpose: the resampler.  librosa's default (soxr_hq) is a closed third-party design; the windowed sinc of
include/diffusynth_hip.h (fc = 0.95 min(1, rate), 32 zero crossings, Kaiser beta 12) is this package's definition.

Everything that is floored or rounded — frame counts, the phase vocoder's time steps, round(len / rate), ceil(len * rate),
int(start_sec * sr) — is computed here on the host in float64 and handed to the kernels as integers and tables.  No CPU fallback.
"""
import bisect
import itertools
import math

import numpy as np
import torch

from . import _lib as L

N_FFT, HOP = 4096, 1024
_NO_GPU = "diffusynth_amd arranger runs on MI355X only (%s); no CPU fallback"
_PV = L.PV


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
class _Plan:
    """Host side of one batched pitch_shift: the signal table and the time-step tables (float64), packed for ONE upload."""

    def __init__(self, lengths, n_steps):
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


def _shift_flat(x, lengths, n_steps):
    """x: the signals back to back (fp32, CUDA) -> (the shifted signals back to back, their offsets).  Four entry points, six launches."""
    p = _Plan(lengths, n_steps)
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
def pitch_shift(signals, n_steps, sample_rate=16000, n_fft=4096, hop_length=None):
    """librosa.effects.pitch_shift(y, sr, n_steps, n_fft=4096, hop_length=1024) for a batch: a (B, L) CUDA tensor or a list of 1-D CUDA
    tensors of different lengths, n_steps a number or one per signal (any real value of either sign) -> the same shapes, fp32.
    sample_rate does not enter the arithmetic (as in librosa: only the ratio does)."""
    if n_fft != N_FFT or (hop_length is not None and hop_length != HOP):
        raise ValueError(f"pitch_shift: n_fft {N_FFT} / hop_length {HOP} only (the reference's call)")
    sigs, was_tensor = _as_list(signals, "pitch_shift")
    if not sigs:
        return signals
    steps = _per_signal(n_steps, len(sigs), "pitch_shift")
    lengths = [s.numel() for s in sigs]
    out, offs = _shift_flat(sigs[0] if len(sigs) == 1 else torch.cat(sigs), lengths, steps)
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


def _run_tree(sources, requests, step_size=4):
    """sources {key: 1-D fp32 CUDA tensor}; -> {(key, cumulative): tensor} with (key, 0) = the source itself.  One batched launch sequence
    per level."""
    return _run_levels(sources, shift_tree(requests, step_size))


def _run_levels(sources, levels):
    """_run_tree on built levels (shift_tree's or signed_tree's)."""
    have = {(k, 0): v for k, v in sources.items()}
    for nodes in levels:
        parents = [have[(k, lo)] for k, lo, _, _ in nodes]
        lengths = [p.numel() for p in parents]
        out, offs = _shift_flat(parents[0] if len(parents) == 1 else torch.cat(parents), lengths, [st for _, _, _, st in nodes])
        for (k, _, cum, _), o, n in zip(nodes, offs, lengths):
            have[(k, cum)] = out[o:o + n]
    return have


@torch.no_grad()
def pitch_shift_chain(signals, totals, step_size=4, *, signed=False):
    """The reference's pitch_shift_librosa (track_maker.py:12-47) for a batch: ceil(total / step_size) chained shifts of at most step_size
    semitones; total <= 0 returns the input unchanged (the reference's loop is empty).  Signals that are the same tensor share the common
    prefix of their chains; the result is bit for bit what the chains run one by one give.  signed=True: real totals of either sign through
    signed_chain (a total inside its deadband returns the input)."""
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
        have = _run_levels(sources, signed_tree(list(zip(keys, tot)), step_size))
        out = [have[(k, t)] if signed_chain(t, step_size) else s for s, k, t in zip(rows, keys, tot)]
    else:
        have = _run_tree(sources, [(k, t) for k, t in zip(keys, tot) if t > 0], step_size)
        out = [s if t <= 0 else have[(k, t)] for s, k, t in zip(rows, keys, tot)]
    if isinstance(signals, torch.Tensor):
        return torch.stack([o.float() for o in out])
    return out


def pitch_shift_librosa(waveform, sample_rate, total_steps, step_size=4, n_fft=4096, hop_length=None):
    """Drop-in for track_maker.pitch_shift_librosa on one CUDA waveform."""
    if n_fft != N_FFT or (hop_length is not None and hop_length != HOP):
        raise ValueError(f"pitch_shift_librosa: n_fft {N_FFT} / hop_length {HOP} only")
    _require_cuda(waveform, "pitch_shift_librosa")
    return pitch_shift_chain([waveform], [total_steps], step_size)[0]


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


@torch.no_grad()
def mix_notes(notes, events, track_len):
    """notes: list of 1-D fp32 CUDA tensors; events: (start sample, note index) in mixing order -> the (track_len,) fp32 track, every sample
    the sum of the notes covering it in event order."""
    sigs, _ = _as_list(notes, "mix_notes")
    lengths = [s.numel() for s in sigs]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    for start, i in events:
        if start < 0 or start + lengths[i] > track_len:
            raise ValueError(f"mix_notes: a note of {lengths[i]} samples at {start} does not fit a track of {track_len} samples")
    if not events:
        return torch.zeros(track_len, dtype=torch.float32, device=sigs[0].device if sigs else "cuda")
    ev = np.array([(s, offs[i], lengths[i]) for s, i in events], dtype=np.int32)
    ptr, lst = mix_lists(ev[:, 0].tolist(), ev[:, 2].tolist(), track_len)
    flat = sigs[0] if len(sigs) == 1 else torch.cat(sigs)
    host = np.concatenate([ev.reshape(-1), ptr, lst, np.zeros(1, np.int32)])
    tables = torch.from_numpy(host).to(flat.device)
    base = tables.data_ptr()
    track = torch.empty(track_len, dtype=torch.float32, device=flat.device)
    L.call("ds_mix_notes", flat.data_ptr(), flat.numel(), base, len(ev), base + 4 * ev.size, base + 4 * (ev.size + ptr.size), len(lst), track.data_ptr(),
           track_len, L.current_stream())
    return track


def _mix_nodes(have, placed, n):
    """have {node: tensor}; placed: (node, start sample) per event in mixing order -> the track (every distinct node handed over once)."""
    used, index = [], {}
    for node, _ in placed:
        if node not in index:
            index[node] = len(used)
            used.append(have[node])
    return mix_notes(used, [(start, index[node]) for node, start in placed], n)


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
    """The reference's Track for any iterable of mido-like messages (.type, .time, .is_meta, .note, .velocity, .tempo)."""

    def __init__(self, track, ticks_per_beat, max_notes=100):
        track = list(track)
        self._cum = None
        self.tempo_events = self._parse_tempo_events(track)
        self.events = self._parse_note_events(track)
        self.ticks_per_beat = ticks_per_beat
        self.max_notes = int(max_notes)

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

    def schedule(self, sample_rate=16000):
        """Host arithmetic of synthesize_track for the first max_notes events: (duration key, duration_sec, start_sample, note - 52) each."""
        out = []
        for e in self.events[:self.max_notes]:
            spt = tick2second(1, self.ticks_per_beat, self._get_tempo_at(e.start_time))
            dur = max(e.duration * spt, 0.75)
            out.append((str(dur), dur, int(e.start_time * spt * sample_rate), e.note - 52))
        return out

    def track_length(self, sample_rate=16000):
        return int(self._get_total_time() * sample_rate)

    last_pitches = None        # {duration key: MIDI pitch the note was taken to sit at, nan = unpitched} of the last tuned render

    @torch.no_grad()
    def render(self, note_fn, sample_rate=16000, return_tensor=True, notes=None, *, tune=None):
        """synthesize_track on the device.  note_fn(velocity, duration_sec) -> numpy array or tensor on either device, called once per distinct
        duration in event order (the reference's cache); notes: {duration key: tensor} sampled beforehand instead.  One peak normalisation,
        one tree of chains over the distinct (duration, note) pairs, one mix.

        tune=None: the reference's rule (shift by note - 52, nothing at or below 52).  tune=p (a real number): every source is taken to sit
        at MIDI p and each event is shifted by signed_chain(note - p), up or down; 52 is the reference's assumption without its <= 0 rule.
        tune="detect": one pitch.estimate_pitch call over the normalised notes; a pitched note of detected pitch p_k is shifted by
        signed_chain(note - p_k), an unpitched one (noise, percussion) follows the reference's rule.  The chains are planned on the host in
        float64, so "detect" costs exactly one extra device -> host copy per render (a period and a count per distinct note).
        last_pitches holds {duration key: p, p_k or nan} afterwards."""
        tune = _check_tune(tune)
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU % "Track.render")
        sched, n, raw = self._collect(note_fn, sample_rate, notes)
        if not sched:
            track = torch.zeros(n, dtype=torch.float32, device="cuda")
            return track if return_tensor else track.cpu().numpy()
        keys = list(raw)
        normed = dict(zip(keys, peak_normalize([raw[k] for k in keys])))
        if tune is None:
            track = self._mix_reference(sched, n, normed)
        else:
            track = self._mix_tuned(sched, n, normed, _source_pitches(tune, keys, normed, sample_rate))
        return track if return_tensor else track.cpu().numpy()

    def _collect(self, note_fn, sample_rate, notes):
        """(schedule, track length, {duration key: the raw 1-D fp32 CUDA note}) with the fit check."""
        sched = self.schedule(sample_rate)
        n = self.track_length(sample_rate)
        raw = {}
        for (key, dur, _, _), e in zip(sched, self.events):
            if key not in raw:
                s = notes[key] if notes is not None else note_fn(e.velocity, dur)
                s = torch.from_numpy(np.ascontiguousarray(s)) if isinstance(s, np.ndarray) else s
                raw[key] = s.detach().reshape(-1).float().cuda()
        for key, _, start, _ in sched:
            if start + raw[key].numel() > n:
                raise ValueError(f"Track: a note of {raw[key].numel()} samples at sample {start} ends past the track's {n} samples")
        return sched, n, raw

    def _mix_reference(self, sched, n, normed):
        have = _run_tree(normed, [(key, total) for key, _, _, total in sched if total > 0])
        return _mix_nodes(have, [((key, max(total, 0)), start) for key, _, start, total in sched], n)

    def _mix_tuned(self, sched, n, normed, pitches):
        """pitches {duration key: MIDI pitch of the normalised note, nan = unpitched}: the signed tree and the mix."""
        self.last_pitches = {key: float(pitches[key]) for key in normed}
        totals = []
        for key, _, _, total in sched:                                         # total = note - 52
            p = self.last_pitches[key]
            totals.append(max(total, 0) if math.isnan(p) else (total + 52) - p)
        have = _run_levels(normed, signed_tree([(key, t) for (key, _, _, _), t in zip(sched, totals)]))
        return _mix_nodes(have, [((key, t if signed_chain(t) else 0), start) for (key, _, start, _), t in zip(sched, totals)], n)

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
                 condition=None, noise_device="philox", seed=None, tune=None):
        self.noise_prediction_model, self.VAE_quantizer, self.VAE_decoder = noise_prediction_model, VAE_quantizer, VAE_decoder
        self.device, self.model_sample_rate, self.timesteps, self.channels = device, model_sample_rate, timesteps, channels
        self.freq_resolution, self.time_resolution, self.VAE_scale, self.squared = freq_resolution, time_resolution, VAE_scale, squared
        self.height = int(freq_resolution / VAE_scale)
        self.text_encoder, self.CLAP_tokenizer = text_encoder, CLAP_tokenizer
        self.instruments_configs = instruments_configs
        self.condition, self.noise_device, self.seed = condition, noise_device, seed
        self.tune = _check_tune(tune)                # Track.render's tune=, for every track of arrange / get_music
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
    def wanted_notes(tracks, instrument_names, sample_rate=16000):
        """The (instrument name, duration_sec) pair of every event the tracks will mix, in track and event order."""
        return [(instrument_names[i], dur) for i, t in enumerate(tracks) for _, dur, _, _ in t.schedule(sample_rate)]

    @torch.no_grad()
    def arrange(self, tracks, instrument_names, notes, sample_rate=16000, *, tune=_UNSET):
        """The audio stage of get_music on sampled notes {(instrument name, duration_sec): signal}: normalise, chains and mix per track,
        then the sum of the zero-padded tracks (track_maker.py:316-322), all on the device.  tune (default: the constructor's) as in
        Track.render; with "detect" the distinct notes of ALL tracks are normalised in one launch and estimated in ONE estimate_pitch call
        (one extra device -> host copy per call), and each track is then what its own tuned render gives, bit for bit."""
        tune = self.tune if tune is _UNSET else _check_tune(tune)
        per_track = [{key: notes[(instrument_names[i], dur)] for key, dur, _, _ in t.schedule(sample_rate)} for i, t in enumerate(tracks)]
        if tune == "detect":
            audios = self._arrange_detected(tracks, instrument_names, per_track, sample_rate)
        else:
            audios = [t.render(None, sample_rate, notes=per_track[i], tune=tune) for i, t in enumerate(tracks)]
            if tune is not None:
                self.last_pitches = {(instrument_names[i], dur): tune for i, t in enumerate(tracks) for _, dur, _, _ in t.schedule(sample_rate)}
        full = torch.zeros(max(a.numel() for a in audios), dtype=torch.float32, device=audios[0].device)
        for a in audios:                           # the reference's order: full_audio += pad(audio), track by track
            full[:a.numel()] += a
        return full

    def _arrange_detected(self, tracks, instrument_names, per_track, sample_rate):
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU % "DiffSynth.arrange")
        parts = [t._collect(None, sample_rate, per_track[i]) for i, t in enumerate(tracks)]
        ids, flat = {}, []                                                      # every distinct (instrument, duration) note once
        for i, (sched, _, raw) in enumerate(parts):
            for key, dur, _, _ in sched:
                if (instrument_names[i], dur) not in ids:
                    ids[(instrument_names[i], dur)] = len(flat)
                    flat.append(raw[key])
        audios = [torch.zeros(n, dtype=torch.float32, device="cuda") for _, n, _ in parts]
        if not flat:
            self.last_pitches = {}
            return audios
        normed = peak_normalize(flat)
        midi = _source_pitches("detect", list(range(len(flat))), normed, sample_rate)
        self.last_pitches = {name_dur: midi[j] for name_dur, j in ids.items()}
        for i, (sched, n, raw) in enumerate(parts):
            if sched:
                own = {key: ids[(instrument_names[i], dur)] for key, dur, _, _ in sched}
                audios[i] = tracks[i]._mix_tuned(sched, n, {key: normed[j] for key, j in own.items()}, {key: midi[j] for key, j in own.items()})
        return audios

    @torch.no_grad()
    def get_music(self, mid, instrument_names, sample_rate=16000, max_notes=100, return_tensor=False):
        tracks = [Track(t, mid.ticks_per_beat, max_notes) for t in mid.tracks]
        assert len(tracks) <= len(
            instrument_names), f"len(tracks) = {len(tracks)} > {len(instrument_names)} = len(instrument_names)"
        assert sample_rate == self.model_sample_rate, "sample_rate != model_sample_rate"
        wanted = self.wanted_notes(tracks, instrument_names, sample_rate)
        full = self.arrange(tracks, instrument_names, self.sample_notes(wanted) if wanted else {}, sample_rate)
        return full if return_tensor else full.cpu().numpy()
