#!/usr/bin/env python3
"""Drive the suite's shapes through the bounds-checked diagnostic library (GPU box):

    DS_LIB=libdiffusynth_hip_bounds.so python tools/bounds_sweep.py

Covers what the r01 abort pointed at (VQGAN encoder on (1,3,512,12) in bf16, narrow-BN tiles, empty split-K slices)
plus the production U-Net / decoder at ragged widths and split-K batch sizes, in both tiers.  Prints one line per
group and `BOUNDS OK` when ds_bounds_report() found no access outside its operand's extent."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DS_LIB", "libdiffusynth_hip_bounds.so")

import torch  # noqa: E402

from diffusynth_amd import _lib as L  # noqa: E402
from diffusynth_amd.synth import synth_input, synth_state_dict  # noqa: E402


def report(tag, fail):
    buf = C.create_string_buffer(4096)
    n = L.load().ds_bounds_report(buf, 4096, 1)
    msg = buf.value.decode()
    print(f"[bounds] {tag}: {n} violation record(s) {msg}", flush=True)
    if n != 0:
        fail.append((tag, n, msg))


def sweep_ui_images(fail):
    """The UI images (csrc/ui_images.hip): both paths of ds_stft_images (16-byte loads / one pixel per thread), ragged last blocks, rows and
    clips whose byte offset is not a multiple of 16, misaligned views, the second magnitude source, and ds_latent_image."""
    from diffusynth_amd import ui_images as U
    for B, F, T in ((2, 512, 64), (3, 512, 100), (1, 512, 27), (1, 512, 300), (1, 512, 16), (1, 128, 20), (1, 512, 1), (3, 512, 9),
                    (8, 512, 256), (2, 37, 5)):
        enc = synth_input("bs_ui%d_%d" % (F, T), (B, 3, F, T))
        U.stft_images(enc.cuda())
        flat = torch.zeros(enc.numel() + 1, device="cuda")
        flat[1:] = enc.flatten().cuda()
        U.stft_images(flat[1:].view(B, 3, F, T))
        amp = synth_input("bs_ui_amp%d_%d" % (F, T), (B, 2, F, T)).cuda()
        U.stft_images(enc.cuda(), amp)
    report("stft_images 10 shapes x (aligned, misaligned view, second magnitude source)", fail)
    for shape in ((1, 4, 128, 64), (3, 4, 16, 12), (2, 4, 5, 3), (64, 4, 128, 64)):
        U.latent_images(synth_input("bs_lat%d" % shape[3], shape).cuda())
    report("latent_image 4 shapes", fail)


def sweep_arranger(fail):
    """The arranger's audio stage (csrc/arranger.hip): ragged batches incl. a signal shorter than one hop and one of a single odd frame pair,
    both directions of the shift, the chain tree, peak normalisation, and a mix with notes at both ends of the track."""
    from diffusynth_amd import arranger as A
    sigs = [synth_input("bs_arr%d" % n, (n,)).cuda() for n in (28416, 77568, 30001, 4097, 1023, 50000, 2048, 1)]
    A.pitch_shift(sigs[:7], [1, 2, 3, 4, -3, 0.5, 4])
    A.pitch_shift(sigs[:7], [-12, 12, 0, -4, 7, 4, -1])
    A.pitch_shift(torch.stack([sigs[0], sigs[0]]), 4)
    report("pitch_shift 2 ragged batches of 7 + a (2, L) batch", fail)
    A.pitch_shift_chain([sigs[0], sigs[0], sigs[2], sigs[4]], [31, 5, 9, 2])
    report("pitch_shift_chain tree (8 levels)", fail)
    A.pitch_shift(sigs[:7], [-12, 12, 0, -4, 7, 4, -1], formant=A.Formant(order=512, max_gain_db=60))
    A.pitch_shift_chain([sigs[0], sigs[0], sigs[2], sigs[4]], [31, 5, 9, 2], formant=A.Formant())
    report("pitch_shift with a Formant (ds_pv_formant): a ragged batch of 7 at the caps + the chain tree with per-node orders", fail)
    normed = A.peak_normalize(sigs)
    report("peak_normalize 8 signals (1 .. 77568 samples)", fail)
    n = 100000
    A.mix_notes(normed, [(0, 0), (n - 77568, 1), (1023, 7), (n - 1, 7), (0, 7), (500, 3), (500, 3), (n - 1023, 4), (60000, 2)], n)
    A.mix_notes(normed[7:], [(3, 0)], 5)
    report("mix_notes 9 events over 98 blocks + a 5-sample track", fail)


def sweep_perform(fail):
    """The performed mode (ds_mix_notes_shaped in csrc/arranger.hip): events from sample 0 to the last sample, an event with every segment
    of 0 or 1 samples, envelopes longer and shorter than their notes, a 5-sample track, adsr_envelope on a ragged batch, and a performed
    render on top."""
    from diffusynth_amd import arranger as A
    sigs = [synth_input("bs_prf%d" % n, (n,)).cuda() for n in (28416, 5000, 2048, 1, 77568)]
    n = 100000
    events = [(0, 0), (n - 5000, 1), (1023, 3), (n - 1, 3), (500, 2), (500, 2), (n - 77568, 4), (60000, 0), (0, 4), (3000, 1), (70000, 2)]
    envs = [(1024, 1023, 1026, 4000, 0.6), (100, 200, 9000, 1600, 0.5), (1, 0, 0, 0, 1.0), (0, 1, 0, 0, 0.5), (1, 1, 1, 1, 0.25), (0, 0, 0, 0, 1.0),
            (3000, 5000, 60000, 9568, 0.4), (0, 0, 28416, 0, 1.0), (0, 0, 100, 16000, 1.0), (10, 20, 500, 300, 0.7), (0, 1, 0, 1, 0.0)]
    A.mix_notes(sigs, events, n, gains=[0.1 * (e + 1) for e in range(len(events))], envelopes=envs)
    A.mix_notes(sigs, events, n, gains=[1.0] * len(events))
    A.mix_notes(sigs[3:4], [(3, 0)], 5, gains=[0.5])
    A.mix_notes(sigs[1:2], [(0, 0)], 5, envelopes=[(1, 1, 2, 1, 0.5)])
    report("mix_notes shaped: 11 events over 98 blocks, whole-note gains, two 5-sample tracks", fail)
    A.adsr_envelope(sigs, 16000, [0.5, 1.0, 0.001, 0.0, 6.0], [0.01, 0.0, 0.0, 0.0, 1.5], [0.05, 0.0, 0.0005, 0.0, 0.25], [0.7, 1.0, 0.5, 0.0, 0.3],
                    [0.1, 0.0, 1.0, 0.5, 0.2])
    A.adsr_envelope(sigs[3], 7, 0.0, 0.0, 0.0, 1.0, 0.0)
    report("adsr_envelope ragged batch of 5 + a one-sample signal at 7 Hz", fail)
    rows = [(0, 0, 60, 100, 0, 0), (0, 0, 64, 50, 0, 0), (0, 120, 64, 0, 0, 0), (1, 360, 60, 0, 0, 0), (0, 0, 45, 127, 0, 0), (0, 2400, 45, 0, 0, 0)]
    import arranger_ref as R
    t = A.Track(R.messages(rows), 480, pairing="midi")
    t.render(lambda v, d: synth_input("bs_prf_note", (256 * (4 * int(16 * (d + 1)) - 1),)), perform=A.Performance(attack_time=0.01, release_time=0.3), tune=52.0)
    report("Track.render pairing=midi, performed and tuned", fail)


def sweep_pitch(fail):
    """Pitch detection (csrc/pitch.hip): a ragged batch with frameless signals at both ends and one sample either side of a frame, the
    largest LDS image (frame_length 2048, tau_max 1024, tau_min 2) with an odd hop, an odd frame length, the median at its frame limit, and
    the tuned arranger on top (signed chains of both signs)."""
    from diffusynth_amd import arranger as A
    from diffusynth_amd import pitch
    sigs = [synth_input("bs_pitch%d" % n, (n,)).cuda() for n in (100, 28416, 1313, 1314, 1570, 30001, 4097, 77568, 1)]
    t = torch.arange(28416, device="cuda") / 16000.0
    tone = torch.sin(2 * torch.pi * 150.0 * t) * torch.exp(-1.5 * t)
    pitch.estimate_pitch(sigs + [tone])
    pitch.yin(torch.stack([tone, tone]))
    report("estimate_pitch ragged batch of 10 + a (2, L) batch", fail)
    pitch.estimate_pitch([sigs[1], tone, sigs[6]], fmin=15.625, fmax=8000.0, frame_length=2048, hop_length=301)
    pitch.estimate_pitch([tone, sigs[5]], fmin=15.625, fmax=8000.0, frame_length=1023, hop_length=7)
    pitch.estimate_pitch([tone[:1314 + 8191]], hop_length=1)
    report("estimate_pitch largest LDS image, odd frame length, 8192 frames", fail)
    A.pitch_shift_chain([tone, tone, tone, sigs[6]], [-9.37, 6.63, -3.37, -1.5], signed=True)
    report("pitch_shift_chain signed tree", fail)


def sweep_ingest(fail):
    """The ingest path (csrc/resample_poly.hip): one ragged launch of eight rate pairs (a signal shorter than its filter, outputs over several
    blocks, up = 1, down = 1, the largest filter), fix_length targets on both sides of NRES, a steep decimation whose blocks shrink to fit the
    span, rows that stay out of the launch, and uploads_to_stft on top."""
    import numpy as np
    from diffusynth_amd import ingest as G
    lengths = (1, 2, 160, 441, 442, 1000, 3001, 7777)
    origs = (44100, 48000, 8000, 11025, 22050, 16000, 16000, 8000)
    targets = (16000, 16000, 16000, 16000, 16000, 48000, 44100, 16000)
    sigs = [synth_input("bs_ing%d" % n, (n,)).cuda() for n in lengths]
    G.resample_poly(sigs, list(origs), list(targets))
    G.resample_poly(sigs, list(origs), list(targets), lengths=[5, 1, 200, 1500, 321, 2048, 8272, 20000])
    report("resample_poly ragged batch of 8 rate pairs, with and without fix_length targets", fail)
    G.resample_poly([sigs[7], sigs[6], sigs[5]], [96000, 16000, 44100], [8000, 16000, 16000], lengths=[700, 100, 4000])
    G.resample_poly(torch.stack([sigs[7], sigs[7]]), 44100, 16000, lengths=65280)
    report("resample_poly 12:1 decimation, an equal-rate row, a (2, L) batch", fail)
    ups = [(44100, (synth_input("bs_ing_a", (13230,)).numpy() * 3000).astype(np.int16)), (48000, synth_input("bs_ing_b", (48000,)).double()),
           (16000, synth_input("bs_ing_c", (5000,)))]
    G.uploads_to_stft(ups, 1, time_resolution=48)
    G.uploads_to_stft(ups, 3)
    report("uploads_to_stft 3 uploads at two durations", fail)


def sweep_master(fail):
    """The mastering stage (csrc/master.hip): ragged batches on both sides of a tile at no look-ahead, the defaults and the caps (the largest
    LDS image), with and without the int16 output, a (B, L) batch, and more chunks than the reduction has partials."""
    from diffusynth_amd import arranger as A
    sigs = [3.0 * synth_input("bs_ms%d" % n, (n,)).cuda() for n in (1, 2, 161, 4095, 4096, 4097, 20001)]
    for look, hold in ((0.0, 0.0), (0.005, 0.05), (1024.5 / 16000, 8192.5 / 16000)):
        m = A.Mastering(lookahead=look, hold=hold)
        A.master(sigs, m, return_stats=True)
        A.master(sigs[::-1], m, pcm16=True)
    report("master ragged batch of 7 at three (lookahead, hold) pairs, fp32 and int16", fail)
    A.master(torch.stack([sigs[6], -sigs[6]]), A.Mastering(target_rms=None))
    A.master(synth_input("bs_ms_long", (2 ** 20 + 4099,)).cuda(), pcm16=True)
    report("master (2, L) batch, 2^20 + 4099 samples", fail)


def sweep_loudness(fail):
    """The loudness meter (csrc/loudness.hip): ragged batches on both sides of four hops at three rates (three chunkings of a hop), with and
    without the block energies, a long carry chain, and master() to a LUFS target."""
    import importlib
    from diffusynth_amd import arranger as A
    LM = importlib.import_module("diffusynth_amd.loudness")
    for fs in (16000, 11025, 48000):
        h = LM.hop(fs)
        sigs = [synth_input("bs_lu%d_%d" % (fs, n), (n,)).cuda() for n in (1, 4 * h - 1, 4 * h, 5 * h + 1, 9 * h + 77)]
        LM.loudness(sigs, fs)
        LM.loudness(sigs[::-1], fs, return_blocks=True)
    report("loudness ragged batch of 5 at 16, 11.025 and 48 kHz, with and without the block energies", fail)
    long = synth_input("bs_lu_long", (2 ** 20 + 3001,)).cuda()
    LM.loudness(torch.stack([long, -long]), 16000, return_blocks=True)
    A.master([long, long[:7000], long[:100]], A.Mastering(target_rms=None, target_lufs=-16.0), return_stats=True, return_loudness=True)
    report("loudness (2, L) batch of 2^20 + 3001 samples, master() to a LUFS target", fail)


def sweep_true_peak(fail):
    """The true-peak meter and the limiter that takes its envelope (csrc/true_peak.hip, ds_master_limit_tp): ragged batches on both sides of
    the interpolator's reach and of a tile, with and without the envelope, a (B, L) batch, a long signal, and master() with true_peak=True
    at no look-ahead, the defaults and the caps, with the int16 output and on a long signal.  No LUFS target here: it would add only
    csrc/loudness.hip's kernels, which sweep_loudness covers, and a ds_loudness call behind a ds_loudness_gain call of the same process
    reports that translation unit's older extent table on one XCD ("found, not fixed")."""
    import diffusynth_amd
    from diffusynth_amd import arranger as A
    T = L.TP["DS_TP_TILE"]
    sigs = [3.0 * synth_input("bs_tp%d" % n, (n,)).cuda() for n in (1, 2, 5, 6, 7, 11, 12, 13, T - 1, T, T + 1, 2 * T + 13, 20001)]
    diffusynth_amd.true_peak(sigs)
    diffusynth_amd.true_peak(sigs[::-1], return_envelope=True)
    report("true_peak ragged batch of 13, with and without the envelope", fail)
    long = synth_input("bs_tp_long", (2 ** 20 + 3001,)).cuda()
    diffusynth_amd.true_peak(torch.stack([long, -long]), return_envelope=True)
    report("true_peak (2, L) batch of 2^20 + 3001 samples", fail)
    for look, hold in ((0.0, 0.0), (0.005, 0.05), (1024.5 / 16000, 8192.5 / 16000)):
        m = A.Mastering(lookahead=look, hold=hold, true_peak=True)
        A.master(sigs, m, return_stats=True, return_true_peak=True)
        A.master(sigs[::-1], m, pcm16=True)
    A.master([long, long[:7000], long[:100]], A.Mastering(true_peak=True), return_stats=True, return_true_peak=True)
    report("master(true_peak=True) ragged batch of 13 at three (lookahead, hold) pairs, fp32 and int16, and 2^20 + 3001 samples", fail)


def sweep_linattn_paths(fail):
    """The plain linear-attention files at eight exact cases of tests/linattn_ref.py, through the C ABI (this build compiles attn_out_kernel<float>
    without its row-transposition path, and nothing else here calls ds_vq_attn_* directly): empty segments (N = 10 in 7), ragged N, 7 and 8 heads,
    strided labels, both dtypes; both C of the vq kernels with an empty block (nseg = 16 over five groups, nseg = 8 at N = 33), one block over six
    ragged groups, stats_ws NULL.  The results are compared bit for bit as in tests/test_hip_linattn_paths.py."""
    import linattn_ref as R
    import test_hip_linattn_paths as T
    lin = [dict(bf16=False, B=3, N=10, heads=4, nseg=7), dict(bf16=True, B=1, N=10, heads=1, nseg=7, token=True, pad=8),
           dict(bf16=False, B=3, N=257, heads=7, nseg=2, q_softmax=1, lq=True, pad=8), dict(bf16=True, B=1, N=513, heads=8, nseg=2, q_softmax=1, lq=True, pad=8)]
    for a in lin:
        assert a in R.linattn_args()
        c = R.linattn_case(**a)
        assert ("empty_segment" in R.seg_paths(c.N, c.nseg, c.bf16)) == (c.N == 10)
        ctx, out = T._run_linattn(c)
        assert torch.equal(ctx, c.want_ctx) and torch.equal(out, c.want_out), c.id
    report("linattn paths: empty segments, ragged N, 7 / 8 heads, strided labels (fp32 and bf16)", fail)
    vq = [(80, 3, 600, True, 16, True), (160, 3, 600, False, 16, True), (80, 3, 657, True, 4, True), (160, 1, 33, True, 4, False)]
    for a in vq:
        assert a in R.vq_args()
        Cc, B, N, skip, nseg, st = a
        assert ("empty_block" in R.vq_paths(N, nseg)) == (nseg == 16) and "ragged_tile" in R.vq_paths(N, nseg)
        c, want = R.vq_case(Cc, B, N, skip), R.vq_expect(R.vq_case(Cc, B, N, skip), nseg)
        ctx, wfold, y, ws = T._run_vq(c, nseg, st)
        assert torch.equal(ctx, want.ctx) and torch.equal(wfold, want.wfold) and torch.equal(y, want.y) and (ws is None or torch.equal(ws.double(), want.stats)), a
    report("vq_attn paths: C 80 / 160, an empty block, one block over six ragged groups, stats_ws NULL", fail)


def sweep_attn_paths(fail):
    """The fused attention of both tiers at eight exact cases of tests/attn_ref.py, through the C ABI and compared bit for bit as in
    tests/test_hip_attn_paths.py: bf16 first generation with empty segments (nseg 65 over nine groups), 64-pixel groups with a ragged second
    tile (N = 4129) walked by one block per sample (batch_hint 512), the 384-channel context pass with two heads per block, second-generation
    waves past nseg and without a tile, gen = 0 across its threshold; split precision at C = 96 (fused q + Z) and C = 192 / 384 (q planes),
    form B with out_planes, nseg 65 over nine tiles."""
    import attn_ref as R
    import test_hip_attn_paths as T
    want = [dict(C=96, B=2, N=257, gen=1, nseg=65), dict(C=96, B=1, N=4129, gen=1, nseg=65, hint=512, wide=False), dict(C=384, B=1, N=1057, gen=2, nseg=8, wide=False),
            dict(C=192, B=2, N=33, gen=2, nseg=2), dict(C=96, B=2, N=129, gen=0, nseg="lib", hint=96)]
    cases = R.gpu_cases()
    for w in want:
        k = next(k for k in cases if all(k[n] == v for n, v in w.items()))
        T.test_attn_fused_exact(k)
    report("attn_fused paths: empty segments, T = 2 ragged, one block per sample, C = 384 second generation, waves without a tile, gen 0", fail)
    x3 = R.x3_gpu_cases()
    for w in (dict(C=96, N=1057, flavour="wlo"), dict(C=192, N=257, nseg=65), dict(C=384, N=33)):
        k = next(k for k in x3 if all(k[n] == v for n, v in w.items()))
        T.test_attn_x3_exact(k)
    report("attn_x3 paths: fused q + Z, q planes, form B with out_planes, nseg above the tile count", fail)


def _partials(stored, parts):
    """(sum, sumsq) of ``parts`` chunks of each sample of a device tensor as fp32 [B][parts][2], placed 24 bytes into a NaN-filled allocation:
    the base is 8-byte but not 16-byte aligned and anything read beyond the buffer is NaN (tests/gn_partials_ref.py:guarded)."""
    xd = stored.double().flatten(1)
    p = torch.stack([torch.stack([c.sum(1), (c * c).sum(1)], 1) for c in torch.tensor_split(xd, parts, dim=1)], 1).float()
    buf = torch.full((6 + p.numel() + 58,), float("nan"), device="cuda")
    view = buf[6:6 + p.numel()].view(p.shape)
    view.copy_(p)
    return view


def _set_part(p, part, count):
    p.gn_ab, p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = None, part.data_ptr(), part.shape[1], float(count), 1e-5


def _conv(x, wpk, out, out_C, B, C0, H, W, cout, cout_pad, k, tile, dt, wk_order, part=None, count=0, ks=1, **kw):
    """One ds_conv_igemm launch (stride 1, same size; + ds_conv_splitk_reduce for K slices) with statistics; returns its partials."""
    p = L.ConvParams(src0=x.data_ptr(), src1=None, C0=C0, C1=0, H=H, W=W, H1=0, W1=0, off_h1=0, off_w1=0, wpk=wpk.data_ptr(), Cout=cout,
                     cout_pad=cout_pad, KH=k, KW=k, stride=1, pad_h=k // 2, pad_w=k // 2, Ho=H, Wo=W, transposed=0, out=out.data_ptr(), out_C=out_C,
                     out_c0=0, out_nchw_f32=0, bias=None, gn_ab=None, fold_t1=None, fold_t2=None, ncls=9 if k == 3 else 1, act=L.ACT_NONE, res=None,
                     stats_part=None, B=B, dtype=dt, tile=tile, wk_order=wk_order)
    for key, v in kw.items():
        setattr(p, key, v)
    if part is not None:
        _set_part(p, part, count)
    slab = None
    if ks > 1:
        slab = torch.full((ks * B * H * W * ((cout + 7) // 8 * 8),), float("nan"), device="cuda")
        p.ksplit, p.slab = ks, slab.data_ptr()
    st = torch.zeros(B, L.load().ds_conv_stats_parts(C.byref(p)), 2, device="cuda")
    p.stats_part = st.data_ptr()
    L.call("ds_conv_igemm", C.byref(p), L.current_stream())
    if ks > 1:
        L.call("ds_conv_splitk_reduce", C.byref(p), L.current_stream())
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(st).all()
    return st


def sweep_gn_partials(fail):
    """GroupNorm from raw partials, the shapes of tests/test_hip_gn_partials.py: every kernel that reduces gn_part with 1 .. 300 partials
    (the halo kernel also 64 / 65 / 256 / 257: both sides of its 4 x 64 prefetch) behind an 8-byte-aligned base, every depthwise family and
    tile instantiation as a producer, and the producer -> consumer chains without ds_gn_finalize."""
    from diffusynth_amd.engine import split3_weight, to_split_planes
    from hip_helpers import PackedConv, to_nhwc
    lib = L.load()
    st = L.current_stream()
    bf, f32 = L.DS_BF16, L.DS_F32
    tdt = {bf: torch.bfloat16, f32: torch.float32}
    PARTS, PARTS_HALO = (1, 65, 300), (1, 64, 65, 256, 257, 300)
    vec = lambda tag, n, s=1.0: (1.0 if s == 0 else 0.0) + synth_input(tag, (n,), s or 0.2).cuda()

    # ---- ds_gn_apply: fast form (every channel count, HW below `rows` / ragged / several blocks, the grid cap at B = 64), generic lazy form
    def gn_apply(dt, B, Cc, HW, res, cbias=False, act=L.ACT_NONE):
        x = to_nhwc(synth_input("bs_gp_x", (B, Cc, HW, 1)) * 1.5 + 0.7, dt)
        r = to_nhwc(synth_input("bs_gp_r", (B, Cc, HW, 1)), dt) if res else None
        cb = synth_input("bs_gp_cb", (B, Cc)).cuda() if cbias else None
        g, be = vec("bs_gp_g", Cc, 0), vec("bs_gp_be", Cc, 0.3)
        for parts in PARTS:
            part = _partials(x, parts)
            out = torch.full_like(x, float("nan"))
            p = L.GnApplyParams(x=x.data_ptr(), res=L.ptr(r), out=out.data_ptr(), gn_ab=None, gamma=g.data_ptr(), beta=be.data_ptr(), cbias=L.ptr(cb),
                                cb_stride=Cc, B=B, HW=HW, C=Cc, G=1, act=act, dtype=dt)
            p.gn_part, p.gn_parts, p.gn_count, p.gn_eps = part.data_ptr(), parts, float(Cc * HW), 1e-5
            L.call("ds_gn_apply", C.byref(p), st)
            torch.cuda.synchronize()
            assert torch.isfinite(out.float()).all()

    for Cc in (64, 96, 192, 384, 768):
        for HW in (5, 67, 600):
            for res in (False, True):
                gn_apply(bf, 3, Cc, HW, res)
    gn_apply(bf, 64, 768, 520, True)
    report("gn_apply from partials, fast form 31 shapes x 3 partial counts", fail)
    gn_apply(f32, 3, 96, 70, True)
    gn_apply(bf, 3, 160, 70, False, cbias=True)
    gn_apply(bf, 3, 96, 70, False, act=L.ACT_SILU)
    report("gn_apply from partials, generic lazy form 3 shapes x 3 partial counts", fail)

    # ---- generic igemm tiles: 3x3 fold (GELU + residual + statistics), 1x1 fold on two tiles, both dtypes
    def folded(tag, cout, cin, k, dt, tile):
        w = synth_input("bs_gp_w%s" % tag, (cout, cin, k, k), 0.05)
        return PackedConv(w, synth_input("bs_gp_b%d" % cout, (cout,)), dt, tile, gamma=1 + 0.2 * synth_input("bs_gp_g%d" % cin, (cin,)),
                          beta=0.3 * synth_input("bs_gp_be%d" % cin, (cin,)))

    def fold_kw(pc):
        return dict(bias=L.ptr(pc.bias), fold_t1=pc.t1.data_ptr(), fold_t2=pc.t2.data_ptr())

    for dt in (f32, bf):
        for cout, k, (H, W), tiles in ((192, 3, (9, 7), (L.TILE_128x192,)), (384, 1, (8, 16), (L.TILE_128x192, L.TILE_256x96))):
            x = to_nhwc(synth_input("bs_gp_ix%d" % k, (3, 96, H, W)) * 2 + 0.7, dt)
            r = to_nhwc(synth_input("bs_gp_ir%d" % k, (3, cout, H, W)), dt)
            for tile in tiles:
                pc = folded("i%d" % k, cout, 96, k, dt, tile)
                for parts in PARTS:
                    out = torch.full((3, H, W, cout), float("nan"), device="cuda").to(tdt[dt])
                    _conv(x, pc.w, out, cout, 3, 96, H, W, cout, pc.cout_pad, k, tile, dt, 0, _partials(x, parts), 96 * H * W,
                          act=L.ACT_GELU if k == 3 else L.ACT_NONE, res=r.data_ptr() if k == 3 else None, **fold_kw(pc))
        report(f"conv_igemm from partials dtype {dt}", fail)

    # ---- halo kernel, bf16: the three patch widths, GELU + residual + statistics, whole K and K slices
    HT = L.TILE_HALO3_256x96
    for (B, cin, H, W), cout in (((3, 96, 8, 64), 192), ((3, 32, 33, 8), 96), ((3, 64, 7, 3), 96)):
        x = to_nhwc(synth_input("bs_gp_hx%d" % cin, (B, cin, H, W)) * 1.5 + 0.4, bf)
        r = to_nhwc(synth_input("bs_gp_hr%d" % cin, (B, cout, H, W)), bf)
        pc = folded("h%d" % cin, cout, cin, 3, bf, HT)
        for ks in (1, 2, 3):
            if (cin // 32) % ks:
                continue
            for parts in PARTS_HALO:
                out = torch.full((B, H, W, cout), float("nan"), device="cuda").bfloat16()
                _conv(x, pc.w, out, cout, B, cin, H, W, cout, pc.cout_pad, 3, HT, bf, 1, _partials(x, parts), cin * H * W, ks, act=L.ACT_GELU,
                      res=r.data_ptr(), **fold_kw(pc))
    report("conv3x3_halo3 bf16 from partials, 3 shapes x K slices x 6 partial counts", fail)

    # ---- halo kernel, split precision (hi / lo planes in; planes out + GELU, or fp32 out + residual), two samples per block incl. an odd batch
    class X3:
        def __init__(self, tag, cout, cin):
            w = synth_input("bs_gp_xw%s" % tag, (cout, cin, 3, 3), 0.05)
            g, be = 1 + 0.2 * synth_input("bs_gp_xg%d" % cin, (cin,)), 0.3 * synth_input("bs_gp_xbe%d" % cin, (cin,))
            self.cout, self.cin = cout, cin
            self.pc = PackedConv(split3_weight(w, g), synth_input("bs_gp_xb%d" % cout, (cout,)), bf, HT)
            self.t1, self.t2 = torch.empty(9 * cout, device="cuda"), torch.empty(9 * cout, device="cuda")
            wd, gd, bd = w.cuda().contiguous(), g.cuda(), be.cuda()
            L.call("ds_conv_fold_tables", wd.data_ptr(), self.pc.bias.data_ptr(), gd.data_ptr(), bd.data_ptr(), cout, cin, 3, 3, self.t1.data_ptr(),
                   self.t2.data_ptr(), st)
            torch.cuda.synchronize()

        def run(self, planes, B, H, W, split_out, part, ks=1, res=None):
            cout = self.cout
            out = torch.full((B, H, W, 2 * cout), float("nan"), device="cuda").bfloat16() if split_out else torch.full((B, H, W, cout), float("nan"), device="cuda")
            sp = _conv(planes, self.pc.w, out, 2 * cout if split_out else cout, B, 2 * self.cin, H, W, cout, self.pc.cout_pad, 3, HT, bf, 1, part,
                       self.cin * H * W, ks, bias=self.pc.bias.data_ptr(), fold_t1=self.t1.data_ptr(), fold_t2=self.t2.data_ptr(),
                       act=L.ACT_GELU if split_out else L.ACT_NONE, res=L.ptr(res), flags=1 | (2 if split_out else 4))
            return out, sp

    def planes_sum(pl):
        c = pl.shape[-1] // 2
        return pl[..., :c].float() + pl[..., c:].float()

    for (B, cin, H, W), cout in (((3, 96, 8, 64), 192), ((3, 96, 16, 8), 192), ((5, 32, 16, 5), 96), ((2, 64, 12, 7), 96)):
        cv = X3("%d_%d" % (cout, cin), cout, cin)
        xs = to_split_planes((synth_input("bs_gp_sx%d" % cin, (B, H, W, cin)) * 1.5 + 0.4)).cuda()
        r = synth_input("bs_gp_sr%d" % cin, (B, H, W, cout)).cuda()
        for ks in (1, 2, 3):
            if (cin // 32) % ks:
                continue
            for parts in PARTS_HALO:
                part = _partials(planes_sum(xs), parts)
                cv.run(xs, B, H, W, True, part, ks)
                cv.run(xs, B, H, W, False, part, ks, res=r)
    report("conv3x3_halo3 split precision from partials, 4 shapes x 2 output modes x K slices x 6 partial counts", fail)

    # ---- halo kernel with the fused 1x1 res_conv over two sources
    B, cin, H, W, cout, c0, c1 = 2, 96, 9, 27, 96, 96, 96
    pc = folded("rc", cout, cin, 3, bf, HT)
    rpk = torch.empty(lib.ds_pack_conv_elems(c0 + c1, 1, 1, pc.cout_pad, 0), dtype=torch.bfloat16, device="cuda")
    wr = synth_input("bs_gp_wr", (cout, c0 + c1, 1, 1), 0.1).cuda().contiguous()
    pp = L.PackConvParams(w=wr.data_ptr(), gamma=None, dst=rpk.data_ptr(), dtype=bf, Cout=cout, Cin=c0 + c1, cin_pad=c0 + c1, KH=1, KW=1,
                          cout_pad=pc.cout_pad, transposed=0, k_order=1)
    L.call("ds_pack_conv_weight", C.byref(pp), st)
    wall, br = torch.cat([rpk, pc.w]), synth_input("bs_gp_br", (cout,)).cuda()
    x = to_nhwc(synth_input("bs_gp_rcx", (B, cin, H, W)) * 1.5 + 0.4, bf)
    x0, x1 = to_nhwc(synth_input("bs_gp_rc0", (B, c0, H, W)), bf), to_nhwc(synth_input("bs_gp_rc1", (B, c1, H - 2, W - 1)), bf)
    for parts in PARTS_HALO:
        out = torch.full((B, H, W, cout), float("nan"), device="cuda").bfloat16()
        _conv(x, wall, out, cout, B, cin, H, W, cout, pc.cout_pad, 3, HT, bf, 1, _partials(x, parts), cin * H * W, res_src0=x0.data_ptr(),
              res_src1=x1.data_ptr(), res_C0=c0, res_C1=c1, res_H1=H - 2, res_W1=W - 1, res_off_h1=1, res_off_w1=0, res_steps=(c0 + c1) // 32,
              res_bias=br.data_ptr(), **fold_kw(pc))
    report("conv3x3_halo3 + fused res_conv from partials", fail)

    # ---- fused attention, both generations, and its split-precision form; then the tail without ds_gn_finalize (partials of y -> gn_apply)
    def attention(Cc, H, W, cond, x3):
        B, N = 3, H * W
        dt = f32 if x3 else bf
        x = to_nhwc(synth_input("bs_gp_ax%d" % Cc, (B, Cc, H, W)) * 1.3 + 0.6, dt)
        wq, wo = synth_input("bs_gp_awq%d" % Cc, (384, Cc), Cc ** -0.5).cuda(), synth_input("bs_gp_awo%d" % Cc, (Cc, 128), 0.09).cuda()
        g, be, bo = vec("bs_gp_ag", Cc, 0), vec("bs_gp_abe", Cc, 0.3), vec("bs_gp_abo", Cc, 0.3)
        go, bo2 = vec("bs_gp_ago", Cc, 0), vec("bs_gp_abo2", Cc, 0.3)
        lq = synth_input("bs_gp_alq", (B, 128)).cuda() if cond else None
        t1, t2 = torch.empty(384, device="cuda"), torch.empty(384, device="cuda")
        L.call("ds_conv_fold_tables", wq.data_ptr(), None, g.data_ptr(), be.data_ptr(), 384, Cc, 1, 1, t1.data_ptr(), t2.data_ptr(), st)
        ctx = torch.empty(B * 4 * 1024, device="cuda")
        for parts in PARTS:
            part = _partials(x, parts)
            y = torch.full((B, H, W, Cc), float("nan"), device="cuda").to(tdt[dt])
            if x3:
                whl = torch.empty(2 * 384 * Cc, dtype=torch.bfloat16, device="cuda")
                L.call("ds_pack_attn_x3", wq.data_ptr(), g.data_ptr(), whl.data_ptr(), Cc, st)
                runs = []
                for nseg in sorted({3, lib.ds_attn_x3_segments(B, N, Cc)}):
                    scratch = (torch.empty(lib.ds_linattn_part_floats(B, 4, nseg), device="cuda"),
                               torch.empty(lib.ds_attn_x3_qplane_bytes(B, N), dtype=torch.uint8, device="cuda"),
                               torch.empty(lib.ds_attn_x3_mfold_bytes(B, Cc), dtype=torch.uint8, device="cuda"))
                    p = L.AttnX3Params(x=x.data_ptr(), B=B, N=N, C=Cc, nseg=nseg, wqkv_hl=whl.data_ptr(), t1=t1.data_ptr(), t2=t2.data_ptr(), gn_ab=None,
                                       label_q=L.ptr(lq), lq_stride=128, scale=32 ** -0.5, part=scratch[0].data_ptr(), ctx=ctx.data_ptr(),
                                       qplanes=scratch[1].data_ptr(), mfold=scratch[2].data_ptr(), wout=wo.data_ptr(), bias_out=bo.data_ptr(),
                                       y=y.data_ptr(), stats_part=None)
                    runs.append((p, "ds_attn_x3", lib.ds_attn_x3_stats_parts, scratch))
            else:
                wq16, wo16 = torch.empty(384 * Cc, dtype=torch.bfloat16, device="cuda"), torch.empty(Cc * 128, dtype=torch.bfloat16, device="cuda")
                L.call("ds_pack_attn_fused", wq.data_ptr(), g.data_ptr(), wo.data_ptr(), wq16.data_ptr(), wo16.data_ptr(), Cc, st)
                runs = []
                for gen in (1, 2):
                    scratch = (torch.empty(lib.ds_linattn_part_floats(B, 4, 3), device="cuda"),
                               torch.empty(B * Cc * 128, dtype=torch.bfloat16, device="cuda") if gen == 2 else None)
                    p = L.AttnFusedParams(x=x.data_ptr(), B=B, N=N, C=Cc, nseg=3, wqkv=wq16.data_ptr(), t1=t1.data_ptr(), t2=t2.data_ptr(), gn_ab=None,
                                          label_q=L.ptr(lq), lq_stride=128, scale=32 ** -0.5, part=scratch[0].data_ptr(), ctx=ctx.data_ptr(),
                                          wout_perm=wo16.data_ptr(), bias_out=bo.data_ptr(), y=y.data_ptr(), stats_part=None)
                    p.mfold, p.gen = L.ptr(scratch[1]), gen
                    runs.append((p, "ds_attn_fused", lib.ds_attn_fused_stats_parts, scratch))
            for p, name, nparts, _scratch in runs:
                _set_part(p, part, Cc * N)
                sp = torch.zeros(B, nparts(C.byref(p)), 2, device="cuda")
                p.stats_part = sp.data_ptr()
                L.call(name + "_context", C.byref(p), st)
                L.call(name + "_output", C.byref(p), st)
                out = torch.full_like(y, float("nan"))
                gp = L.GnApplyParams(x=y.data_ptr(), res=x.data_ptr(), out=out.data_ptr(), gn_ab=None, gamma=go.data_ptr(), beta=bo2.data_ptr(),
                                     cbias=None, cb_stride=0, B=B, HW=N, C=Cc, G=1, act=L.ACT_NONE, dtype=dt)
                gp.gn_part, gp.gn_parts, gp.gn_count, gp.gn_eps = sp.data_ptr(), sp.shape[1], float(Cc * N), 1e-5
                L.call("ds_gn_apply", C.byref(gp), st)
                torch.cuda.synchronize()
                assert torch.isfinite(y.float()).all() and torch.isfinite(out.float()).all()

    for x3 in (False, True):
        for Cc, (H, W), cond in ((96, (5, 10), False), (192, (33, 32), True), (384, (8, 6), True)):
            attention(Cc, H, W, cond, x3)
        report("attn_%s from partials + gn_apply from the partials of y, 3 shapes x 3 partial counts" % ("x3" if x3 else "fused gen 1 / 2"), fail)

    # ---- depthwise 7x7: every family and tile instantiation (two sources with pad offsets, time bias, B = 3)
    def dwconv(dt, c0, c1, H, W, wexp=False, out_split=0, strip=0):
        B, Cc = 3, c0 + c1
        x0 = to_nhwc(synth_input("bs_gp_d0", (B, c0, H, W)) * 1.5 + 0.5, dt)
        x1 = to_nhwc(synth_input("bs_gp_d1", (B, c1, H - 1, W - 3)), dt) if c1 else None
        w = synth_input("bs_gp_dw%d" % Cc, (Cc, 1, 7, 7), 0.2).cuda().contiguous()
        wt = torch.empty(49 * Cc, device="cuda")
        L.call("ds_pack_dw_weight", w.data_ptr(), Cc, wt.data_ptr(), st)
        we = None
        if wexp:
            we = torch.empty(Cc * 6 * 64 * 8, dtype=torch.bfloat16, device="cuda")
            L.call("ds_pack_dw_weight_mfma", w.data_ptr(), Cc, we.data_ptr(), st)
        b, tb = synth_input("bs_gp_db", (Cc,)).cuda(), synth_input("bs_gp_dtb", (B, Cc + 12)).cuda()
        out = torch.full((B, H, W, 2 * Cc), float("nan"), device="cuda").bfloat16() if out_split else torch.full((B, H, W, Cc), float("nan"), device="cuda").to(tdt[dt])
        p = L.DwconvParams(src0=x0.data_ptr(), src1=L.ptr(x1), C0=c0, C1=c1, H=H, W=W, H1=(H - 1 if c1 else 0), W1=(W - 3 if c1 else 0), off_h1=0,
                           off_w1=1, wt=wt.data_ptr(), bias=b.data_ptr(), tbias=tb.data_ptr() + 4 * 5, tb_stride=Cc + 12, out=out.data_ptr(),
                           stats_part=None, B=B, dtype=dt, wexp=L.ptr(we), out_split=out_split, strip=strip)
        sp = torch.zeros(B, lib.ds_dwconv_stats_parts(C.byref(p)), 2, device="cuda")
        p.stats_part = sp.data_ptr()
        L.call("ds_dwconv7", C.byref(p), st)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all() and torch.isfinite(sp).all()
        return out, sp

    dwconv(bf, 40, 0, 10, 9)
    dwconv(f32, 20, 0, 10, 9)
    for W in (7, 12, 40):
        dwconv(bf, 32, 64, 19, W)
        dwconv(f32, 48, 0, 19, W)
        dwconv(f32, 16, 32, 19, W)
    for H, W in ((16, 8), (19, 24)):
        for split in (0, 1):
            dwconv(f32, 96, 0, H, W, out_split=split)
    dwconv(f32, 96, 0, 64, 16, out_split=1, strip=1)
    dwconv(f32, 32, 64, 70, 37, out_split=1, strip=1)
    dwconv(bf, 96, 192, 40, 16, wexp=True)
    dwconv(bf, 96, 192, 37, 70, wexp=True)
    report("dwconv7 family matrix: direct, 8 / 16 / 32-wide tiles (bf16, fp32 NV = 4 / 8), strip, matrix cores", fail)

    # ---- ConvNeXt chains without ds_gn_finalize: depthwise -> 3x3 (GELU, statistics) -> 3x3 + residual, partials handed on raw
    c1x, c2x = X3("ch1", 192, 96), X3("ch2", 96, 192)
    for (H, W), strip in (((16, 8), 0), ((19, 24), 0), ((64, 16), 1)):
        pl0, sp0 = dwconv(f32, 96, 0, H, W, out_split=1, strip=strip)
        pl1, sp1 = c1x.run(pl0, 3, H, W, True, sp0)
        c1x.run(pl0, 3, H, W, True, sp0, ks=3)
        c2x.run(pl1, 3, H, W, False, sp1, res=synth_input("bs_gp_chr", (3, H, W, 96)).cuda())
    H, W = 37, 70
    y0, sp0 = dwconv(bf, 96, 0, H, W, wexp=True)
    p1, p2 = folded("cb1", 192, 96, 3, bf, HT), folded("cb2", 96, 192, 3, bf, HT)
    y1 = torch.full((3, H, W, 192), float("nan"), device="cuda").bfloat16()
    sp1 = _conv(y0, p1.w, y1, 192, 3, 96, H, W, 192, p1.cout_pad, 3, HT, bf, 1, sp0, 96 * H * W, act=L.ACT_GELU, **fold_kw(p1))
    y2 = torch.full((3, H, W, 96), float("nan"), device="cuda").bfloat16()
    r = to_nhwc(synth_input("bs_gp_chrb", (3, 96, H, W)), bf)
    _conv(y1, p2.w, y2, 96, 3, 192, H, W, 96, p2.cout_pad, 3, HT, bf, 1, sp1, 192 * H * W, res=r.data_ptr(), **fold_kw(p2))
    report("chains dwconv -> conv3x3 -> conv3x3 on raw partials (split precision: tile, two samples per block, strip; bf16: matrix cores)", fail)


def main():
    lib = L.load()
    assert "bounds" in L.lib_path(), L.lib_path()
    fail = []
    if "--only-gn-partials" in sys.argv:
        sweep_gn_partials(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-ui-images" in sys.argv:
        sweep_ui_images(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-pitch" in sys.argv:
        sweep_pitch(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-ingest" in sys.argv:
        sweep_ingest(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-master" in sys.argv:
        sweep_master(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-loudness" in sys.argv:
        sweep_loudness(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-true-peak" in sys.argv:
        sweep_true_peak(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-perform" in sys.argv:
        sweep_perform(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-linattn-paths" in sys.argv:
        sweep_linattn_paths(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-attn-paths" in sys.argv:
        sweep_attn_paths(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    if "--only-arranger" in sys.argv:
        sweep_arranger(fail)
        print("BOUNDS VIOLATIONS %s" % fail if fail else "BOUNDS OK")
        sys.exit(1 if fail else 0)
    # 0) the tool detects a violation (negative control) and resets
    b = torch.zeros(16, device="cuda")
    sink = torch.zeros(1, device="cuda")
    lib.ds_bounds_selftest.restype = C.c_int
    lib.ds_bounds_selftest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.ds_bounds_selftest(b.data_ptr(), sink.data_ptr(), L.current_stream()) == 0
    buf = C.create_string_buffer(4096)
    n = lib.ds_bounds_report(buf, 4096, 1)
    print("[bounds] self-test:", n, buf.value.decode(), flush=True)
    assert n == 1 and b"offset 56 outside extent 64" in buf.value, "the bounds build did not catch its own negative control"
    assert lib.ds_bounds_report(buf, 4096, 1) == 0

    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        keys = json.load(f)
    from diffusynth_amd.unet import PRODUCTION_CONFIG, ConditionedUnet
    from diffusynth_amd.vqgan import PRODUCTION_CONFIG as VQ_CFG, VQGAN
    # 1) VQGAN encoder / decoder, the shapes of tests/test_hip_tail.py (enc2 = (1,3,512,12) is where r01 aborted)
    vae = VQGAN(**VQ_CFG)
    vae.load_state_dict(synth_state_dict([(k, tuple(s)) for k, s in keys["vqgan_production"]]))
    vae.to("cuda")
    for dt in ("fp32", "bf16"):
        vae._encoder.set_compute_dtype(dt)
        vae._decoder.set_compute_dtype(dt)
        for shape in ((1, 3, 512, 12), (2, 3, 512, 48), (1, 3, 512, 20)):
            z = vae._encoder(synth_input("bs_enc%d" % shape[3], shape).cuda())
            assert torch.isfinite(z).all()
        for shape in ((2, 4, 128, 3), (1, 4, 128, 5), (3, 4, 128, 16)):
            y = vae._decoder(synth_input("bs_dec%d" % shape[3], shape).cuda())
            assert torch.isfinite(y).all()
        report(f"vqgan encoder+decoder {dt}", fail)
    # 2) production U-Net, both tiers: ragged / odd widths, batch sizes on both sides of every split-K threshold
    net = ConditionedUnet(**PRODUCTION_CONFIG)
    net.load_state_dict(synth_state_dict([(k, tuple(s)) for k, s in keys["unet_production"]]))
    net.to("cuda")
    for dt, shapes in (("fp32", ((1, 128, 64), (1, 128, 27), (3, 32, 64), (2, 32, 48))),
                       # (the headline tier: split-precision 3x3 incl. its split-K slices, conv1x1_x3, attn_x3 — ragged tiles, one and many segments)
                       ("bf16x3", ((1, 128, 64), (1, 128, 27), (3, 32, 64), (2, 32, 48), (1, 128, 100), (16, 256, 64), (1, 256, 64))),
                       ("bf16", ((1, 128, 64), (1, 128, 27), (1, 128, 20), (1, 128, 100), (2, 128, 144), (3, 32, 64), (2, 32, 48),
                                 (16, 256, 64), (5, 256, 64), (32, 128, 64), (1, 256, 64), (1, 128, 256)))):
        net.set_compute_dtype(dt)
        for B, H, W in shapes:
            for cond in (True, False):
                y = net(synth_input("bs_x", (B, 4, H, W)).cuda(), torch.arange(B).cuda() * 37 % 1000,
                        synth_input("bs_c", (B, 512)).cuda() if cond else None)
                if not torch.isfinite(y).all():              # a suppressed store shows up as garbage downstream: say which access first
                    report(f"unet {dt} {(B, H, W)} NON-FINITE OUTPUT", fail)
                    raise AssertionError((dt, B, H, W))
        report(f"unet {dt} {len(shapes)} shapes", fail)
    # 3) kernel-level: narrow BN tiles and split-K through the C entry, weights packed for exactly the tile
    from hip_helpers import PackedConv, run_conv, to_nhwc
    for dt in (L.DS_F32, L.DS_BF16):
        for tile, cout, cin, k, hw, ks in ((L.TILE_128x32, 4, 96, 3, (16, 8), 1), (L.TILE_128x32, 3, 8, 7, (32, 12), 1),
                                           (L.TILE_64x192, 192, 192, 1, (8, 8), 1), (L.TILE_64x192, 384, 384, 4, (16, 8), 4),
                                           (L.TILE_256x96, 80, 80, 3, (24, 6), 1), (L.TILE_128x192, 160, 80, 4, (32, 6), 2)):
            if ks > 1 and dt != L.DS_BF16:
                continue
            w = synth_input(f"bs_w{cout}_{cin}_{k}", (cout, cin, k, k), 0.05)
            pc = PackedConv(w, synth_input("bs_b%d" % cout, (cout,)), dt, tile)
            x = to_nhwc(synth_input(f"bs_cx{cin}", (2, cin) + hw), dt)
            stride, pad = (2, 1) if k == 4 else (1, k // 2)
            run_conv(pc, x, stride=stride, pad=pad, ksplit=ks, want_stats=True)
        report(f"conv_igemm narrow tiles / split-K dtype {dt}", fail)
    # empty split-K slices are rejected at the boundary now (nq = 9, ksplit = 4: the last slice would start past the weights)
    pc = PackedConv(synth_input("bs_w9", (96, 32, 3, 3), 0.05), None, L.DS_BF16, L.TILE_256x96)
    try:
        run_conv(pc, to_nhwc(synth_input("bs_x9", (1, 32, 16, 16)), L.DS_BF16), pad=1, ksplit=4)
        fail.append(("empty slice accepted", 0, ""))
    except L.DsError as e:
        print("[bounds] empty split-K slice rejected:", str(e)[-90:], flush=True)
    report("after rejected launch", fail)
    # 4) the UI images
    sweep_ui_images(fail)
    # 5) the arranger's audio stage
    sweep_arranger(fail)
    sweep_perform(fail)
    sweep_pitch(fail)
    sweep_ingest(fail)
    sweep_master(fail)
    sweep_loudness(fail)
    sweep_true_peak(fail)
    # 6) GroupNorm from raw partials in every kernel that reduces them, the depthwise families, the chains without ds_gn_finalize
    sweep_gn_partials(fail)
    # 7) the plain linear-attention files on the paths of tests/test_hip_linattn_paths.py
    sweep_linattn_paths(fail)
    sweep_attn_paths(fail)
    if fail:
        print("BOUNDS VIOLATIONS", fail)
        sys.exit(1)
    print("BOUNDS OK")


if __name__ == "__main__":
    main()
