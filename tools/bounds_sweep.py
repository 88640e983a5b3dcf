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
    normed = A.peak_normalize(sigs)
    report("peak_normalize 8 signals (1 .. 77568 samples)", fail)
    n = 100000
    A.mix_notes(normed, [(0, 0), (n - 77568, 1), (1023, 7), (n - 1, 7), (0, 7), (500, 3), (500, 3), (n - 1023, 4), (60000, 2)], n)
    A.mix_notes(normed[7:], [(3, 0)], 5)
    report("mix_notes 9 events over 98 blocks + a 5-sample track", fail)


def main():
    lib = L.load()
    assert "bounds" in L.lib_path(), L.lib_path()
    fail = []
    if "--only-ui-images" in sys.argv:
        sweep_ui_images(fail)
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
    if fail:
        print("BOUNDS VIOLATIONS", fail)
        sys.exit(1)
    print("BOUNDS OK")


if __name__ == "__main__":
    main()
