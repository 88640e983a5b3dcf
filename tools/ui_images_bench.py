#!/usr/bin/env python3
"""What the UI images add to the latent -> audio tail, fp32 decoder tier, (B, 4, 128, 64) latents -> (B, 3, 512, 256) STFT+ (one MI355X).

    python tools/ui_images_bench.py [--root OTHER_TREE] [--what base,images,host] [--batches 8,64] [--out FILE.json]

  base    latents_to_audio(decoder, q): synchronised wall-clock median.  --root runs it from another checkout (the parent commit built
          in a second directory), so the job script can interleave the two trees on one box like tools/ab.sh does for two libraries
  images  ui_images.stft_images on the decoder output (device time, synchronised), the two device -> host copies of the byte images,
          and the whole encodeBatch2GradioOutput_STFT
  host    the reference's way: the fp32 decoder output to the host + the numpy chain per clip (tests/ui_images_ref.py) on 16 threads
Prints one JSON line; the byte model is 2.9 MB per 512 x 256 clip."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median_ms(fn, iters, sync):
    ts = []
    for _ in range(iters):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--what", default="base,images,host")
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    from diffusynth_amd.synth import synth_input, synth_state_dict
    from diffusynth_amd.vocoder import latents_to_audio
    from diffusynth_amd.vqgan import PRODUCTION_CONFIG, VQGAN
    what = set(a.what.split(","))
    with open(os.path.join(root, "tests", "golden", "state_dict_keys.json")) as f:
        keys = [(k, tuple(s)) for k, s in json.load(f)["vqgan_production"]]
    vae = VQGAN(**PRODUCTION_CONFIG)
    vae.load_state_dict(synth_state_dict(keys))
    vae = vae.cuda()
    vae._decoder.set_compute_dtype("fp32")
    sync = torch.cuda.synchronize
    res = {"root": os.path.relpath(root, HERE), "device": torch.cuda.get_device_name(0), "iters": a.iters, "batches": {}}
    for B in (int(b) for b in a.batches.split(",")):
        q = vae._vq_vae(synth_input("ui_bench_z", (B, 4, 128, 64)).cuda())[0]
        r = {}
        for _ in range(2):                                             # warm-up: plans, workspaces
            latents_to_audio(vae._decoder, q)
        if "base" in what:
            r["latents_to_audio_ms"] = median_ms(lambda: latents_to_audio(vae._decoder, q), a.iters, sync)
        if "images" in what or "host" in what:
            rec = vae._decoder(q)
        if "images" in what:
            from diffusynth_amd.ui_images import stft_images
            from diffusynth_amd.vocoder import encodeBatch2GradioOutput_STFT
            spec, phase = stft_images(rec)
            r["stft_images_device_ms"] = median_ms(lambda: stft_images(rec), a.iters, sync)
            r["two_image_copies_d2h_ms"] = median_ms(lambda: (spec.cpu(), phase.cpu()), a.iters, sync)
            encodeBatch2GradioOutput_STFT(vae._decoder, q)
            r["encodeBatch2GradioOutput_STFT_ms"] = median_ms(lambda: encodeBatch2GradioOutput_STFT(vae._decoder, q), a.iters, sync)
            r["byte_model_us"] = B * 2.9e6 / 4.4e12 * 1e6
            if "latents_to_audio_ms" in r:
                r["images_share_of_latents_to_audio"] = r["stft_images_device_ms"] / r["latents_to_audio_ms"]
        if "host" in what:
            from concurrent.futures import ThreadPoolExecutor
            sys.path.insert(0, os.path.join(root, "tests"))
            import ui_images_ref as R
            torch.set_num_threads(16)

            def host_way():
                x = rec.cpu().numpy()
                with ThreadPoolExecutor(16) as ex:
                    return list(ex.map(R.stft_images_ref, x))
            r["host_numpy_chain_16_threads_ms"] = median_ms(host_way, 3, sync)
            t0 = time.perf_counter()
            R.stft_images_ref(rec[0].cpu().numpy())
            r["host_numpy_chain_one_clip_ms"] = (time.perf_counter() - t0) * 1e3
        res["batches"][str(B)] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
