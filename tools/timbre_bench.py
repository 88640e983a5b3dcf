#!/usr/bin/env python3
"""What scoring a batch of sampled sounds costs: multi_modal_model.get_timbre_features on (B, 4, 128, W) latents, production encoder
(3 LSTM layers of 1024 units) and two projection layers, fp32, one MI355X.

    python tools/timbre_bench.py [--shapes 8x64,16x144,64x64] [--iters 9] [--what device,step,host] [--out FILE.json]

  device  get_timbre_features, device events around `iters` calls after warm-up: median per call
  step    ds_lstm_layer alone on one layer's pre (T launches): time per step and the w_hh bytes a step reads over it.  Every step re-reads
          the whole w_hh (3 T |W_hh| bytes per call, 16 MiB each at H = 1024), from L2 once the first step has brought it in
  host    the reference-equivalent torch CPU module (nn.Linear + nn.LSTM + the projection head of tests/timbre_ref.py) on 16 threads,
          on the host this runs on: the only way the reference has (app.py:59 moves the model to the CPU)
Prints one JSON line.  Needs a GPU: no figure is produced without one."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def event_ms(fn, iters, torch):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x64,16x144,64x64")
    ap.add_argument("--what", default="device,step,host")
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import timbre_ref as R
    from diffusynth_amd import _lib as L
    from diffusynth_amd.synth import synth_input, synth_state_dict
    from diffusynth_amd.timbre import TimbreEncoder, multi_modal_model
    assert torch.cuda.is_available(), "timbre_bench needs an MI355X"
    what = set(a.what.split(","))
    sd = synth_state_dict(R.keys("mmm"))
    m = multi_modal_model(TimbreEncoder(**R.PROD_CONFIG), None, **R.MMM_CONFIG)
    m.load_state_dict(sd)
    m.cuda()
    H = R.PROD_CONFIG["hidden_dim"]
    whh_bytes = 4 * H * H * 4
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "w_hh_bytes": whh_bytes, "shapes": {}}
    if "host" in what:
        torch.set_num_threads(16)
        cfg = R.PROD_CONFIG
        cpu = torch.nn.ModuleDict({"input_layer": torch.nn.Linear(cfg["input_dim"], cfg["feature_dim"]),
                                   "lstm": torch.nn.LSTM(cfg["feature_dim"], H, num_layers=cfg["num_layers"], batch_first=True)})
        cpu.load_state_dict({k[len("timbre_encoder."):]: v for k, v in sd.items()
                             if k.startswith("timbre_encoder.input_layer") or k.startswith("timbre_encoder.lstm")})
        cpu.eval()
    for shape in a.shapes.split(","):
        B, W = (int(v) for v in shape.split("x"))
        x = synth_input(f"timbre_bench:{shape}", (B, 4, 128, W)).cuda()
        r = {}
        for _ in range(2):
            m.get_timbre_features(x)
        torch.cuda.synchronize()
        if "device" in what:
            r["get_timbre_features_ms"] = event_ms(lambda: m.get_timbre_features(x), a.iters, torch)
            r["w_hh_reread_bytes_per_call"] = 3 * W * whh_bytes
        if "step" in what:
            pre = synth_input(f"timbre_bench_pre:{shape}", (B, W, 4 * H)).cuda()
            w_hh = m.timbre_encoder._weights()["layers"][1][1]
            ws = torch.empty(L.load().ds_lstm_ws_floats(B, H), device="cuda")
            hs, h_last = torch.empty(B, W, H, device="cuda"), torch.empty(B, H, device="cuda")

            def layer():
                L.call("ds_lstm_layer", pre.data_ptr(), W * 4 * H, 4 * H, w_hh.data_ptr(), B, W, H, hs.data_ptr(), h_last.data_ptr(), ws.data_ptr(),
                       L.current_stream())
            layer()
            torch.cuda.synchronize()
            ms = event_ms(layer, a.iters, torch)
            r["lstm_layer_ms"], r["lstm_step_us"] = ms, ms / W * 1e3
            r["w_hh_bytes_per_s_of_a_step"] = whh_bytes * ((B + 15) // 16) / (ms / W * 1e-3)       # every 16-sample tile of blocks reads all of w_hh
        if "host" in what:
            xc = x.cpu()

            def host_way():
                with torch.no_grad():
                    y = cpu["input_layer"](xc.reshape(B, -1, W).permute(0, 2, 1))
                    return R.projection_head(sd, "spectrogram_projection", cpu["lstm"](y)[0][:, -1], torch.float32)
            host_way()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                host_way()
                ts.append((time.perf_counter() - t0) * 1e3)
            r["torch_cpu_16_threads_ms"] = statistics.median(ts)
        res["shapes"][shape] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
