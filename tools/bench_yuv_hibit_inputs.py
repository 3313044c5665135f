"""Encode from P010 frames measured, by the method of tools/bench_yuv_inputs.py: the RGB frames route of
section 15 against the P010 route on the same video, by where the frames lie.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream).  Source: a synthetic P010 video of 720 x 1280 (10-bit samples in the high bits of 16-bit words, random bits below
them), BT.2020 limited range; the RGB route gets the uint8 frames tdc_yuv_to_rgb makes of it, so both routes encode the same
pixels and their outputs are asserted torch.equal.  Cases (T0 frames decoded, frame cap): (1000, 224) and (512, 512).  Routes,
alternating inside one process, device events, --steps (>= 10) timed steps after --warmup rounds:

  rgb_pinned   encode_frames from pinned host RGB frames        p010_pinned   encode_frames from pinned host P010 planes
  rgb_device   encode_frames from device-resident RGB frames    p010_device   encode_frames from device-resident P010 planes

Per route: ms per step (median, min, max), bytes uploaded per step (RGB and P010 both upload 3 bytes per pixel).  Per case: the
conversion alone, ONE tdc_yuv_to_rgb launch over all kept frames (ms, bytes moved per second at 6 bytes per pixel), beside ONE
tdc_yuv420_to_rgb launch over as many 8-bit NV12 frames in the same run (4.5 bytes per pixel) and the resize of the same
frames, and

  spread_ms                        max - min of the RGB route's timed steps in that run (per residence)
  p010_minus_rgb_{pinned,device}   must not exceed spread_ms + the conversion's ms
  conversion tb_per_s              must be at least half of the 8-bit launch's in that run

--cpu-frames N (default 8) also times converting N frames on the host with numpy (the definition, as a caller without this
entry would have to for all T0 frames) and reports ms per frame.  The requirements are reported as booleans and make the exit
status.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_p010(T0, H, W, dev, seed=0, scene_len=21):
    """deterministic P010 planes on `dev` as int16 bit patterns: y [T0, H, W], uv [T0, H/2, W] - a scene is a constant base
    plus per-frame noise; the six bits below the sample hold random junk"""
    import torch
    g = torch.Generator(device=dev)
    y = torch.empty(T0, H, W, device=dev, dtype=torch.int16)
    uv = torch.empty(T0, H // 2, W, device=dev, dtype=torch.int16)

    def words(samples, shape):
        w = (samples.clamp_(0, 1023).to(torch.int32) << 6) | torch.randint(0, 64, shape, device=dev, generator=g, dtype=torch.int32)
        return torch.where(w >= 32768, w - 65536, w).to(torch.int16)      # the 16-bit pattern as int16

    for t in range(T0):
        if t % scene_len == 0:
            g.manual_seed(seed * 7919 + t // scene_len)
            by = torch.randint(0, 1024, (H, W), device=dev, generator=g, dtype=torch.int32)
            bc = torch.randint(0, 1024, (H // 2, W), device=dev, generator=g, dtype=torch.int32)
        g.manual_seed(seed * 104729 + 1000003 + t)
        y[t] = words(by + torch.randint(-48, 49, (H, W), device=dev, generator=g, dtype=torch.int32), (H, W))
        uv[t] = words(bc + torch.randint(-24, 25, (H // 2, W), device=dev, generator=g, dtype=torch.int32), (H // 2, W))
    return y, uv


def cpu_convert_ms_per_frame(y, uv, coef, n):
    """the definition in numpy on n host frames of P010 -> ms per frame (what converting outside the library costs)"""
    import numpy as np
    yw, cw = y[:n].cpu().numpy().view(np.uint16), uv[:n].cpu().numpy().view(np.uint16)
    y_off, cy, crv, cgu, cgv, cbu = (np.int32(c) for c in coef)
    t0 = time.perf_counter()
    Y = ((yw >> 6) & 1023).astype(np.int32)
    U = np.repeat(np.repeat(((cw[:, :, 0::2] >> 6) & 1023).astype(np.int32) - 512, 2, axis=1), 2, axis=2)
    V = np.repeat(np.repeat(((cw[:, :, 1::2] >> 6) & 1023).astype(np.int32) - 512, 2, axis=1), 2, axis=2)
    yy = cy * (Y - y_off) + np.int32(1 << 17)
    rgb = np.stack([np.clip((yy + crv * V) >> 18, 0, 255), np.clip((yy - cgu * U - cgv * V) >> 18, 0, 255),
                    np.clip((yy + cbu * U) >> 18, 0, 255)], axis=-1).astype(np.uint8)
    return (time.perf_counter() - t0) * 1e3 / n, rgb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--source", default="720x1280")
    ap.add_argument("--cases", default="1000:224,512:512", help="T0:cap pairs")
    ap.add_argument("--cpu-frames", type=int, default=8, help="frames converted on the host for the outside-the-library cost (0: skip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_hibit_inputs.py measures on a GPU; none is visible")
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import encode, ops, preprocess
    from tdc_video_amd.pipeline import VideoEncoder
    dev = torch.device("cuda", 0)
    K, H = args.K, args.hidden
    gen = torch.Generator(device=dev).manual_seed(0)
    sd = bench.random_state_dict(H, K, dev, gen)
    enc = VideoEncoder(sd, bench.model_cfg(H, K, 512), dtype=torch.float16, device=dev, tower_batch=512,
                       tower_dtype=torch.bfloat16, tower_res_dtype=torch.float16)
    del sd
    torch.cuda.empty_cache()
    prompt_ids = [101] + list(range(2000, 2010)) + [102]
    Hs, Ws = (int(v) for v in args.source.split("x"))
    coef = preprocess.yuv_coefficients("bt2020", False, 10)
    coef8 = preprocess.yuv_coefficients()

    def timed_ms(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def pinned(t):
        p = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        p.copy_(t)
        return p

    def p010(y, uv):
        return preprocess.YuvFrames.p010(y, uv, matrix="bt2020")

    results, ok, cpu = [], True, None
    for case in args.cases.split(","):
        T0, cap = (int(v) for v in case.split(":"))
        enc.two_streams = min(T0, cap) <= 128
        y, uv = synth_p010(T0, Hs, Ws, dev)
        rgb = ops.yuv_to_rgb(y, uv, uv[:, :, 1:], 2, coef, Hs, Ws, 10, True, "420")
        if args.cpu_frames and cpu is None:
            ms_frame, host_rgb = cpu_convert_ms_per_frame(y, uv, coef, min(args.cpu_frames, T0))
            assert torch.equal(torch.from_numpy(host_rgb), rgb[:host_rgb.shape[0]].cpu()), "the host conversion differs"
            cpu = {"frames_timed": int(host_rgb.shape[0]), "ms_per_frame": round(ms_frame, 2), "threads": torch.get_num_threads()}
            del host_rgb
        sources = {"rgb_pinned": pinned(rgb), "p010_pinned": p010(pinned(y), pinned(uv)), "rgb_device": rgb, "p010_device": p010(y, uv)}
        torch.cuda.synchronize()
        idx = encode.frame_indices(enc.cfg, T0, 64, cap)
        kept = len(idx)
        px = Hs * Ws
        uploaded = {"rgb_pinned": kept * px * 3, "p010_pinned": 2 * kept * (px + 2 * (Hs // 2) * (Ws // 2)), "rgb_device": 0, "p010_device": 0}
        ms = {n: [] for n in sources}
        outs = {}
        for r in range(args.warmup + args.steps):
            for name, src in sources.items():
                t, out = timed_ms(lambda: enc.encode_frames(src, 64, 64, prompt_ids, frame_cap=cap))
                outs[name] = out
                if r >= args.warmup:
                    ms[name].append(t)
                del out
        same = all(torch.equal(outs[n], outs["rgb_device"]) for n in sources)
        assert same, "the routes' outputs differ"
        outs.clear()
        # the upload as the product counts it, the two conversion launches alone and the resize of the same frames
        stats = {}
        enc.pixels_from_frames(sources["p010_pinned"], idx, stats=stats)
        assert stats["bytes_uploaded"] == uploaded["p010_pinned"], stats
        sel = torch.tensor(idx, device=dev)
        ky, kuv = y[sel], uv[sel]
        ky8 = ((ky.to(torch.int32) >> 8) & 255).to(torch.uint8)      # as many 8-bit NV12 frames for the older launch
        kuv8 = ((kuv.to(torch.int32) >> 8) & 255).to(torch.uint8)
        scratch = torch.empty(kept, Hs, Ws, 3, device=dev, dtype=torch.uint8)
        conv, conv8, resize = [], [], []
        for r in range(args.warmup + args.steps):
            t, _ = timed_ms(lambda: ops.yuv_to_rgb(ky, kuv, kuv[:, :, 1:], 2, coef, Hs, Ws, 10, True, "420", out=scratch))
            t8, _ = timed_ms(lambda: ops.yuv420_to_rgb(ky8, kuv8, kuv8[:, :, 1:], 2, coef8, Hs, Ws, out=scratch))
            t2, pxs = timed_ms(lambda: enc.pixels_from_frames(rgb, idx))
            del pxs
            if r >= args.warmup:
                conv.append(t)
                conv8.append(t8)
                resize.append(t2)
        del ky, kuv, ky8, kuv8, scratch
        conv_ms, conv8_ms, resize_ms = statistics.median(conv), statistics.median(conv8), statistics.median(resize)
        rate, rate8 = kept * px * 6 / (conv_ms * 1e-3) / 1e12, kept * px * 4.5 / (conv8_ms * 1e-3) / 1e12
        med = {n: statistics.median(v) for n, v in ms.items()}
        spread = {k: max(ms["rgb_" + k]) - min(ms["rgb_" + k]) for k in ("pinned", "device")}
        d_pin, d_dev = med["p010_pinned"] - med["rgb_pinned"], med["p010_device"] - med["rgb_device"]
        pin_ok, dev_ok = d_pin <= spread["pinned"] + conv_ms, d_dev <= spread["device"] + conv_ms
        rate_ok = rate >= 0.5 * rate8
        ok = ok and pin_ok and dev_ok and rate_ok
        results.append({"source": args.source, "frames_in": T0, "frame_cap": cap, "frames_kept": kept,
                        "routes": {n: {"ms_per_step": round(med[n], 3), "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3),
                                       "bytes_uploaded": uploaded[n]} for n in sources},
                        "outputs_bit_equal": same,
                        "conversion": {"ms": round(conv_ms, 4), "bytes_moved": kept * px * 6, "tb_per_s": round(rate, 3), "launches": 1},
                        "conversion_8bit_nv12_same_run": {"ms": round(conv8_ms, 4), "bytes_moved": int(kept * px * 4.5),
                                                          "tb_per_s": round(rate8, 3)},
                        "resize_same_frames_ms": round(resize_ms, 3),
                        "spread_ms": {k: round(v, 3) for k, v in spread.items()},
                        "p010_minus_rgb_pinned_ms": round(d_pin, 3), "p010_minus_rgb_device_ms": round(d_dev, 3),
                        "pinned_within_spread_plus_conversion": pin_ok, "device_within_spread_plus_conversion": dev_ok,
                        "conversion_at_least_half_the_8bit_rate": rate_ok})
        print("[bench_yuv_hibit_inputs] T0=%d cap=%d done" % (T0, cap), file=sys.stderr, flush=True)
        del sources, y, uv, rgb
        torch.cuda.empty_cache()
    res = {"tool": "bench_yuv_hibit_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "layout": "p010", "matrix": "bt2020", "full_range": False, "frame_slab": enc.frame_slab, "steps": args.steps,
           "warmup": args.warmup, "host_conversion_numpy": cpu, "cases": results, "requirements_met": ok}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
