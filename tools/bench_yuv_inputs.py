"""Encode from YUV 4:2:0 frames measured: the RGB frames route of section 15 against the 4:2:0 route on
the same video, by where the frames lie.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream), as tools/bench_frame_inputs.py builds it.  Source: a synthetic NV12 video of 720 x 1280; the RGB route gets the
uint8 frames tdc_yuv420_to_rgb makes of it, so both routes encode the same pixels and their outputs are asserted
torch.equal.  Cases (T0 frames decoded, frame cap): (1000, 224) and (512, 512).  Routes, alternating inside one process,
device events, --steps (>= 10) timed steps after --warmup rounds:

  rgb_pinned   encode_frames from pinned host RGB frames        yuv_pinned   encode_frames from pinned host NV12 planes
  rgb_device   encode_frames from device-resident RGB frames    yuv_device   encode_frames from device-resident NV12 planes

Per route: ms per step (median, min, max), bytes uploaded per step, torch.cuda.max_memory_allocated over a step above the
bytes allocated before it.  Per case: the conversion alone, ONE launch over all kept frames (ms, bytes moved per second at 4.5
bytes per pixel), beside the resize of the same frames (pixels_from_frames on the device-resident RGB frames), and

  spread_ms                  max - min of the RGB route's timed steps in that run (per residence)
  yuv_minus_rgb_pinned_ms    must not exceed spread_ms
  yuv_minus_rgb_device_ms    must not exceed spread_ms + the conversion's ms

The two requirements are reported as booleans and make the exit status.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_nv12(T0, H, W, dev, seed=0, scene_len=21):
    """deterministic NV12 planes on `dev`: y [T0, H, W], uv [T0, H/2, W] - a scene is a constant base plus per-frame noise"""
    import torch
    g = torch.Generator(device=dev)
    y = torch.empty(T0, H, W, device=dev, dtype=torch.uint8)
    uv = torch.empty(T0, H // 2, W, device=dev, dtype=torch.uint8)
    for t in range(T0):
        if t % scene_len == 0:
            g.manual_seed(seed * 7919 + t // scene_len)
            by = torch.randint(0, 256, (H, W), device=dev, generator=g, dtype=torch.int16)
            bc = torch.randint(0, 256, (H // 2, W), device=dev, generator=g, dtype=torch.int16)
        g.manual_seed(seed * 104729 + 1000003 + t)
        y[t] = (by + torch.randint(-12, 13, (H, W), device=dev, generator=g, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
        uv[t] = (bc + torch.randint(-6, 7, (H // 2, W), device=dev, generator=g, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
    return y, uv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--source", default="720x1280")
    ap.add_argument("--cases", default="1000:224,512:512", help="T0:cap pairs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_inputs.py measures on a GPU; none is visible")
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
    coef = preprocess.yuv_coefficients()

    def timed_ms(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def pinned(t):
        p = torch.empty(t.shape, dtype=torch.uint8, pin_memory=True)
        p.copy_(t)
        return p

    results, ok = [], True
    for case in args.cases.split(","):
        T0, cap = (int(v) for v in case.split(":"))
        enc.two_streams = min(T0, cap) <= 128
        y, uv = synth_nv12(T0, Hs, Ws, dev)
        rgb = ops.yuv420_to_rgb(y, uv, uv[:, :, 1:], 2, coef, Hs, Ws)
        sources = {"rgb_pinned": pinned(rgb), "yuv_pinned": preprocess.YuvFrames.nv12(pinned(y), pinned(uv)),
                   "rgb_device": rgb, "yuv_device": preprocess.YuvFrames.nv12(y, uv)}
        torch.cuda.synchronize()
        idx = encode.frame_indices(enc.cfg, T0, 64, cap)
        kept = len(idx)
        px = Hs * Ws
        uploaded = {"rgb_pinned": kept * px * 3, "yuv_pinned": kept * (px + 2 * (Hs // 2) * (Ws // 2)), "rgb_device": 0, "yuv_device": 0}
        ms = {n: [] for n in sources}
        peak, outs = {}, {}
        for r in range(args.warmup + args.steps):
            for name, src in sources.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                t, out = timed_ms(lambda: enc.encode_frames(src, 64, 64, prompt_ids, frame_cap=cap))
                outs[name] = out
                if r >= args.warmup:
                    ms[name].append(t)
                    peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated(dev) - base)
                del out
        same = all(torch.equal(outs[n], outs["rgb_device"]) for n in sources)
        assert same, "the routes' outputs differ"
        outs.clear()
        # stats of the upload as the product counts it, the conversion launch alone and the resize of the same frames
        stats = {}
        enc.pixels_from_frames(sources["yuv_pinned"], idx, stats=stats)
        assert stats["bytes_uploaded"] == uploaded["yuv_pinned"], stats
        sel = torch.tensor(idx, device=dev)
        ky, kuv = y[sel], uv[sel]
        scratch = torch.empty(kept, Hs, Ws, 3, device=dev, dtype=torch.uint8)
        conv, resize = [], []
        for r in range(args.warmup + args.steps):
            t, _ = timed_ms(lambda: ops.yuv420_to_rgb(ky, kuv, kuv[:, :, 1:], 2, coef, Hs, Ws, out=scratch))
            t2, pxs = timed_ms(lambda: enc.pixels_from_frames(rgb, idx))
            del pxs
            if r >= args.warmup:
                conv.append(t)
                resize.append(t2)
        del ky, kuv, scratch
        conv_ms, resize_ms = statistics.median(conv), statistics.median(resize)
        med = {n: statistics.median(v) for n, v in ms.items()}
        spread = {k: max(ms["rgb_" + k]) - min(ms["rgb_" + k]) for k in ("pinned", "device")}
        d_pin, d_dev = med["yuv_pinned"] - med["rgb_pinned"], med["yuv_device"] - med["rgb_device"]
        pin_ok, dev_ok = d_pin <= spread["pinned"], d_dev <= spread["device"] + conv_ms
        ok = ok and pin_ok and dev_ok
        results.append({"source": args.source, "frames_in": T0, "frame_cap": cap, "frames_kept": kept,
                        "routes": {n: {"ms_per_step": round(med[n], 3), "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3),
                                       "bytes_uploaded": uploaded[n], "step_peak_over_before": peak[n]} for n in sources},
                        "outputs_bit_equal": same,
                        "conversion": {"ms": round(conv_ms, 4), "bytes_moved": int(kept * px * 4.5),
                                       "tb_per_s": round(kept * px * 4.5 / (conv_ms * 1e-3) / 1e12, 3), "launches": 1,
                                       "gather_rows_tb_per_s_section_14": 5.1},
                        "resize_same_frames_ms": round(resize_ms, 3),
                        "spread_ms": {k: round(v, 3) for k, v in spread.items()},
                        "yuv_minus_rgb_pinned_ms": round(d_pin, 3), "yuv_minus_rgb_device_ms": round(d_dev, 3),
                        "pinned_within_spread": pin_ok, "device_within_spread_plus_conversion": dev_ok})
        print("[bench_yuv_inputs] T0=%d cap=%d done" % (T0, cap), file=sys.stderr, flush=True)
        del sources, y, uv, rgb
        torch.cuda.empty_cache()
    res = {"tool": "bench_yuv_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "layout": "nv12", "matrix": "bt601", "full_range": False, "frame_slab": enc.frame_slab, "steps": args.steps,
           "warmup": args.warmup, "cases": results, "requirements_met": ok}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
