"""Encode from decoded uint8 frames measured: what a caller with a real video pays in front of the
towers, by the route it takes.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream), as tools/bench_feature_store.py builds it.  Sources: synthetic uint8 videos of 360 x 640 and 720 x 1280.  Cases
(T0 frames decoded, frame cap): (512, 512) - a1 keeps every frame, all routes do the same device work - and (1000, 224) - the
reference's drivers' frame count against its own cap.  Routes, alternating inside one process, device events, --steps (>= 10)
timed steps after --warmup rounds:

  pixels_device   process_images of ALL T0 frames (device-resident), then encode_video: the only route before section 15
  pixels_pinned   the same from pinned host frames (process_images uploads every frame, once per tower)
  frames_device   encode_frames from device-resident frames
  frames_pinned   encode_frames from pinned host frames (the kept frames are gathered on the host and uploaded)

Per route: ms per step (median, min, max), the resize's own ms (process_images / pixels_from_frames alone) and its share of
the step, bytes uploaded per step, torch.cuda.max_memory_allocated over a step and the bytes allocated before it.  The outputs
of all routes are compared with torch.equal.  No threshold is fixed: at (512, 512) `frames_minus_pixels_device_ms` is reported
beside `alternation_spread_ms`, the spread (max - min) of the routes' own timed steps.

Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_frames(T0, H, W, dev, seed=0, scene_len=21):
    """deterministic uint8 [T0, H, W, 3] on `dev`: scene = constant base image + per-frame noise (bench.synth_video's shape)"""
    import torch
    g = torch.Generator(device=dev)
    out = torch.empty(T0, H, W, 3, device=dev, dtype=torch.uint8)
    base = None
    for t in range(T0):
        if t % scene_len == 0:
            g.manual_seed(seed * 7919 + t // scene_len)
            base = torch.randint(0, 256, (H, W, 3), device=dev, generator=g, dtype=torch.int16)
        g.manual_seed(seed * 104729 + 1000003 + t)
        out[t] = (base + torch.randint(-12, 13, (H, W, 3), device=dev, generator=g, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sources", default="360x640,720x1280")
    ap.add_argument("--cases", default="512:512,1000:224", help="T0:cap pairs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_frame_inputs.py measures on a GPU; none is visible")
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import encode, preprocess
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
    towers = enc.frame_towers

    def timed_ms(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    results = []
    for src in args.sources.split(","):
        Hs, Ws = (int(v) for v in src.split("x"))
        for case in args.cases.split(","):
            T0, cap = (int(v) for v in case.split(":"))
            enc.two_streams = min(T0, cap) <= 128
            fdev = synth_frames(T0, Hs, Ws, dev)
            fpin = torch.empty(fdev.shape, dtype=torch.uint8, pin_memory=True)
            fpin.copy_(fdev)
            torch.cuda.synchronize()
            frame_bytes = Hs * Ws * 3
            uploaded = {}

            def pixels_route(frames):
                ps, pd = preprocess.process_images(frames, enc.dtype, towers)
                return enc.encode_video(ps, pd, (Hs, Ws), 64, 64, prompt_ids, frame_cap=cap)

            def frames_route(frames, name):
                info = {}
                out = enc.encode_frames(frames, 64, 64, prompt_ids, frame_cap=cap, info=info)
                uploaded[name] = 0 if frames.is_cuda else info["frames_resized"] * frame_bytes
                return out

            routes = [("pixels_device", lambda: pixels_route(fdev)), ("pixels_pinned", lambda: pixels_route(fpin)),
                      ("frames_device", lambda: frames_route(fdev, "frames_device")),
                      ("frames_pinned", lambda: frames_route(fpin, "frames_pinned"))]
            uploaded.update(pixels_device=0, pixels_pinned=len(towers) * T0 * frame_bytes)
            ms = {n: [] for n, _ in routes}
            peak, before, outs = {}, {}, {}
            for r in range(args.warmup + args.steps):
                for name, fn in routes:
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    t, out = timed_ms(fn)
                    outs[name] = out
                    if r >= args.warmup:
                        ms[name].append(t)
                        peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated(dev))
                        before[name] = base
                    del out
            same = all(torch.equal(outs[n], outs["pixels_device"]) for n, _ in routes)
            outs.clear()
            # the resize alone: all T0 frames (the pixel routes) against the kept ones (the frame routes), device-resident
            idx = encode.frame_indices(enc.cfg, T0, 64, cap)
            kept = len(idx)
            resize = {"pixels": [], "frames": []}
            for r in range(args.warmup + args.steps):
                t, px = timed_ms(lambda: preprocess.process_images(fdev, enc.dtype, towers))
                del px
                t2, px = timed_ms(lambda: enc.pixels_from_frames(fdev, idx))
                del px
                if r >= args.warmup:
                    resize["pixels"].append(t)
                    resize["frames"].append(t2)

            def row(name):
                med = statistics.median(ms[name])
                rz = statistics.median(resize["pixels" if name.startswith("pixels") else "frames"])
                return {"ms_per_step": round(med, 3), "ms_min": round(min(ms[name]), 3), "ms_max": round(max(ms[name]), 3),
                        "resize_ms_device_resident": round(rz, 3), "resize_share_of_step": round(rz / med, 4),
                        "bytes_uploaded": uploaded[name], "max_memory_allocated": peak[name],
                        "allocated_before_step": before[name], "step_peak_over_before": peak[name] - before[name]}
            spread = max(max(v) - min(v) for v in ms.values())
            results.append({"source": src, "frames_in": T0, "frame_cap": cap, "frames_kept": kept,
                            "routes": {n: row(n) for n, _ in routes}, "outputs_bit_equal": same,
                            "frames_minus_pixels_device_ms": round(statistics.median(ms["frames_device"]) -
                                                                   statistics.median(ms["pixels_device"]), 3),
                            "frames_pinned_minus_pixels_pinned_ms": round(statistics.median(ms["frames_pinned"]) -
                                                                          statistics.median(ms["pixels_pinned"]), 3),
                            "alternation_spread_ms": round(spread, 3)})
            print("[bench_frame_inputs] %s T0=%d cap=%d done" % (src, T0, cap), file=sys.stderr, flush=True)
            del fdev, fpin
            torch.cuda.empty_cache()
    res = {"tool": "bench_frame_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "frame_towers": [t["R"] for t in towers], "frame_slab": enc.frame_slab, "steps": args.steps, "warmup": args.warmup,
           "cases": results}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
