"""Encode from rotated video measured: a step fed preprocess.Oriented(frames, 90) - the stored landscape
surface plus "rotate 90", turned upright on the device - against the same step fed frames that were rotated beforehand, which
is what a caller had to do before.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream), as tools/bench_yuv_inputs.py builds it.  Source: the synthetic P010 video of tools/bench_yuv_hibit_inputs.py,
720 x 1280, and the RGB frames tdc_yuv_to_rgb makes of it.  Cases (T0 frames decoded, frame cap): (1000, 224) and (512, 512).
Routes, alternating inside one process, device events, --steps (>= 10) timed steps after --warmup rounds, for kind in
(rgb, p010) and residence in (pinned, device):

  <kind>_<residence>_oriented   encode_frames(Oriented(stored frames, 90))
  <kind>_<residence>_rotated    encode_frames(frames rotated beforehand): torch.rot90 of the RGB frames, or of the luma plane and
                                of the plane of (u, v) pairs (4:2:0 with even sizes stays 4:2:0 under a quarter turn)

The two routes of a kind encode the same pixels and their outputs are asserted torch.equal.  Per route: ms per step (median,
min, max), bytes uploaded per step, peak memory of a step above the bytes allocated before it.  Per case: oriented minus
rotated per kind and residence beside the rotated route's spread (max - min); the host rotation a caller paid before the call -
np.ascontiguousarray(np.rot90(frame, -1)) per frame, timed on --host-frames frames and scaled to T0, the whole video since the
caller rotates before a1 selects - and the rotated step with it added.  Once: ONE tdc_orient_frames launch over 224 frames
of 720 x 1280 for each of the seven non-identity orientations and the plain copy (ms, GB/s counting the bytes read and the
bytes written), and the resize of the same frames.  Nothing is required of the numbers: the exit status is 0 when the
outputs agree.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--source", default="720x1280")
    ap.add_argument("--cases", default="1000:224,512:512", help="T0:cap pairs")
    ap.add_argument("--host-frames", type=int, default=128, help="frames the host rotation is timed on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_orient_inputs.py measures on a GPU; none is visible")
    import bench
    import tdc_video_amd  # noqa: F401
    from bench_yuv_hibit_inputs import synth_p010
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
    assert Hs % 2 == 0 and Ws % 2 == 0, "the pre-rotated 4:2:0 planes need even sizes"
    coef = preprocess.yuv_coefficients("bt2020", False, 10)
    Oriented = preprocess.Oriented

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

    def quarter_turn(y, uv):
        """the planes of the frames turned 90 degrees clockwise: the luma plane and the plane of (u, v) pairs, each turned"""
        T0, Hc, W2 = uv.shape
        pairs = torch.rot90(uv.view(T0, Hc, W2 // 2, 2), -1, dims=(1, 2)).contiguous()
        return torch.rot90(y, -1, dims=(1, 2)).contiguous(), pairs.view(T0, W2 // 2, 2 * Hc)

    launch = None
    results, same_all = [], True
    for case in args.cases.split(","):
        T0, cap = (int(v) for v in case.split(":"))
        enc.two_streams = min(T0, cap) <= 128
        y, uv = synth_p010(T0, Hs, Ws, dev)
        rgb = ops.yuv_to_rgb(y, uv, uv[:, :, 1:], 2, coef, Hs, Ws, 10, True, "420")
        rgb_up = torch.rot90(rgb, -1, dims=(1, 2)).contiguous()
        y_up, uv_up = quarter_turn(y, uv)
        idx = encode.frame_indices(enc.cfg, T0, 64, cap)
        kept = len(idx)

        # what a caller paid before the call: every frame of the video rotated on the host
        n_host = min(args.host_frames, T0)
        host = rgb[:n_host].cpu().numpy()
        t0 = time.perf_counter()
        turned = [np.ascontiguousarray(np.rot90(f, -1)) for f in host]
        host_ms_frame = (time.perf_counter() - t0) * 1e3 / n_host
        assert torch.equal(torch.from_numpy(np.stack(turned)), rgb_up[:n_host].cpu()), "the host rotation differs"
        del host, turned

        if launch is None:      # the launch alone, once: 224 frames
            n = min(224, T0)
            src, dst = rgb[:n].contiguous(), torch.empty(n * Hs * Ws * 3, device=dev, dtype=torch.uint8)
            moved = 2 * src.numel()
            launch = {"frames": n, "bytes_read_plus_written": moved, "orientations": {}}
            for q, h in [(0, 0)] + [(r // 90, int(f)) for r in (0, 90, 180, 270) for f in (False, True) if (r, f) != (0, False)]:
                out = dst.view(n, Ws, Hs, 3) if q & 1 else dst.view(n, Hs, Ws, 3)
                ms = []
                for r in range(args.warmup + args.steps):
                    t, _ = timed_ms(lambda: ops.orient_frames(src, q, h, out=out))
                    if r >= args.warmup:
                        ms.append(t)
                want = torch.rot90(src[-1], -q, dims=(0, 1))
                assert torch.equal(out[-1], want.flip(1) if h else want), (q, h)
                m = statistics.median(ms)
                launch["orientations"]["copy" if (q, h) == (0, 0) else "rotate%d%s" % (90 * q, "_hflip" if h else "")] = \
                    {"ms": round(m, 4), "gb_per_s": round(moved / (m * 1e-3) / 1e9, 1)}
            resize = []
            for r in range(args.warmup + args.steps):
                t, pxs = timed_ms(lambda: enc.pixels_from_frames(rgb_up[:n], None))
                del pxs
                if r >= args.warmup:
                    resize.append(t)
            launch["resize_same_frames_ms"] = round(statistics.median(resize), 3)
            o = launch["orientations"]
            launch["slowest_transposing_over_rotate180"] = round(max(o[k]["ms"] for k in o if "90" in k or "270" in k) / o["rotate180"]["ms"], 3)
            del src, dst, out
            print("[bench_orient_inputs] launch alone done", file=sys.stderr, flush=True)

        sources = {"rgb_pinned_oriented": Oriented(pinned(rgb), 90), "rgb_pinned_rotated": pinned(rgb_up),
                   "rgb_device_oriented": Oriented(rgb, 90), "rgb_device_rotated": rgb_up,
                   "p010_pinned_oriented": Oriented(p010(pinned(y), pinned(uv)), 90), "p010_pinned_rotated": p010(pinned(y_up), pinned(uv_up)),
                   "p010_device_oriented": Oriented(p010(y, uv), 90), "p010_device_rotated": p010(y_up, uv_up)}
        torch.cuda.synchronize()
        ms = {n: [] for n in sources}
        peak, outs, uploaded = {}, {}, {}
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
            print("[bench_orient_inputs] T0=%d cap=%d round %d" % (T0, cap, r), file=sys.stderr, flush=True)
        same = all(torch.equal(outs[k + "_oriented"], outs["rgb_device_rotated"]) and torch.equal(outs[k + "_rotated"], outs["rgb_device_rotated"])
                   for k in ("rgb_pinned", "rgb_device", "p010_pinned", "p010_device"))
        same_all = same_all and same
        outs.clear()
        for name, src in sources.items():
            stats = {}
            enc.pixels_from_frames(src, idx, stats=stats)
            uploaded[name] = stats["bytes_uploaded"]
        med = {n: statistics.median(v) for n, v in ms.items()}
        pairs = {}
        for k in ("rgb_pinned", "rgb_device", "p010_pinned", "p010_device"):
            rot = ms[k + "_rotated"]
            pairs[k] = {"oriented_minus_rotated_ms": round(med[k + "_oriented"] - med[k + "_rotated"], 3),
                        "rotated_spread_ms": round(max(rot) - min(rot), 3)}
        host_ms = host_ms_frame * T0
        results.append({"source": args.source, "rotate": 90, "frames_in": T0, "frame_cap": cap, "frames_kept": kept,
                        "routes": {n: {"ms_per_step": round(med[n], 3), "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3),
                                       "bytes_uploaded": uploaded[n], "step_peak_over_before": peak[n]} for n in sources},
                        "outputs_bit_equal": same, "pairs": pairs,
                        "host_rotation": {"what": "np.ascontiguousarray(np.rot90(frame, -1)) per RGB frame", "frames_timed": n_host,
                                          "ms_per_frame": round(host_ms_frame, 3), "ms_whole_video": round(host_ms, 1),
                                          "rotated_step_plus_host_rotation_ms": round(med["rgb_pinned_rotated"] + host_ms, 1),
                                          "p010": "not measured: the planes of a YuvFrames had no host rotation route"}})
        print("[bench_orient_inputs] T0=%d cap=%d done" % (T0, cap), file=sys.stderr, flush=True)
        del sources, y, uv, rgb, rgb_up, y_up, uv_up
        torch.cuda.empty_cache()
    res = {"tool": "bench_orient_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "frame_slab": enc.frame_slab, "steps": args.steps, "warmup": args.warmup, "launch_alone": launch, "cases": results,
           "outputs_bit_equal": same_all}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if same_all else 1)


if __name__ == "__main__":
    main()
