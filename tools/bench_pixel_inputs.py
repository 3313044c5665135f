"""Encode from channel-first, BGRA and gray frames measured: a step fed preprocess.RgbFrames over the
pictures as their source writes them - packed to R G B on the device - against the same step fed the [T0, H, W, 3] RGB frames a
host converted beforehand, which is what a caller had to do before and is the yardstick.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream), as tools/bench_orient_inputs.py builds it.  Source: the RGB frames of the synthetic video of
tools/bench_yuv_hibit_inputs.py, 720 x 1280, stored three ways: channel-first [T0, 3, H, W] ("chw"), B G R A pixels with a row
pitch of W * 4 + 64 bytes and random alpha ("bgra"), and one gray plane [T0, H, W] (the G channel; "gray").  Cases (T0 frames
decoded, frame cap): (1000, 224) and (512, 512).  Routes, alternating inside one process, device events, --steps (>= 10) timed
steps after --warmup rounds, for residence in (pinned, device):

  plain_<residence>         encode_frames(the [T0, H, W, 3] RGB frames): the yardstick of chw and bgra
  chw_<residence>           encode_frames(RgbFrames.chw(...))
  bgra_<residence>          encode_frames(RgbFrames(..., "hwc", "bgra"))
  grayplain_<residence>     encode_frames(the gray plane replicated into [T0, H, W, 3] beforehand): the yardstick of gray
  gray_<residence>          encode_frames(RgbFrames.gray(...))

A route and its yardstick encode the same pixels and their outputs are asserted torch.equal.  Per route: ms per step (median,
min, max), bytes uploaded per step, peak memory of a step above the bytes allocated before it.  Per case: route minus yardstick
beside the yardstick's spread (max - min).  The host conversions a caller paid before the call, timed on --host-frames frames
and scaled to T0 (the whole video: the caller converts before a1 selects): permute(0, 2, 3, 1).contiguous() of a channel-first
tensor, [..., ::-1].copy() of B G R frames, [..., :3].copy() of R G B A frames.  Once: ONE tdc_pack_rgb launch over 224 frames of
720 x 1280 per form - planar colour, planar gray, interleaved-3 (bgr), interleaved-4 as one 16-byte load (bgra, dense),
interleaved-4 as four words (bgra, base 4 bytes off), and the byte form of each (dst one byte off) - beside
tdc_orient_frames's (0, False) plain copy of the same frames in the same run (ms, GB/s counting the bytes read and the bytes
written, and the rate relative to the copy's scaled by (C + 3) / 6), and the resize of the same frames.  Nothing is required of
the numbers: the exit status is 0 when the outputs agree.  --launch-only stops after the launch alone.  Prints one JSON line;
--out also writes it."""
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
    ap.add_argument("--host-frames", type=int, default=128, help="frames the host conversions are timed on")
    ap.add_argument("--launch-only", action="store_true", help="the launch alone and the host conversions, no steps")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pixel_inputs.py measures on a GPU; none is visible")
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
    coef = preprocess.yuv_coefficients("bt2020", False, 10)
    RgbFrames = preprocess.RgbFrames
    PITCH = Ws * 4 + 64

    def timed_ms(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def pinned(t):
        """a pinned copy of t with t's strides (t: a view that starts at the first byte of its memory)"""
        n = sum((d - 1) * s for d, s in zip(t.shape, t.stride())) + 1
        p = torch.empty(n, dtype=t.dtype, pin_memory=True).as_strided(t.shape, t.stride(), 0)
        p.copy_(t)
        return p

    def bgra_of(rgb, offset=0):
        """B G R A pixels with a row pitch and random alpha, `offset` bytes into their allocation"""
        T = rgb.shape[0]
        buf = torch.empty(offset + T * Hs * PITCH, dtype=torch.uint8, device=dev).random_(0, 256, generator=gen)
        view = buf.as_strided((T, Hs, Ws, 4), (Hs * PITCH, PITCH, 4, 1), offset)
        view[..., :3] = rgb.flip(3)
        return view

    def median_ms(fn):
        ms = []
        for r in range(args.warmup + args.steps):
            t, _ = timed_ms(fn)
            if r >= args.warmup:
                ms.append(t)
        return statistics.median(ms)

    launch, host_cost = None, None
    results, same_all = [], True
    for case in args.cases.split(","):
        T0, cap = (int(v) for v in case.split(":"))
        enc.two_streams = min(T0, cap) <= 128
        y, uv = synth_p010(T0, Hs, Ws, dev)
        rgb = ops.yuv_to_rgb(y, uv, uv[:, :, 1:], 2, coef, Hs, Ws, 10, True, "420")
        del y, uv
        chw = rgb.permute(0, 3, 1, 2).contiguous()
        bgra = bgra_of(rgb)
        gray = rgb[..., 1].contiguous()
        grayplain = gray[..., None].expand(T0, Hs, Ws, 3).contiguous()
        idx = encode.frame_indices(enc.cfg, T0, 64, cap)
        kept = len(idx)

        if host_cost is None:      # what a caller paid before the call, per frame of the whole video
            n_host = min(args.host_frames, T0)
            h_chw, h_rgb = chw[:n_host].cpu(), rgb[:n_host].cpu().numpy()
            h_bgr, h_rgba = np.ascontiguousarray(h_rgb[..., ::-1]), np.concatenate([h_rgb, h_rgb[..., :1]], -1)
            host_cost = {"frames_timed": n_host, "ms_per_frame": {}}
            for name, fn, want in (("chw: permute(0, 2, 3, 1).contiguous()", lambda: h_chw.permute(0, 2, 3, 1).contiguous().numpy(), h_rgb),
                                   ("bgr: [..., ::-1].copy()", lambda: h_bgr[..., ::-1].copy(), h_rgb),
                                   ("rgba: [..., :3].copy()", lambda: h_rgba[..., :3].copy(), h_rgb)):
                t0 = time.perf_counter()
                got = fn()
                host_cost["ms_per_frame"][name] = round((time.perf_counter() - t0) * 1e3 / n_host, 4)
                assert np.array_equal(got, want), name
            del h_chw, h_rgb, h_bgr, h_rgba, got

        if launch is None:      # the launch alone, once: 224 frames
            n = min(224, T0)
            src = rgb[:n].contiguous()
            room = torch.empty(n * Hs * Ws * 3 + 4, device=dev, dtype=torch.uint8)
            px = n * Hs * Ws
            copy_ms = median_ms(lambda: ops.orient_frames(src, 0, 0, out=room[:3 * px].view(n, Hs, Ws, 3)))
            assert torch.equal(room[:3 * px].view(n, Hs, Ws, 3)[-1], src[-1])
            copy_rate = 6 * px / (copy_ms * 1e-3)
            launch = {"frames": n, "copy": {"what": "tdc_orient_frames (0, False)", "ms": round(copy_ms, 4), "bytes_per_pixel": 6,
                                            "gb_per_s": round(copy_rate / 1e9, 1)}, "forms": {}}
            bgr3 = src.flip(3).contiguous()
            forms = {"planar_colour": (RgbFrames.chw(chw[:n]), src, 3), "planar_gray": (RgbFrames.gray(gray[:n]), grayplain[:n], 1),
                     "interleaved3_bgr": (RgbFrames(bgr3, "hwc", "bgr"), src, 3),
                     "interleaved4_bgra_16_byte_loads": (RgbFrames(bgra[:n], "hwc", "bgra"), src, 4),
                     "interleaved4_bgra_word_loads": (RgbFrames(bgra_of(src, 4), "hwc", "bgra"), src, 4)}
            for name, (r, want, C) in forms.items():
                for off, kind in ((0, "word"), (1, "byte")):
                    out = room[off:off + 3 * px].view(n, Hs, Ws, 3)
                    if kind == "byte" and "word_loads" in name:
                        continue       # the same byte form as the 16-byte case's
                    m = median_ms(lambda: r.pack(out))
                    assert torch.equal(out[-1], want[-1]) and torch.equal(out[0], want[0]), (name, kind)
                    moved = (C + 3) * px
                    launch["forms"][name if kind == "word" else name.split("_16_")[0] + "_byte_form"] = \
                        {"ms": round(m, 4), "bytes_per_pixel": C + 3, "gb_per_s": round(moved / (m * 1e-3) / 1e9, 1),
                         "rate_over_copy_rate": round(moved / (m * 1e-3) / copy_rate, 3),
                         "ms_expected_at_copy_rate": round(copy_ms * (C + 3) / 6, 4)}
            resize = []
            for r in range(args.warmup + args.steps):
                t, pxs = timed_ms(lambda: enc.pixels_from_frames(src, None))
                del pxs
                if r >= args.warmup:
                    resize.append(t)
            launch["resize_same_frames_ms"] = round(statistics.median(resize), 3)
            del src, room, out, bgr3, forms
            torch.cuda.empty_cache()
            print("[bench_pixel_inputs] launch alone done", file=sys.stderr, flush=True)
        if args.launch_only:
            break

        sources = {"plain_pinned": pinned(rgb), "plain_device": rgb,
                   "chw_pinned": RgbFrames.chw(pinned(chw)), "chw_device": RgbFrames.chw(chw),
                   "bgra_pinned": RgbFrames(pinned(bgra), "hwc", "bgra"), "bgra_device": RgbFrames(bgra, "hwc", "bgra"),
                   "grayplain_pinned": pinned(grayplain), "grayplain_device": grayplain,
                   "gray_pinned": RgbFrames.gray(pinned(gray)), "gray_device": RgbFrames.gray(gray)}
        yardstick = {"chw": "plain", "bgra": "plain", "gray": "grayplain"}
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
            print("[bench_pixel_inputs] T0=%d cap=%d round %d" % (T0, cap, r), file=sys.stderr, flush=True)
        same = all(torch.equal(outs["%s_%s" % (k, res)], outs[y + "_device"]) and torch.equal(outs["%s_%s" % (y, res)], outs[y + "_device"])
                   for k, y in yardstick.items() for res in ("pinned", "device"))
        same_all = same_all and same
        outs.clear()
        for name, src in sources.items():
            stats = {}
            enc.pixels_from_frames(src, idx, stats=stats)
            uploaded[name] = stats["bytes_uploaded"]
        med = {n: statistics.median(v) for n, v in ms.items()}
        pairs = {}
        for k, y in yardstick.items():
            for res in ("pinned", "device"):
                ref = ms["%s_%s" % (y, res)]
                pairs["%s_%s" % (k, res)] = {"yardstick": "%s_%s" % (y, res),
                                             "minus_yardstick_ms": round(med["%s_%s" % (k, res)] - med["%s_%s" % (y, res)], 3),
                                             "yardstick_spread_ms": round(max(ref) - min(ref), 3)}
        results.append({"source": args.source, "frames_in": T0, "frame_cap": cap, "frames_kept": kept, "bgra_row_pitch": PITCH,
                        "routes": {n: {"ms_per_step": round(med[n], 3), "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3),
                                       "bytes_uploaded": uploaded[n], "step_peak_over_before": peak[n]} for n in sources},
                        "outputs_bit_equal": same, "pairs": pairs,
                        "host_conversion_ms_whole_video": {k: round(v * T0, 1) for k, v in host_cost["ms_per_frame"].items()}})
        print("[bench_pixel_inputs] T0=%d cap=%d done" % (T0, cap), file=sys.stderr, flush=True)
        del sources, rgb, chw, bgra, gray, grayplain
        torch.cuda.empty_cache()
    res = {"tool": "bench_pixel_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "frame_slab": enc.frame_slab, "steps": args.steps, "warmup": args.warmup, "launch_alone": launch,
           "host_conversion": host_cost, "cases": results, "outputs_bit_equal": same_all}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if same_all else 1)


if __name__ == "__main__":
    main()
