"""Encode from YUV with interpolated chroma measured, by the method of tools/bench_yuv_packed_inputs.py:
the replicate route of sections 19 / 20 / 21 / 25 against the linear route on the same surface, by where the frames lie.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream).  Source: a synthetic video of 720 x 1280 as NV12 (siting left, BT.601), P010 (topleft, BT.2020), P010 with
transfer="pq" (topleft) and v210 (left, BT.2020; rows padded to 128 bytes).  Cases (T0 frames decoded, frame cap): (1000, 224)
and (512, 512).  Routes, alternating inside one process, device events, --steps (>= 10) timed steps after --warmup rounds:

  replicate_pinned   encode_frames, upsample="replicate", pinned host      linear_pinned   the same object with upsample="linear"
  replicate_device   the same, device-resident                             linear_device   the same object with upsample="linear"

Per route: ms per step (median, min, max).  Per surface and case: the conversion alone, ONE launch over all kept frames
(ms, bytes read + written per second), replicate beside linear in the same run, and

  spread_ms                             max - min of the replicate route's timed steps in that run (per residence)
  linear_minus_replicate_{pinned,device}   requirement 1: must not exceed spread_ms + (linear launch ms - replicate launch ms)
  conversion tb_per_s                   requirement 2: the linear launch's must be at least half of the replicate launch's

and what the feature buys: the largest per-channel difference between the two routes' RGB on a synthetic frame of saturated
colours meeting at a vertical and a horizontal edge.  The requirements are reported as booleans and make the exit status.
Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

#        name -> (layout, bits, matrix, transfer, siting)
KINDS = {"nv12_left": ("nv12", 8, "bt601", "sdr", "left"), "p010_topleft": ("p010", 10, "bt2020", "sdr", "topleft"),
         "p010_pq_topleft": ("p010", 10, "bt2020", "pq", "topleft"), "v210_left": ("v210", 10, "bt2020", "sdr", "left")}


def synth(layout, T0, H, W, dev):
    """the planes of one synthetic video on `dev`, as the constructor of its layout takes them"""
    if layout == "nv12":
        from bench_yuv_inputs import synth_nv12
        return synth_nv12(T0, H, W, dev)
    if layout == "p010":
        from bench_yuv_hibit_inputs import synth_p010
        return synth_p010(T0, H, W, dev)
    from bench_yuv_packed_inputs import pack_surface, synth_422
    return (pack_surface(*synth_422(T0, H, W, 10, dev), "v210", dev),)


def edge_frame(layout, H, W, dev):
    """one frame of mid luma whose chroma is saturated: (max, 0) left of the middle column and (0, max) right of it in the
    upper half, the other way round in the lower half"""
    import torch
    from bench_yuv_packed_inputs import as_int16, pack_surface
    bits = 8 if layout == "nv12" else 10
    top = (1 << bits) - 1
    Hc = H if layout == "v210" else H // 2
    left = torch.arange(W // 2, device=dev)[None, :] < W // 4 + 1                # an edge at an odd chroma column
    upper = torch.arange(Hc, device=dev)[:, None] < Hc // 2 + 1
    u = torch.where(left == upper, top, 0).to(torch.int32)[None]
    v = top - u
    y = torch.full((1, H, W), 1 << (bits - 1), device=dev, dtype=torch.int32)
    if layout == "v210":
        return (pack_surface(y.to(torch.int16), u.to(torch.int16), v.to(torch.int16), "v210", dev),)
    uv = torch.stack([u, v], -1).view(1, Hc, W)
    if layout == "nv12":
        return y.to(torch.uint8), uv.to(torch.uint8)
    return as_int16(y << 6), as_int16(uv << 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--source", default="720x1280")
    ap.add_argument("--cases", default="1000:224,512:512", help="T0:cap pairs")
    ap.add_argument("--kinds", default=",".join(KINDS), help="of %s" % ", ".join(KINDS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_chroma_inputs.py measures on a GPU; none is visible")
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
    Hs, Ws = (int(v) for v in args.source.split("x"))
    px = Hs * Ws

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

    results, ok = [], True
    for kind in args.kinds.split(","):
        layout, bits, matrix, transfer, siting = KINDS[kind]

        def frames(planes, upsample):
            kw = dict(matrix=matrix, transfer=transfer, upsample=upsample, siting=siting)
            if layout == "v210":
                return preprocess.YuvFrames.v210(planes[0], Ws, **kw)
            return (preprocess.YuvFrames.nv12 if layout == "nv12" else preprocess.YuvFrames.p010)(*planes, **kw)

        # what the feature buys: the two routes' RGB on saturated colours meeting at an edge
        edge = edge_frame(layout, Hs, Ws, dev)
        rgbs = []
        for up in preprocess.CHROMA_UPSAMPLE:
            f = frames(edge, up)
            rgbs.append(f.to_rgb(list(f.planes()), torch.empty(1, Hs, Ws, 3, device=dev, dtype=torch.uint8)).to(torch.int16))
        edge_diff = [int(v) for v in (rgbs[0] - rgbs[1]).abs().amax(dim=(0, 1, 2)).tolist()]
        del edge, rgbs

        for case in args.cases.split(","):
            T0, cap = (int(v) for v in case.split(":"))
            enc.two_streams = min(T0, cap) <= 128
            planes = synth(layout, T0, Hs, Ws, dev)
            host = tuple(pinned(p) for p in planes)
            sources = {"replicate_pinned": frames(host, "replicate"), "linear_pinned": frames(host, "linear"),
                       "replicate_device": frames(planes, "replicate"), "linear_device": frames(planes, "linear")}
            torch.cuda.synchronize()
            idx = encode.frame_indices(enc.cfg, T0, 64, cap)
            kept = len(idx)
            ms = {n: [] for n in sources}
            outs = {}
            for r in range(args.warmup + args.steps):
                for name, src in sources.items():
                    t, out = timed_ms(lambda: enc.encode_frames(src, 64, 64, prompt_ids, frame_cap=cap))
                    outs[name] = out
                    if r >= args.warmup:
                        ms[name].append(t)
                    del out
            same = all(torch.equal(outs[r + "_pinned"], outs[r + "_device"]) for r in preprocess.CHROMA_UPSAMPLE)
            assert same, "a route's output depends on where the frames lie"
            routes_differ = not torch.equal(outs["replicate_device"], outs["linear_device"])
            outs.clear()
            # the conversion launches alone, on the kept frames
            sel = torch.tensor(idx, device=dev)
            f_rep, f_lin = sources["replicate_device"], sources["linear_device"]
            kept_planes = [p[sel] for p in f_rep.planes()]
            read = sum(p[0].numel() * p.element_size() for p in kept_planes)
            scratch = torch.empty(kept, Hs, Ws, 3, device=dev, dtype=torch.uint8)
            launches = {"replicate": lambda: f_rep.to_rgb(kept_planes, scratch), "linear": lambda: f_lin.to_rgb(kept_planes, scratch)}
            lms = {n: [] for n in launches}
            for r in range(args.warmup + args.steps):
                for n, fn in launches.items():
                    t, _ = timed_ms(fn)
                    if r >= args.warmup:
                        lms[n].append(t)
            del sources, kept_planes, scratch, f_rep, f_lin
            moved = kept * (read + 3 * px)
            conv = {n: {"ms": round(statistics.median(v_), 4), "bytes_moved": moved,
                        "tb_per_s": round(moved / (statistics.median(v_) * 1e-3) / 1e12, 3)} for n, v_ in lms.items()}
            extra = statistics.median(lms["linear"]) - statistics.median(lms["replicate"])
            med = {n: statistics.median(v_) for n, v_ in ms.items()}
            spread = {k: max(ms["replicate_" + k]) - min(ms["replicate_" + k]) for k in ("pinned", "device")}
            d_pin, d_dev = med["linear_pinned"] - med["replicate_pinned"], med["linear_device"] - med["replicate_device"]
            pin_ok, dev_ok = d_pin <= spread["pinned"] + extra, d_dev <= spread["device"] + extra
            rate_ok = conv["linear"]["tb_per_s"] >= 0.5 * conv["replicate"]["tb_per_s"]
            ok = ok and pin_ok and dev_ok and rate_ok
            results.append({"kind": kind, "layout": layout, "bits": bits, "matrix": matrix, "transfer": transfer, "siting": siting,
                            "source": args.source, "frames_in": T0, "frame_cap": cap, "frames_kept": kept,
                            "routes": {n: {"ms_per_step": round(med[n], 3), "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3)}
                                       for n in ms},
                            "residences_bit_equal": same, "routes_differ": routes_differ, "conversion": conv,
                            "linear_launch_minus_replicate_launch_ms": round(extra, 4),
                            "spread_ms": {k: round(v_, 3) for k, v_ in spread.items()},
                            "linear_minus_replicate_pinned_ms": round(d_pin, 3), "linear_minus_replicate_device_ms": round(d_dev, 3),
                            "requirement_1_pinned_met": pin_ok, "requirement_1_device_met": dev_ok, "requirement_2_met": rate_ok,
                            "saturated_edge_largest_difference_rgb": edge_diff})
            print("[bench_yuv_chroma_inputs] %s T0=%d cap=%d done" % (kind, T0, cap), file=sys.stderr, flush=True)
            del planes, host
            torch.cuda.empty_cache()
    res = {"tool": "bench_yuv_chroma_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "full_range": False, "frame_slab": enc.frame_slab, "steps": args.steps, "warmup": args.warmup, "cases": results,
           "requirements_met": ok}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
