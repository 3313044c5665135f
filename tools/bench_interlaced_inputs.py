"""Encode from interlaced video measured: a step fed preprocess.Interlaced(surface) - one field kept,
uploaded, converted and rebuilt to full height on the device - against the same step fed full-height frames of the same
surface kind, which is what a caller who deinterlaces on the host hands over.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream), as tools/bench_yuv_inputs.py builds it.  Sources at 720 x 1280: the synthetic RGB video of tools/bench_frame_inputs.py
and the NV12 video of tools/bench_yuv_inputs.py; at 1080 x 1920: the v210 surface of tools/bench_yuv_packed_inputs.py (one
case).  Cases (T0 frames decoded, frame cap): (1000, 224) and (512, 512).  Routes, alternating inside one process, device
events, --steps (>= 10) timed steps after --warmup rounds, for residence in (pinned, device):

  rgb_<residence>_interlaced    encode_frames(Interlaced(frames, "top", "cubic"))
  rgb_<residence>_rebuilt       encode_frames(the frames rebuilt beforehand by the same formula) - outputs asserted torch.equal
  nv12_<residence>_interlaced   encode_frames(Interlaced(NV12 surface, "top", "cubic"))
  nv12_<residence>_full         encode_frames(the full-height NV12 surface): the bytes and launches of a host-rebuilt NV12 video,
                                but another picture - the step's cost behind a1 follows the content, so this pair also
                                measures the difference of the two pictures
  nv12_<residence>_rebuilt_rgb  encode_frames(the RGB frames rebuilt beforehand from the NV12 top field): the same pixels as the
                                Interlaced NV12 route - outputs asserted torch.equal
  v210_<residence>_interlaced / _full   as nv12's at 1080 x 1920, first case only

Per route: ms per step (median, min, max), the funnel alone (pixels_from_frames of the kept frames: upload, conversion,
rebuild, resize - the part this section changes, whatever the content), bytes uploaded per step.  Per pair: interlaced minus
counterpart beside the counterpart's spread, the same for the funnel alone, and requirement 1 - the interlaced median lies at
or below the counterpart's maximum plus the launch for the kept frames.  The host rebuild a caller paid before the call: tests/interlace_cases.rebuild (numpy) per decoded frame, both
fills, timed on --host-frames frames.  Once: ONE tdc_field_to_frame launch over 224 fields of 360 x 1280, both fills, in the
16-byte form (dense, and strided inside interleaved frames), the 4-byte form and the byte form (the same picture at pointer
offsets 4 and 1), next to tdc_orient_frames's (0, False) plain copy of the same output in the same run (ms, GB/s counting the
bytes read and the bytes written), and requirement 2 - the widest form takes at most 1.5 times the copy's time.  The exit
status is 0 when the outputs agree; a requirement that is not met is reported, not failed.  Prints one JSON line; --out also
writes it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--source", default="720x1280")
    ap.add_argument("--v210-source", default="1080x1920", help="'' leaves the v210 row out")
    ap.add_argument("--cases", default="1000:224,512:512", help="T0:cap pairs")
    ap.add_argument("--host-frames", type=int, default=16, help="frames the host rebuild is timed on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_interlaced_inputs.py measures on a GPU; none is visible")
    import bench
    import interlace_cases as ic
    import tdc_video_amd  # noqa: F401
    from bench_frame_inputs import synth_frames
    from bench_yuv_inputs import synth_nv12
    from bench_yuv_packed_inputs import pack_surface, synth_422
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
    assert Hs % 4 == 0, "the 4:2:0 source splits into fields at H % 4 == 0"
    Interlaced, YuvFrames = preprocess.Interlaced, preprocess.YuvFrames
    FIELD, FILL = "top", "cubic"

    def timed_ms(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def median_ms(fn):
        ms = []
        for r in range(args.warmup + args.steps):
            t, _ = timed_ms(fn)
            if r >= args.warmup:
                ms.append(t)
        return statistics.median(ms), min(ms), max(ms)

    def pinned(t):
        p = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        p.copy_(t)
        return p

    # ---- the launch alone, once: 224 fields of Hs / 2 x Ws ------------------------------------------------------------------
    n, Hf = 224, Hs // 2
    woven = synth_frames(n, Hs, Ws, dev)
    field = woven[:, 0::2].contiguous()
    nb = field.numel()
    moved = 3 * nb                                                   # the field read once, the frame written
    room_in = torch.empty(nb + 16, device=dev, dtype=torch.uint8)
    room_out = torch.empty(2 * nb + 16, device=dev, dtype=torch.uint8)
    want = {f: ops.field_to_frame(field, 0, f) for f in ic.FILLS}
    for f in ic.FILLS:                                               # the device's bytes are the restatement's
        assert torch.equal(want[f][:2].cpu(), torch.from_numpy(ic.rebuild(field[:2].cpu().numpy(), 0, f))), f
    launch = {"fields": n, "field_shape": [Hf, Ws], "bytes_read_plus_written": moved, "forms": {}}
    for f in ic.FILLS:
        for form, off in (("16_byte", 0), ("4_byte", 4), ("byte", 1)):
            src = room_in[off:off + nb].view(n, Hf, Ws, 3)
            src.copy_(field)
            out = room_out[off:off + 2 * nb].view(n, Hs, Ws, 3)
            m, lo, hi = median_ms(lambda: ops.field_to_frame(src, 0, f, out=out))
            assert torch.equal(out, want[f]), (f, form)
            launch["forms"]["%s_%s" % (f, form)] = {"ms": round(m, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                                                    "gb_per_s": round(moved / (m * 1e-3) / 1e9, 1)}
        out = room_out[:2 * nb].view(n, Hs, Ws, 3)
        m, lo, hi = median_ms(lambda: ops.field_to_frame(woven[:, 0::2], 0, f, out=out))      # read where it lies: row stride 6 W
        assert torch.equal(out, want[f]), (f, "strided")
        launch["forms"]["%s_16_byte_strided" % f] = {"ms": round(m, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                                                     "gb_per_s": round(moved / (m * 1e-3) / 1e9, 1)}
    out = room_out[:2 * nb].view(n, Hs, Ws, 3)
    m, lo, hi = median_ms(lambda: ops.orient_frames(want[FILL], 0, 0, out=out))
    launch["copy"] = {"what": "tdc_orient_frames (0, False) of the same output", "ms": round(m, 4), "ms_min": round(lo, 4),
                      "ms_max": round(hi, 4), "bytes_read_plus_written": 4 * nb, "gb_per_s": round(4 * nb / (m * 1e-3) / 1e9, 1)}
    ratios = {f: round(launch["forms"][f + "_16_byte"]["ms"] / launch["copy"]["ms"], 3) for f in ic.FILLS}
    launch["requirement_2"] = {"what": "the 16-byte form takes at most 1.5 times the identity copy's time", "ratio": ratios,
                               "met": all(r <= 1.5 for r in ratios.values())}
    launch_ms = launch["forms"][FILL + "_16_byte"]["ms"]
    del woven, field, room_in, room_out, want, out, src
    torch.cuda.empty_cache()
    print("[bench_interlaced_inputs] launch alone done", file=sys.stderr, flush=True)

    results, same_all = [], True
    for ci, case in enumerate(args.cases.split(",")):
        T0, cap = (int(v) for v in case.split(":"))
        enc.two_streams = min(T0, cap) <= 128
        idx = encode.frame_indices(enc.cfg, T0, 64, cap)
        kept = len(idx)
        rgb = synth_frames(T0, Hs, Ws, dev)
        rebuilt = torch.empty_like(rgb)
        for s in range(0, T0, 64):
            ops.field_to_frame(rgb[s:s + 64, 0::2], 0, FILL, out=rebuilt[s:s + 64])
        y, uv = synth_nv12(T0, Hs, Ws, dev)

        # what a caller paid before the call: every decoded frame rebuilt on the host
        n_host = min(args.host_frames, T0)
        host = rgb[:n_host].cpu().numpy()
        host_ms = {}
        for f in ic.FILLS:
            t0 = time.perf_counter()
            made = [ic.rebuild(fr[0::2], 0, f) for fr in host]
            host_ms[f] = (time.perf_counter() - t0) * 1e3 / n_host
        assert torch.equal(torch.from_numpy(np.stack(made)), rebuilt[:n_host].cpu()), "the host rebuild differs"
        del host, made

        def nv12(a, b):
            return YuvFrames.nv12(a, b, matrix="bt709")

        # the RGB frames a host rebuilds from the NV12 top field: the same pixels as the Interlaced NV12 routes, so the same work
        # behind the funnel (the full-height NV12 surface is another picture, and the step's cost behind a1 follows the content)
        top = nv12(y, uv).field(0)
        top_rgb = torch.empty(top.shape, dtype=torch.uint8, device=dev)
        nv_rebuilt = torch.empty_like(rgb)
        for s in range(0, T0, 64):
            top[s:s + 64].to_rgb(list(top[s:s + 64].planes()), top_rgb[s:s + 64])
            ops.field_to_frame(top_rgb[s:s + 64], 0, FILL, out=nv_rebuilt[s:s + 64])
        del top, top_rgb
        y_p, uv_p = pinned(y), pinned(uv)
        sources = {"rgb_pinned_interlaced": Interlaced(pinned(rgb), FIELD, FILL), "rgb_pinned_rebuilt": pinned(rebuilt),
                   "rgb_device_interlaced": Interlaced(rgb, FIELD, FILL), "rgb_device_rebuilt": rebuilt,
                   "nv12_pinned_interlaced": Interlaced(nv12(y_p, uv_p), FIELD, FILL), "nv12_pinned_full": nv12(y_p, uv_p),
                   "nv12_pinned_rebuilt_rgb": pinned(nv_rebuilt),
                   "nv12_device_interlaced": Interlaced(nv12(y, uv), FIELD, FILL), "nv12_device_full": nv12(y, uv),
                   "nv12_device_rebuilt_rgb": nv_rebuilt}
        pairs_of = [("rgb_pinned", "rebuilt"), ("rgb_device", "rebuilt"), ("nv12_pinned", "full"), ("nv12_device", "full"),
                    ("nv12_pinned", "rebuilt_rgb"), ("nv12_device", "rebuilt_rgb")]
        if ci == 0 and args.v210_source:
            Hv, Wv = (int(v) for v in args.v210_source.split("x"))
            surf = pack_surface(*synth_422(T0, Hv, Wv, 10, dev), "v210", dev)
            surf_p = pinned(surf)
            sources.update({"v210_pinned_interlaced": Interlaced(YuvFrames.v210(surf_p, Wv, matrix="bt709"), FIELD, FILL),
                            "v210_pinned_full": YuvFrames.v210(surf_p, Wv, matrix="bt709"),
                            "v210_device_interlaced": Interlaced(YuvFrames.v210(surf, Wv, matrix="bt709"), FIELD, FILL),
                            "v210_device_full": YuvFrames.v210(surf, Wv, matrix="bt709")})
            pairs_of += [("v210_pinned", "full"), ("v210_device", "full")]
        torch.cuda.synchronize()
        ms = {k: [] for k in sources}
        outs, uploaded = {}, {}
        for r in range(args.warmup + args.steps):
            for name, src in sources.items():
                t, out = timed_ms(lambda: enc.encode_frames(src, 64, 64, prompt_ids, frame_cap=cap))
                outs[name] = out
                if r >= args.warmup:
                    ms[name].append(t)
                del out
            print("[bench_interlaced_inputs] T0=%d cap=%d round %d" % (T0, cap, r), file=sys.stderr, flush=True)
        same = all(torch.equal(outs[k], outs["rgb_device_rebuilt"]) for k in sources if k.startswith("rgb_"))
        same = same and all(torch.equal(outs[k], outs["nv12_device_rebuilt_rgb"]) for k in sources if k.startswith("nv12_") and not k.endswith("_full"))
        same_all = same_all and same
        outs.clear()
        # the funnel alone - upload, conversion, rebuild, resize of the kept frames: what this section changes, whatever the content
        front = {k: [] for k in sources}
        for r in range(args.warmup + args.steps):
            for name, src in sources.items():
                stats = {}
                t, px = timed_ms(lambda: enc.pixels_from_frames(src, idx, stats=stats))
                del px
                uploaded[name] = stats["bytes_uploaded"]
                if r >= args.warmup:
                    front[name].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        fmed = {k: statistics.median(v) for k, v in front.items()}
        pairs = {}
        for k, other in pairs_of:
            a, b = k + "_interlaced", k + "_" + other
            scale = (int(args.v210_source.split("x")[0]) * int(args.v210_source.split("x")[1])) / (Hs * Ws) if k.startswith("v210") else 1.0
            allowed = max(ms[b]) + launch_ms * kept / n * scale
            pairs[k + "_vs_" + other] = {"same_pixels": other != "full", "interlaced_minus_counterpart_ms": round(med[a] - med[b], 3),
                                         "counterpart_spread_ms": round(max(ms[b]) - min(ms[b]), 3),
                                         "launch_for_kept_frames_ms": round(launch_ms * kept / n * scale, 3),
                                         "requirement_1_met": med[a] <= allowed,
                                         "funnel_alone_interlaced_minus_counterpart_ms": round(fmed[a] - fmed[b], 3)}
        results.append({"source": args.source, "field": FIELD, "fill": FILL, "frames_in": T0, "frame_cap": cap, "frames_kept": kept,
                        "routes": {k: {"ms_per_step": round(med[k], 3), "ms_min": round(min(ms[k]), 3), "ms_max": round(max(ms[k]), 3),
                                       "funnel_alone_ms": round(fmed[k], 3), "bytes_uploaded": uploaded[k]} for k in sources},
                        "same_pixel_outputs_bit_equal": same, "pairs": pairs,
                        "host_rebuild": {"what": "tests/interlace_cases.rebuild (numpy) per decoded RGB frame", "frames_timed": n_host,
                                         "ms_per_frame": {f: round(v, 3) for f, v in host_ms.items()},
                                         "ms_whole_video": {f: round(v * T0, 1) for f, v in host_ms.items()}}})
        print("[bench_interlaced_inputs] T0=%d cap=%d done" % (T0, cap), file=sys.stderr, flush=True)
        del sources, rgb, rebuilt, nv_rebuilt, y, uv, y_p, uv_p
        torch.cuda.empty_cache()
    req1 = all(p["requirement_1_met"] for c in results for p in c["pairs"].values())
    res = {"tool": "bench_interlaced_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "frame_slab": enc.frame_slab, "steps": args.steps, "warmup": args.warmup, "launch_alone": launch, "cases": results,
           "requirement_1": {"what": "each Interlaced step's median lies at or below its counterpart's maximum plus the launch for the kept frames",
                             "met": req1,
                             "met_where_the_counterpart_holds_the_same_pixels": all(p["requirement_1_met"] for c in results
                                                                                    for p in c["pairs"].values() if p["same_pixels"])},
           "requirement_2": launch["requirement_2"], "outputs_bit_equal": same_all}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if same_all else 1)


if __name__ == "__main__":
    main()
