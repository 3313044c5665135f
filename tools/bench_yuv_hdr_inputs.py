"""Encode from HDR P010 frames measured, by the method of tools/bench_yuv_hibit_inputs.py: the RGB frames
route of section 15 and the SDR P010 route of section 20 against the HDR P010 route (transfer="pq") on the same planes, by
where the frames lie.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream).  Source: the synthetic P010 video of bench_yuv_hibit_inputs (720 x 1280, BT.2020 limited, random bits below the
samples) read as PQ; the RGB route gets the uint8 frames tdc_yuv_hdr_to_rgb makes of it, so the RGB and the HDR route encode
the same pixels and their outputs are asserted torch.equal (the SDR route encodes other pixels: it is there for its time).
Cases (T0 frames decoded, frame cap): (1000, 224) and (512, 512).  Routes, alternating inside one process, device events,
--steps (>= 10) timed steps after --warmup rounds: rgb, sdr (P010, tdc_yuv_to_rgb) and hdr (P010, tdc_yuv_hdr_to_rgb), each
from pinned host memory and device-resident.

Per route: ms per step (median, min, max).  Per case: ONE tdc_yuv_hdr_to_rgb launch over all kept frames (ms, bytes per second
at 6 bytes in and 3 out per 4:4:4-equivalent pixel, i.e. 6 per pixel at 4:2:0), beside ONE tdc_yuv_to_rgb launch and the resize
of the same frames in the same run, their ratio, and

  spread_ms                      max - min of the RGB route's timed steps in that run (per residence)
  hdr_minus_rgb_{pinned,device}  must not exceed spread_ms + the HDR conversion's ms
  hdr conversion ms              must be below the resize's ms

--cpu-frames N (default 2) also times the definition in numpy on N host frames (stage A in integers, stage B in float64, as
a caller without this entry would have to for all T0 frames), checks it against the kernel (every byte within 1) and reports
ms per frame and the differing share.  The requirements are reported as booleans and make the exit status.  Prints one JSON
line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def cpu_definition(y, uv, coef, table, hdr, n):
    """the definition in numpy on n host frames of P010 -> (ms per frame, rgb uint8 [n, H, W, 3])"""
    import numpy as np
    yw, cw = y[:n].cpu().numpy().view(np.uint16), uv[:n].cpu().numpy().view(np.uint16)
    y_off, ky, krv, kgu, kgv, kbu = (int(c) for c in coef)
    t0 = time.perf_counter()
    Y = ((yw >> 6) & 1023).astype(np.int64)
    U = np.repeat(np.repeat(((cw[:, :, 0::2] >> 6) & 1023).astype(np.int64) - 512, 2, axis=1), 2, axis=2)
    V = np.repeat(np.repeat(((cw[:, :, 1::2] >> 6) & 1023).astype(np.int64) - 512, 2, axis=1), 2, axis=2)
    yy = ky * (Y - y_off) + 32768
    lut = table.astype(np.float64)
    l = np.stack([lut[np.clip(a >> 16, 0, 1023)] for a in (yy + krv * V, yy - kgu * U - kgv * V, yy + kbu * U)])
    if hdr["ootf_exp"] != 0.0:
        ys = sum(w * c for w, c in zip(hdr["luma"], l))
        l = l * np.where(ys > 0, hdr["ootf_scale"] * np.maximum(ys, 1e-300) ** hdr["ootf_exp"], 0.0)
    m = l.max(axis=0)
    l = l * ((1.0 + m * hdr["inv_p2"]) / (1.0 + m))
    x = np.clip(np.tensordot(np.asarray(hdr["gamut"], np.float64).reshape(3, 3), l, axes=1), 0.0, 1.0)
    v = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.maximum(x, 1e-300) ** (1.0 / 2.4) - 0.055)
    rgb = np.moveaxis(np.floor(255.0 * v + 0.5), 0, -1).astype(np.uint8)
    return (time.perf_counter() - t0) * 1e3 / n, rgb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--source", default="720x1280")
    ap.add_argument("--cases", default="1000:224,512:512", help="T0:cap pairs")
    ap.add_argument("--transfer", default="pq", choices=("pq", "hlg"))
    ap.add_argument("--cpu-frames", type=int, default=2, help="frames of the definition computed on the host (0: skip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_hdr_inputs.py measures on a GPU; none is visible")
    import numpy as np
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
    coef_sdr = preprocess.yuv_coefficients("bt2020", False, 10)

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

    def p010(y, uv, transfer):
        return preprocess.YuvFrames.p010(y, uv, matrix="bt2020", transfer=transfer)

    results, ok, cpu = [], True, None
    for case in args.cases.split(","):
        T0, cap = (int(v) for v in case.split(":"))
        enc.two_streams = min(T0, cap) <= 128
        y, uv = synth_p010(T0, Hs, Ws, dev)
        hdr_frames = p010(y, uv, args.transfer)
        hdr = dict(hdr_frames.hdr, lut=preprocess.hdr_lut(args.transfer, 10, hdr_frames.peak_nits, hdr_frames.sdr_white, dev))
        coef = hdr_frames.coef

        def hdr_launch(yy, cc, out=None):
            return ops.yuv_hdr_to_rgb(yy, cc, cc[:, :, 1:], 2, coef, Hs, Ws, 10, True, "420", hdr, out=out)

        rgb = hdr_launch(y, uv)
        if args.cpu_frames and cpu is None:
            table = preprocess.hdr_table(args.transfer, 10, hdr_frames.peak_nits, hdr_frames.sdr_white)[0]
            ms_frame, host_rgb = cpu_definition(y, uv, coef, table, hdr_frames.hdr, min(args.cpu_frames, T0))
            diff = np.abs(host_rgb.astype(np.int16) - rgb[:host_rgb.shape[0]].cpu().numpy().astype(np.int16))
            assert int(diff.max()) <= 1, "the kernel is more than 1 from the definition"
            cpu = {"frames_timed": int(host_rgb.shape[0]), "ms_per_frame": round(ms_frame, 2), "threads": torch.get_num_threads(),
                   "kernel_largest_difference": int(diff.max()), "kernel_differing_share": float((diff != 0).mean())}
            del host_rgb, diff
        py, puv = pinned(y), pinned(uv)
        sources = {"rgb_pinned": pinned(rgb), "sdr_pinned": p010(py, puv, "sdr"), "hdr_pinned": p010(py, puv, args.transfer),
                   "rgb_device": rgb, "sdr_device": p010(y, uv, "sdr"), "hdr_device": hdr_frames}
        torch.cuda.synchronize()
        idx = encode.frame_indices(enc.cfg, T0, 64, cap)
        kept = len(idx)
        px = Hs * Ws
        ms = {n: [] for n in sources}
        outs = {}
        for r in range(args.warmup + args.steps):
            for name, src in sources.items():
                t, out = timed_ms(lambda: enc.encode_frames(src, 64, 64, prompt_ids, frame_cap=cap))
                outs[name] = out
                if r >= args.warmup:
                    ms[name].append(t)
                del out
        same = all(torch.equal(outs[n], outs["rgb_device"]) for n in ("rgb_pinned", "hdr_pinned", "hdr_device"))
        assert same, "the RGB and HDR routes' outputs differ"
        outs.clear()
        # the two conversion launches alone and the resize of the same frames
        sel = torch.tensor(idx, device=dev)
        ky, kuv = y[sel], uv[sel]
        scratch = torch.empty(kept, Hs, Ws, 3, device=dev, dtype=torch.uint8)
        conv, conv_sdr, resize = [], [], []
        for r in range(args.warmup + args.steps):
            t, _ = timed_ms(lambda: hdr_launch(ky, kuv, scratch))
            t1, _ = timed_ms(lambda: ops.yuv_to_rgb(ky, kuv, kuv[:, :, 1:], 2, coef_sdr, Hs, Ws, 10, True, "420", out=scratch))
            t2, pxs = timed_ms(lambda: enc.pixels_from_frames(rgb, idx))
            del pxs
            if r >= args.warmup:
                conv.append(t)
                conv_sdr.append(t1)
                resize.append(t2)
        del ky, kuv, scratch
        conv_ms, sdr_ms, resize_ms = statistics.median(conv), statistics.median(conv_sdr), statistics.median(resize)
        med = {n: statistics.median(v) for n, v in ms.items()}
        spread = {k: max(ms["rgb_" + k]) - min(ms["rgb_" + k]) for k in ("pinned", "device")}
        d_pin, d_dev = med["hdr_pinned"] - med["rgb_pinned"], med["hdr_device"] - med["rgb_device"]
        pin_ok, dev_ok = d_pin <= spread["pinned"] + conv_ms, d_dev <= spread["device"] + conv_ms
        launch_ok = conv_ms < resize_ms
        ok = ok and pin_ok and dev_ok and launch_ok
        results.append({"source": args.source, "frames_in": T0, "frame_cap": cap, "frames_kept": kept,
                        "routes": {n: {"ms_per_step": round(med[n], 3), "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3)}
                                   for n in sources},
                        "rgb_and_hdr_outputs_bit_equal": same,
                        "hdr_conversion": {"ms": round(conv_ms, 4), "bytes_moved": kept * px * 6,
                                           "tb_per_s": round(kept * px * 6 / (conv_ms * 1e-3) / 1e12, 3), "launches": 1},
                        "sdr_conversion_same_run": {"ms": round(sdr_ms, 4), "tb_per_s": round(kept * px * 6 / (sdr_ms * 1e-3) / 1e12, 3)},
                        "hdr_over_sdr_conversion": round(conv_ms / sdr_ms, 3),
                        "resize_same_frames_ms": round(resize_ms, 3),
                        "spread_ms": {k: round(v, 3) for k, v in spread.items()},
                        "hdr_minus_rgb_pinned_ms": round(d_pin, 3), "hdr_minus_rgb_device_ms": round(d_dev, 3),
                        "hdr_minus_sdr_pinned_ms": round(med["hdr_pinned"] - med["sdr_pinned"], 3),
                        "hdr_minus_sdr_device_ms": round(med["hdr_device"] - med["sdr_device"], 3),
                        "pinned_within_spread_plus_conversion": pin_ok, "device_within_spread_plus_conversion": dev_ok,
                        "conversion_below_the_resize": launch_ok})
        print("[bench_yuv_hdr_inputs] T0=%d cap=%d done" % (T0, cap), file=sys.stderr, flush=True)
        del sources, y, uv, py, puv, rgb, hdr_frames
        torch.cuda.empty_cache()
    res = {"tool": "bench_yuv_hdr_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "layout": "p010", "matrix": "bt2020", "full_range": False, "transfer": args.transfer, "peak_nits": 1000.0,
           "sdr_white": 203.0, "frame_slab": enc.frame_slab, "steps": args.steps, "warmup": args.warmup,
           "host_definition_numpy": cpu, "cases": results, "requirements_met": ok}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
