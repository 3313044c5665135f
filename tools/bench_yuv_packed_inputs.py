"""Encode from packed YUV frames measured, by the method of tools/bench_yuv_hibit_inputs.py: the planar
route of section 20 / 21 against the packed route on the same samples, by where the frames lie.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream).  Source: a synthetic 4:2:2 video of 720 x 1280, held once as planes (what a host would have to unpack to: yuv422p at
8 bits, yuv422p10le at 10) and once packed - YUY2 (8 bits, BT.601), Y210 (10 bits in the high bits of 16-bit words, random bits
below them, BT.2020), v210 (rows padded to 128 bytes, random bits 30-31, BT.2020) and v210 again with transfer="hlg".  Both
routes encode the same samples and their outputs are asserted torch.equal.  Cases (T0 frames decoded, frame cap): (1000, 224)
and (512, 512).  Routes, alternating inside one process, device events, --steps (>= 10) timed steps after --warmup rounds:

  planar_pinned   encode_frames from pinned host planes            packed_pinned   encode_frames from the pinned host surface
  planar_device   encode_frames from device-resident planes        packed_device   encode_frames from the device-resident surface

Per route: ms per step (median, min, max), bytes uploaded per step.  Per format and case: the conversion alone, ONE
tdc_yuv_packed_to_rgb launch over all kept frames (ms, bytes read + written per second) in the form the surface's alignment
selects and in the group form (the same surface one word off its 16-byte alignment), beside ONE tdc_yuv_to_rgb launch over the
same frames in planes in the same run (and, under hlg, ONE tdc_yuv_hdr_to_rgb launch), and

  spread_ms                          max - min of the planar route's timed steps in that run (per residence)
  packed_minus_planar_{pinned,device}   must not exceed spread_ms + the conversion's ms
  conversion tb_per_s                must be at least half of the planar tdc_yuv_to_rgb launch's in that run

v210 also times its 24-pixel units alone: the same surface taken 1272 pixels wide (1280 = 53 * 24 + 8: each row ends in two
units of one group).  The requirements are reported as booleans and make the exit status.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {"yuy2": ("yuyv", 8, "bt601", "sdr"), "y210": ("y210", 10, "bt2020", "sdr"), "v210": ("v210", 10, "bt2020", "sdr"),
         "v210_hlg": ("v210", 10, "bt2020", "hlg")}


def synth_422(T0, H, W, bits, dev, seed=0, scene_len=21):
    """deterministic 4:2:2 samples on `dev` as int16: y [T0, H, W], u, v [T0, H, W / 2] - a scene is a constant base plus
    per-frame noise"""
    import torch
    g = torch.Generator(device=dev)
    top = (1 << bits) - 1
    y = torch.empty(T0, H, W, device=dev, dtype=torch.int16)
    u = torch.empty(T0, H, W // 2, device=dev, dtype=torch.int16)
    v = torch.empty(T0, H, W // 2, device=dev, dtype=torch.int16)
    for t in range(T0):
        if t % scene_len == 0:
            g.manual_seed(seed * 7919 + t // scene_len)
            by = torch.randint(0, top + 1, (H, W), device=dev, generator=g, dtype=torch.int32)
            bu = torch.randint(0, top + 1, (H, W // 2), device=dev, generator=g, dtype=torch.int32)
            bv = torch.randint(0, top + 1, (H, W // 2), device=dev, generator=g, dtype=torch.int32)
        g.manual_seed(seed * 104729 + 1000003 + t)
        a = top // 21
        y[t] = (by + torch.randint(-a, a + 1, (H, W), device=dev, generator=g, dtype=torch.int32)).clamp_(0, top)
        u[t] = (bu + torch.randint(-a // 2, a // 2 + 1, (H, W // 2), device=dev, generator=g, dtype=torch.int32)).clamp_(0, top)
        v[t] = (bv + torch.randint(-a // 2, a // 2 + 1, (H, W // 2), device=dev, generator=g, dtype=torch.int32)).clamp_(0, top)
    return y, u, v


def as_int16(w):
    import torch
    return torch.where(w >= 32768, w - 65536, w).to(torch.int16)


def as_int32(w):
    import torch
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def pack_surface(y, u, v, fmt, dev, seed=1):
    """the samples packed on the device -> the whole-pitch surface [T0, H, pitch words] (include/tdc_hip.h states the layouts)"""
    import torch
    T0, H, W = y.shape
    g = torch.Generator(device=dev).manual_seed(seed)
    if fmt == "yuyv":
        out = torch.empty(T0, H, W // 2, 4, device=dev, dtype=torch.uint8)
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = y[:, :, 0::2], u, y[:, :, 1::2], v
        return out.view(T0, H, 2 * W)
    if fmt == "y210":
        out = torch.empty(T0, H, W // 2, 4, device=dev, dtype=torch.int16)
        for t in range(T0):                                       # frame by frame: the temporaries stay small
            for k, s in enumerate((y[t, :, 0::2], u[t], y[t, :, 1::2], v[t])):
                out[t, :, :, k] = as_int16((s.to(torch.int32) << 6) | torch.randint(0, 64, s.shape, device=dev, generator=g, dtype=torch.int32))
        return out.view(T0, H, 2 * W)
    ng = -(-W // 6)
    pitch = (ng * 16 + 127) // 128 * 128 // 4                     # v210's conventional 128-byte row alignment
    out = torch.zeros(T0, H, pitch, device=dev, dtype=torch.int32)
    for t in range(T0):
        Y = torch.zeros(H, ng * 6, device=dev, dtype=torch.int64)
        U = torch.zeros(H, ng * 3, device=dev, dtype=torch.int64)
        V = torch.zeros(H, ng * 3, device=dev, dtype=torch.int64)
        Y[:, :W], U[:, :W // 2], V[:, :W // 2] = y[t], u[t], v[t]
        Y, U, V = Y.view(H, ng, 6), U.view(H, ng, 3), V.view(H, ng, 3)
        words = torch.stack([U[..., 0] | Y[..., 0] << 10 | V[..., 0] << 20, Y[..., 1] | U[..., 1] << 10 | Y[..., 2] << 20,
                             V[..., 1] | Y[..., 3] << 10 | U[..., 2] << 20, Y[..., 4] | V[..., 2] << 10 | Y[..., 5] << 20], -1)
        words = words | torch.randint(0, 4, words.shape, device=dev, generator=g, dtype=torch.int64) << 30
        out[t, :, :ng * 4] = as_int32(words.view(H, ng * 4))
    return out


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
        sys.exit("bench_yuv_packed_inputs.py measures on a GPU; none is visible")
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
        fmt, bits, matrix, transfer = KINDS[kind]
        ws = ops.YUV_PACKED[fmt][0]
        row_bytes = ops.yuv_packed_words(fmt, Ws) * ws
        bs = 1 if bits == 8 else 2
        coef = preprocess.yuv_coefficients(matrix, False, bits)

        def packed(data, W=Ws):
            return preprocess.YuvFrames.packed(data, fmt, width=W, matrix=matrix, transfer=transfer)

        def planar(y, u, v):
            return preprocess.YuvFrames.i420(y, u, v, bits=bits, subsampling="422", matrix=matrix, transfer=transfer)

        for case in args.cases.split(","):
            T0, cap = (int(v) for v in case.split(":"))
            enc.two_streams = min(T0, cap) <= 128
            y, u, v = synth_422(T0, Hs, Ws, bits, dev)
            surface = pack_surface(y, u, v, fmt, dev)
            if bits == 8:
                y, u, v = y.to(torch.uint8), u.to(torch.uint8), v.to(torch.uint8)
            sources = {"planar_pinned": planar(pinned(y), pinned(u), pinned(v)), "packed_pinned": packed(pinned(surface)),
                       "planar_device": planar(y, u, v), "packed_device": packed(surface)}
            torch.cuda.synchronize()
            idx = encode.frame_indices(enc.cfg, T0, 64, cap)
            kept = len(idx)
            uploaded = {"planar_pinned": kept * 2 * px * bs, "packed_pinned": kept * Hs * row_bytes, "planar_device": 0, "packed_device": 0}
            ms = {n: [] for n in sources}
            outs = {}
            for r in range(args.warmup + args.steps):
                for name, src in sources.items():
                    t, out = timed_ms(lambda: enc.encode_frames(src, 64, 64, prompt_ids, frame_cap=cap))
                    outs[name] = out
                    if r >= args.warmup:
                        ms[name].append(t)
                    del out
            same = all(torch.equal(outs[n], outs["planar_device"]) for n in sources)
            assert same, "the routes' outputs differ"
            outs.clear()
            for name in ("planar_pinned", "packed_pinned"):       # the upload as the product counts it
                stats = {}
                enc.pixels_from_frames(sources[name], idx, stats=stats)
                assert stats["bytes_uploaded"] == uploaded[name], (name, stats)
            del sources
            # the conversion launches alone, on the kept frames: the selected form, the group form, the planar launch(es)
            sel = torch.tensor(idx, device=dev)
            ky, ku, kv = y[sel], u[sel], v[sel]
            on16 = surface[sel]
            off16 = torch.empty((on16.numel() + 1,), device=dev, dtype=surface.dtype)[1:].view(on16.shape)      # one word off: the group form
            off16.copy_(on16)
            scratch = torch.empty(kept, Hs, Ws, 3, device=dev, dtype=torch.uint8)
            f = packed(on16)
            hdr = None if f.hdr is None else dict(f.hdr, lut=preprocess.hdr_lut(transfer, bits, f.peak_nits, f.sdr_white, dev))
            launches = {"selected": lambda: ops.yuv_packed_to_rgb(on16, fmt, f.coef, Hs, Ws, bits, f.msb_aligned, hdr=hdr, out=scratch),
                        "group": lambda: ops.yuv_packed_to_rgb(off16, fmt, f.coef, Hs, Ws, bits, f.msb_aligned, hdr=hdr, out=scratch),
                        "planar": lambda: ops.yuv_to_rgb(ky, ku, kv, 1, coef, Hs, Ws, bits, False, "422", out=scratch)}
            if fmt == "v210":
                launches["vec24_1272_wide"] = lambda: ops.yuv_packed_to_rgb(on16, fmt, f.coef, Hs, 1272, bits, False, hdr=hdr,
                                                                            out=scratch.view(-1)[:kept * Hs * 1272 * 3].view(kept, Hs, 1272, 3))
            if hdr is not None:
                launches["planar_hdr"] = lambda: ops.yuv_hdr_to_rgb(ky, ku, kv, 1, f.coef, Hs, Ws, bits, False, "422", hdr, out=scratch)
            launches["selected"]()
            want = scratch.clone()
            launches["group"]()
            assert torch.equal(scratch, want), "the forms' bytes differ"
            launches["planar_hdr" if hdr is not None else "planar"]()
            assert torch.equal(scratch, want), "the packed and the planar launch differ"
            del want
            lms = {n: [] for n in launches}
            for r in range(args.warmup + args.steps):
                for n, fn in launches.items():
                    t, _ = timed_ms(fn)
                    if r >= args.warmup:
                        lms[n].append(t)
            del ky, ku, kv, on16, off16, scratch
            moved = {"selected": kept * (Hs * row_bytes + 3 * px), "group": kept * (Hs * row_bytes + 3 * px),
                     "planar": kept * (2 * px * bs + 3 * px), "planar_hdr": kept * (2 * px * bs + 3 * px),
                     "vec24_1272_wide": kept * Hs * (1272 // 6 * 16 + 3 * 1272)}
            conv = {n: {"ms": round(statistics.median(v_), 4), "bytes_moved": moved[n],
                        "tb_per_s": round(moved[n] / (statistics.median(v_) * 1e-3) / 1e12, 3)} for n, v_ in lms.items()}
            conv_ms = statistics.median(lms["selected"])
            med = {n: statistics.median(v_) for n, v_ in ms.items()}
            spread = {k: max(ms["planar_" + k]) - min(ms["planar_" + k]) for k in ("pinned", "device")}
            d_pin, d_dev = med["packed_pinned"] - med["planar_pinned"], med["packed_device"] - med["planar_device"]
            pin_ok, dev_ok = d_pin <= spread["pinned"] + conv_ms, d_dev <= spread["device"] + conv_ms
            rate_ok = conv["selected"]["tb_per_s"] >= 0.5 * conv["planar"]["tb_per_s"]
            group_ok = conv["group"]["tb_per_s"] >= 0.5 * conv["planar"]["tb_per_s"]
            ok = ok and pin_ok and dev_ok and rate_ok and group_ok
            results.append({"kind": kind, "format": fmt, "bits": bits, "matrix": matrix, "transfer": transfer, "source": args.source,
                            "frames_in": T0, "frame_cap": cap, "frames_kept": kept,
                            "routes": {n: {"ms_per_step": round(med[n], 3), "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3),
                                           "bytes_uploaded": uploaded[n]} for n in ms},
                            "outputs_bit_equal": same, "conversion": conv,
                            "spread_ms": {k: round(v_, 3) for k, v_ in spread.items()},
                            "packed_minus_planar_pinned_ms": round(d_pin, 3), "packed_minus_planar_device_ms": round(d_dev, 3),
                            "pinned_within_spread_plus_conversion": pin_ok, "device_within_spread_plus_conversion": dev_ok,
                            "selected_form_at_least_half_the_planar_rate": rate_ok, "group_form_at_least_half_the_planar_rate": group_ok})
            print("[bench_yuv_packed_inputs] %s T0=%d cap=%d done" % (kind, T0, cap), file=sys.stderr, flush=True)
            del y, u, v, surface
            torch.cuda.empty_cache()
    res = {"tool": "bench_yuv_packed_inputs", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
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
