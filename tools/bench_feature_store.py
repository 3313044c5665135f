"""The compact feature store measured: lossless (16-bit rows) against compact (e4m3 rows + fp32 row
scales + the stored a5 similarities), each device-resident and in pinned host memory.

One engine with bench.py's geometry and types (T = 512 frames, K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16
residual stream), as tools/bench_stage_c.py builds it.  Reported:

  bytes           per video, both stores
  export / compact  seconds of export_features (lossless, and store="e4m3") and milliseconds of compact_features (device events)
  gather          the decode launch of tdc_gather_rows over all T * P rows of each tower into [T * P, pad64(D)] - with 16-byte
                  loads (row stride D) and with 8-byte loads (the same bytes at row stride D + 8, which rules the 16-byte form
                  out) - as GB/s over 3 x T x P x D bytes (1 read, 2 written), beside the 16-bit form of the same launch at the
                  same shape (4 x T x P x D bytes)
  encode          encode_features frames/s of the four cases, alternating inside one process, device events, --steps (>= 10)
                  timed steps after --warmup rounds
  parity          compact against lossless at full width: the selection, the worst error of the unit-norm compressed rows
                  (absolute) and of the static rows (relative to max|ref|)

Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per case (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_feature_store.py measures on a GPU; none is visible")
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import encode, ops
    from tdc_video_amd.pipeline import VideoEncoder
    from tdc_video_amd.weights import pad64
    dev = torch.device("cuda", 0)
    T, K, H = args.frames, args.K, args.hidden
    gen = torch.Generator(device=dev).manual_seed(0)
    sd = bench.random_state_dict(H, K, dev, gen)
    enc = VideoEncoder(sd, bench.model_cfg(H, K, T), dtype=torch.float16, device=dev, tower_batch=512,
                       tower_dtype=torch.bfloat16, tower_res_dtype=torch.float16)
    enc.two_streams = T <= 128
    del sd
    torch.cuda.empty_cache()
    vs = bench.synth_video(0, T, 384, dev, torch.bfloat16)
    vd = bench.synth_video(0, T, 378, dev, torch.bfloat16, seed=4321)
    prompt_ids = [101] + list(range(2000, 2010)) + [102]

    def timed_ms(fn, reps=1):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps, out

    enc.feature_signature()                                       # the one-time fingerprint of the tower weights: not an export cost
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fs = enc.export_features(vs, vd, (384, 384))
    torch.cuda.synchronize()
    export_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    cs_direct = enc.export_features(vs, vd, (384, 384), store="e4m3")
    torch.cuda.synchronize()
    export_compact_s = time.perf_counter() - t0
    enc.compact_features(fs)                                      # warm-up: allocations
    compact_ms, cs = timed_ms(lambda: enc.compact_features(fs))
    same_bytes = all(torch.equal(getattr(cs_direct, k), t) for k, t in cs.tensors().items())
    del cs_direct, vs, vd
    torch.cuda.empty_cache()
    P = fs.siglip.shape[1]

    # ---- the gather launch alone, per tower
    gather = {}
    n = T * P
    src = np.zeros((n, 2), dtype=np.int32)
    src[:, 1] = np.arange(n)
    src = torch.from_numpy(src).to(dev)
    for name, x8, sc, x16 in (("siglip", cs.siglip, cs.siglip_scale, fs.siglip), ("dino", cs.dino, cs.dino_scale, fs.dino)):
        D = x8.shape[2]
        out = torch.zeros(n, pad64(D), device=dev, dtype=enc.dtype)
        t8, s1, t16 = x8.view(n, D), sc.view(n), x16.view(n, D)
        wide = torch.zeros(n, D + 8, device=dev, dtype=torch.uint8)
        wide[:, :D] = t8
        forms = {"decode_16_byte_loads": lambda: ops.gather_rows([t8], src, n, D, out=out, validated=True, scales=[s1], dtype=enc.dtype),
                 "decode_8_byte_loads": lambda: ops.gather_rows([wide[:, :D]], src, n, D, out=out, validated=True, scales=[s1],
                                                                dtype=enc.dtype),
                 "copy_16_bit": lambda: ops.gather_rows([t16], src, n, D, out=out, validated=True)}
        row = {"D": D, "rows": n}
        for form, fn in forms.items():
            fn()
            ms = [timed_ms(fn)[0] for _ in range(20)]
            nbytes = (4 if form == "copy_16_bit" else 3) * n * D
            row[form] = {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                         "gb_per_s": round(nbytes / statistics.median(ms) / 1e6, 1)}
        gather[name] = row
        del out, wide
    torch.cuda.empty_cache()

    # ---- encode_features, the four cases alternating
    cases = [("lossless_device", fs), ("compact_device", cs), ("lossless_pinned", fs.cpu()), ("compact_pinned", cs.cpu())]
    ms = {c: [] for c, _ in cases}
    outs, infos = {}, {}
    for r in range(args.warmup + args.steps):
        for name, s in cases:
            info = {}
            t, outs[name] = timed_ms(lambda: enc.encode_features(s, 64, 64, prompt_ids, frame_cap=T, info=info))
            infos[name] = info
            if r >= args.warmup:
                ms[name].append(t)

    def row(name):
        med = statistics.median(ms[name])
        return {"ms_per_step": round(med, 3), "frames_per_s": round(T / med * 1e3, 1), "ms_min": round(min(ms[name]), 3),
                "ms_max": round(max(ms[name]), 3)}

    # ---- parity at full width: compact against lossless
    want, got = outs["lossless_device"], outs["compact_device"]
    wi, gi = infos["lossless_device"], infos["compact_device"]
    h, w = wi["final_size"][0]
    plan, _ = encode.emission_plan(enc, len(wi["frame_indices"]), h * (w + 1), wi["seg_indices"], encode.visual_budget(enc.cfg, 64))
    kinds = torch.from_numpy(np.asarray(plan.kind)).to(dev)
    parity = {"selection_equal": gi["seg_indices"] == wi["seg_indices"], "selection_sims": gi.get("selection_sims"),
              "shapes_equal": tuple(got.shape) == tuple(want.shape), "segments": len(gi["seg_indices"]),
              "pinned_equals_device": bool(torch.equal(outs["compact_pinned"], got)) and
              bool(torch.equal(outs["lossless_pinned"], want))}
    if parity["shapes_equal"] and kinds.numel() == want.shape[0]:
        d = (got.float() - want.float()).abs()
        comp, stat = kinds == 1, kinds == 0
        parity.update(compressed_rows=int(comp.sum()), static_rows=int(stat.sum()),
                      compressed_max_abs=float(d[comp].max()) if bool(comp.any()) else None,
                      static_max_rel=float(d[stat].max() / want[stat].float().abs().max()) if bool(stat.any()) else None,
                      static_rms_rel=float(d[stat].pow(2).mean().sqrt() / want[stat].float().pow(2).mean().sqrt())
                      if bool(stat.any()) else None)
    lo, co = statistics.median(ms["lossless_device"]), statistics.median(ms["compact_device"])
    decode_ms = gather["siglip"]["decode_16_byte_loads"]["ms"] + gather["dino"]["decode_16_byte_loads"]["ms"]
    res = {"tool": "bench_feature_store", "device": torch.cuda.get_device_name(dev), "frames": T, "K": K, "H": H, "tokens": P,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16", "tdc_frame_cap": T},
           "steps": args.steps, "warmup": args.warmup,
           "bytes_per_video": {"lossless": fs.nbytes, "compact": cs.nbytes, "ratio": round(cs.nbytes / fs.nbytes, 4)},
           "export_s": {"lossless": round(export_s, 3), "e4m3": round(export_compact_s, 3)},
           "compact_features_ms": round(compact_ms, 3), "export_e4m3_bytes_equal_compact_features": same_bytes,
           "gather": gather, "decode_launches_ms": round(decode_ms, 4),
           "encode_features": {c: row(c) for c, _ in cases},
           "compact_minus_lossless_device_ms": round(co - lo, 3),
           "pinned_speedup": round(statistics.median(ms["lossless_pinned"]) / statistics.median(ms["compact_pinned"]), 3),
           "parity": parity}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
