"""Throughput from tower-level features: "frames/s (C only)" beside "frames/s (V+C)" (DESIGN.md section 13).

One engine with bench.py's geometry and types (model_cfg, random_state_dict, synth_video; T = 512 frames, K = 144, H = 3584,
fp16 connector / Q-Former, bf16 towers, fp16 residual stream).  The video's tower features are exported once
(VideoEncoder.export_features); then, alternating inside one process, each step timed by device events after --warmup
untimed rounds:

  v_plus_c        encode_video(pixels)                 towers + a5 + connector + Q-Former + emission
  c_only          encode_features(set on the device)   the same behind the towers
  c_only_pinned   encode_features(set in pinned host memory): + the upload of the a1-kept rows' source tensors

Every c_only result is compared torch.equal with v_plus_c's (`c_only_equals_v_plus_c`).  One further c_only step runs under the launch profiler
(ops.profile_start / profile_stop: the GEMM, attention, LayerNorm and cross-attention launches) and one is timed on the host
clock alone, so the line says where a C-only step goes: per-kernel-class milliseconds, the largest single launch, the time the
host needs to enqueue a step, and `other_ms` = step - profiled kernels (host gaps, the a5 read, and the launches the profiler
does not record: gathers, pooling, cos-sim).  Prints one JSON line; --out also writes it to a file."""
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
    ap.add_argument("--steps", type=int, default=10, help="timed steps per variant (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_stage_c.py measures on a GPU; none is visible")
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops
    from tdc_video_amd.pipeline import VideoEncoder
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

    t0 = time.perf_counter()
    fs = enc.export_features(vs, vd, (384, 384))                  # includes the one-time signature of the tower weights
    torch.cuda.synchronize()
    export_s = time.perf_counter() - t0
    host_fs = fs.cpu()

    def v_plus_c(info=None):
        return enc.encode_video(vs, vd, (384, 384), budget_text_len=64, n_text_tokens=64, prompt_ids=prompt_ids, frame_cap=T,
                                info=info)

    def c_only(info=None, src=fs):
        return enc.encode_features(src, 64, 64, prompt_ids, frame_cap=T, info=info)

    variants = [("v_plus_c", v_plus_c), ("c_only", c_only), ("c_only_pinned", lambda: c_only(src=host_fs))]
    ms = {n: [] for n, _ in variants}
    outs, equal = {}, True
    for r in range(args.warmup + args.steps):
        for name, fn in variants:                                 # the variants alternate
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            outs[name] = fn()
            b.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                ms[name].append(a.elapsed_time(b))
        equal = equal and torch.equal(outs["c_only"], outs["v_plus_c"]) and torch.equal(outs["c_only_pinned"], outs["v_plus_c"])
    outs.clear()
    wi, gi = {}, {}
    v_plus_c(wi)
    c_only(gi)

    # one C-only step on the host clock: the enqueue (it ends behind the a5 read) and the whole step
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c_only()
    enqueue_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    # ... and one under the launch profiler (a run of its own: it brackets every recorded launch with events)
    ops.profile_start()
    c_only()
    torch.cuda.synchronize()
    recs = ops.profile_stop()
    kinds = {}
    for x in recs:
        k = kinds.setdefault(x["kind"], {"launches": 0, "ms": 0.0})
        k["launches"] += 1
        k["ms"] += x["ms"]
    top = max(recs, key=lambda x: x["ms"])
    kernel_ms = sum(x["ms"] for x in recs)

    def row(name):
        med = statistics.median(ms[name])
        return {"ms_per_step": round(med, 3), "frames_per_s": round(T / med * 1e3, 1), "ms_min": round(min(ms[name]), 3),
                "ms_max": round(max(ms[name]), 3)}
    c_ms = statistics.median(ms["c_only"])
    res = {"tool": "bench_stage_c", "device": torch.cuda.get_device_name(dev), "frames": T, "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16", "tdc_frame_cap": T,
                       "tdc_two_streams": bool(enc.two_streams)},
           "steps": args.steps, "warmup": args.warmup,
           "frames_per_s_v_plus_c": row("v_plus_c")["frames_per_s"], "frames_per_s_c_only": row("c_only")["frames_per_s"],
           "frames_per_s_c_only_pinned": row("c_only_pinned")["frames_per_s"],
           "v_plus_c": row("v_plus_c"), "c_only": row("c_only"), "c_only_pinned": row("c_only_pinned"),
           "c_only_equals_v_plus_c": equal, "info_equal": gi == wi, "n_visual": gi["n_visual"], "segments": len(gi["seg_indices"]),
           "refine_unavailable_pairs": gi.get("refine_unavailable_pairs", 0),
           "feature_set_gb": round(fs.nbytes / 1e9, 3), "export_s": round(export_s, 3),
           "c_only_profile": {"kernel_ms": {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(kinds.items())},
                              "kernel_ms_sum": round(kernel_ms, 3), "launches": len(recs),
                              "largest_launch": {"kind": top["kind"], "ms": round(top["ms"], 3), "M": top["M"], "N": top["N"],
                                                 "K": top["K"]},
                              "largest_kernel_class": max(kinds, key=lambda k: kinds[k]["ms"]),
                              "host_enqueue_ms": round(enqueue_ms, 3), "host_clock_step_ms": round(wall_ms, 3),
                              "other_ms": round(c_ms - kernel_ms, 3), "other_share": round((c_ms - kernel_ms) / c_ms, 3)}}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
