"""What the frame cache (tdc-video_amd/cache.py, encode_video(cache=...)) saves at the bench geometry: bench.py's engine and
video (model_cfg, random_state_dict, synth_video; T = 512, K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16
residual stream), timed with device events after warm-up, median of --reps:

  a  fresh encode, cache off (bench.py's step)
  b  first call with the cache on: every frame a miss (a new cache each repetition)
  c  a second question on the same video (other prompt_ids and n_text_tokens): every frame a hit
  d  the LVCoT pattern (eval/cot.py): each half of the video, then the whole video (a new cache each repetition)
  e  tdc_fingerprint_rows alone over the a1-selected frames of both pixel tensors: ms and bytes/s against 8 TB/s

Every cached result is checked torch.equal against the fresh one.  Prints one JSON object; --out writes it too.
Kernel summary of the cache-hit calls alone: `--legs c --mark-region` brackets leg c's timed calls with two short marker
kernels (torch.cuda._sleep); run that under `rocprofv3 --kernel-trace --output-format csv`, then
`--region-stats <kernel_trace.csv> <out.csv>` writes per-kernel calls / total / average / share of the dispatches between the
markers."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def timed(fn, reps, setup=None):
    """median device ms and host ms of fn() over reps calls (setup() before each, untimed)"""
    dev_ms, host_ms, out = [], [], None
    for _ in range(reps):
        if setup is not None:
            setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(a.elapsed_time(b))
    return round(statistics.median(dev_ms), 3), round(statistics.median(host_ms), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cache-bytes", type=int, default=4 << 30)
    ap.add_argument("--legs", default="abcde")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mark-region", action="store_true", help="marker kernels around leg c's timed calls")
    ap.add_argument("--region-stats", nargs=2, metavar=("TRACE_CSV", "OUT_CSV"), help="summarise a kernel trace between the markers")
    args = ap.parse_args()
    if args.region_stats:
        return region_stats(*args.region_stats)
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops
    from tdc_video_amd.pipeline import VideoEncoder, frame_indices
    dev = torch.device("cuda", 0)
    T, H, K = args.frames, 3584, 144
    gen = torch.Generator(device=dev).manual_seed(0)
    sd = bench.random_state_dict(H, K, dev, gen)
    enc = VideoEncoder(sd, bench.model_cfg(H, K, T), dtype=torch.float16, device=dev, tower_dtype=torch.bfloat16,
                       tower_res_dtype=torch.float16)
    enc.two_streams = T <= 128                                          # bench.py's default
    del sd
    torch.cuda.empty_cache()
    vs = bench.synth_video(0, T, 384, dev, torch.bfloat16)
    vd = bench.synth_video(0, T, 378, dev, torch.bfloat16, seed=4321)
    q1 = [101] + list(range(2000, 2010)) + [102]
    q2 = [101, 3000, 3001, 3002, 3003, 102]

    def call(s, d, prompt=q1, n_text=64, cache=None):
        return enc.encode_video(s, d, (384, 384), budget_text_len=64, n_text_tokens=n_text, prompt_ids=prompt, frame_cap=T,
                                cache=cache)

    res = {"frames": T, "cache_bytes": args.cache_bytes, "reps": args.reps}
    for _ in range(args.warmup):
        want1 = call(vs, vd)
    want2 = call(vs, vd, q2, 40)
    torch.cuda.synchronize()
    box = {}

    def fresh_cache():
        box["c"] = enc.new_cache(args.cache_bytes)

    if "a" in args.legs:
        res["a_fresh_ms"], res["a_fresh_host_ms"], _ = timed(lambda: call(vs, vd), args.reps)
    if "b" in args.legs:
        for _ in range(args.warmup):
            fresh_cache()
            call(vs, vd, cache=box["c"])
        res["b_first_ms"], res["b_first_host_ms"], got = timed(lambda: call(vs, vd, cache=box["c"]), args.reps, fresh_cache)
        assert torch.equal(got, want1), "cached first call differs from the fresh encode"
        st = box["c"].stats()
        res["cache_after_b"] = {k: st[k] for k in ("frames", "bytes", "reserved_bytes", "frames_encoded")}
    if "c" in args.legs:
        c = enc.new_cache(args.cache_bytes)
        call(vs, vd, cache=c)
        for _ in range(args.warmup):
            call(vs, vd, q2, 40, cache=c)
        info = {}
        if args.mark_region:
            torch.cuda._sleep(1000)
        res["c_hit_ms"], res["c_hit_host_ms"], got = timed(lambda: enc.encode_video(
            vs, vd, (384, 384), budget_text_len=64, n_text_tokens=40, prompt_ids=q2, frame_cap=T, cache=c, info=info),
            args.reps)
        if args.mark_region:
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
        assert torch.equal(got, want2), "cached second question differs from the fresh encode"
        res["c_info"] = info["cache"]
        if "a_fresh_ms" in res:
            res["c_over_a"] = round(res["c_hit_ms"] / res["a_fresh_ms"], 4)
    if "d" in args.legs:
        h = T // 2
        halves = [(vs[:h], vd[:h]), (vs[h:], vd[h:]), (vs, vd)]

        def lvcot_fresh():
            return [call(s, d) for s, d in halves]

        def lvcot_cached():
            return [call(s, d, cache=box["c"]) for s, d in halves]
        res["d_lvcot_fresh_ms"], _, w = timed(lvcot_fresh, args.reps)
        res["d_lvcot_cached_ms"], _, g = timed(lvcot_cached, args.reps, fresh_cache)
        assert all(torch.equal(x, y) for x, y in zip(w, g)), "LVCoT sequence differs"
    if "e" in args.legs:
        idx = frame_indices(enc.cfg, T, 64, T)
        nbytes = len(idx) * (vs[0].numel() + vd[0].numel()) * vs.element_size()

        def fp():
            ops.fingerprint_rows(vs, idx)
            return ops.fingerprint_rows(vd, idx)
        for _ in range(args.warmup):
            fp()
        ms, _, _ = timed(fp, max(args.reps, 10))
        res["e_fingerprint_ms"] = ms
        res["e_fingerprint_bytes"] = nbytes
        res["e_fingerprint_GBps"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
        res["e_fraction_of_hbm_peak"] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def region_stats(trace_csv, out_csv, marker="spin_kernel"):
    """per-kernel statistics of the dispatches between the last two marker kernels of a rocprofv3 kernel trace"""
    import csv
    from collections import defaultdict
    with open(trace_csv) as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if marker in r["Kernel_Name"]]
    assert len(marks) >= 2, "no marked region in %s" % trace_csv
    region = rows[marks[-2] + 1:marks[-1]]
    agg = defaultdict(list)
    for r in region:
        agg[r["Kernel_Name"]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = sum(sum(v) for v in agg.values())
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage"])
        for name, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([name, len(v), sum(v), round(sum(v) / len(v), 1), round(100.0 * sum(v) / total, 2)])
    print(json.dumps({"region_dispatches": len(region), "region_kernel_ns": total, "kernels": len(agg)}))


if __name__ == "__main__":
    main()
