"""The gap table of a compact feature set measured: what `gaps="auto"` costs on export and in bytes, and
what it saves and protects on encode.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream), as tools/bench_feature_store.py builds it, at T0 = 512 and T0 = 1000 frames.  Per T0:

  export_s        seconds of export_features(store="e4m3") without and with the table, alternating inside one process,
                  --exports (>= 5) each; the median, the extremes and the difference
  table_ms        VideoEncoder.gap_sims_tensor alone on the video's 16-bit DINOv2 rows: device events around the call (the
                  tdc_pair_cossim launches, the pair uploads and the scatter) and the host's wall clock around it
  bytes           of the set without and with the table
  encode_ms       encode_features at frame cap 224 from the two sets, alternating, host wall clock around a synchronised call:
                  the set with the table skips the a5 launch and the host's read of its result

And on the reduced engine of tests/test_hip_feature_store.py (towers 48 / 64 wide, fp16), over --videos (>= 50) synthetic
videos of 40 frames sub-sampled to 30: how many selections on the decoded rows differ from the lossless set's, how many from a
set with the table do (0: the stored values are the lossless path's, which is also counted), and the largest move of a
similarity under the e4m3 rounding.

No time is gated.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))         # the tests' helpers import from there


def spread(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd), "n": len(v)}


def full_size(args, torch, dev):
    import bench
    from tdc_video_amd.pipeline import VideoEncoder
    K, H = args.K, args.hidden
    gen = torch.Generator(device=dev).manual_seed(0)
    sd = bench.random_state_dict(H, K, dev, gen)
    enc = VideoEncoder(sd, bench.model_cfg(H, K, max(args.frames)), dtype=torch.float16, device=dev, tower_batch=512,
                       tower_dtype=torch.bfloat16, tower_res_dtype=torch.float16)
    enc.two_streams = False
    del sd
    torch.cuda.empty_cache()
    enc.feature_signature()                                       # the one-time fingerprint of the tower weights: not an export cost
    prompt_ids = [101] + list(range(2000, 2010)) + [102]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    rows = {}
    for T0 in args.frames:
        vs = bench.synth_video(0, T0, 384, dev, torch.bfloat16)
        vd = bench.synth_video(0, T0, 378, dev, torch.bfloat16, seed=4321)
        export = {"without": lambda: enc.export_features(vs, vd, (384, 384), store="e4m3"),
                  "with": lambda: enc.export_features(vs, vd, (384, 384), store="e4m3", gaps="auto")}
        sets, secs = {}, {"without": [], "with": []}
        for r in range(1 + args.exports):                         # round 0 warms the allocator up
            for name, fn in export.items():
                t, sets[name] = wall(fn)
                if r:
                    secs[name].append(t)
        plain, cs = sets["without"], sets["with"]
        G = cs.gaps
        # the table alone, on the 16-bit DINOv2 rows the export takes it from
        dino = enc.tower("dino", vd)
        del vs, vd
        enc.gap_sims_tensor(dino, T0, G)
        ev_ms, wall_ms = [], []
        for _ in range(args.exports):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            table = enc.gap_sims_tensor(dino, T0, G)
            b.record()
            torch.cuda.synchronize()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            ev_ms.append(a.elapsed_time(b))
        same = bool(torch.equal(table, cs.gap_sims)) and bool(torch.equal(table[0], enc.sims_tensor(dino, T0)))
        del dino, table
        torch.cuda.empty_cache()
        # encode at the reference's frame cap from both sets
        ms, infos = {"without": [], "with": []}, {}
        for r in range(args.warmup + args.steps):
            for name, s in (("without", plain), ("with", cs)):
                info = {}
                t, _ = wall(lambda: enc.encode_features(s, 64, 64, prompt_ids, frame_cap=224, info=info))
                infos[name] = info
                if r >= args.warmup:
                    ms[name].append(t * 1e3)
        med = {k: statistics.median(v) for k, v in secs.items()}
        rows[str(T0)] = {
            "frames": T0, "gaps": G, "pairs": sum(T0 - g for g in range(1, G + 1)),
            "export_s": {"without": spread(secs["without"]), "with": spread(secs["with"]),
                         "with_minus_without_ms": round((med["with"] - med["without"]) * 1e3, 1),
                         "overhead": round(med["with"] / med["without"] - 1.0, 4)},
            "table_ms": {"device_events": spread(ev_ms), "host_wall": spread(wall_ms), "equals_exported_table": same},
            "bytes": {"without": plain.nbytes, "with": cs.nbytes, "table": cs.nbytes - plain.nbytes},
            "encode_ms_cap_224": {"without": spread(ms["without"]), "with": spread(ms["with"]),
                                  "with_minus_without": round(statistics.median(ms["with"]) - statistics.median(ms["without"]), 3),
                                  "frames_kept": len(infos["with"]["frame_indices"]),
                                  "selection_sims": {k: infos[k].get("selection_sims") for k in infos},
                                  "selection_equal": infos["with"]["seg_indices"] == infos["without"]["seg_indices"]}}
        del plain, cs, sets
        torch.cuda.empty_cache()
    return rows


def reduced_engine(args, torch):
    from tdc_video_amd import encode, features, segment as seg
    from test_hip_feature_store import _load, video
    from test_hip_pipeline import make_encoder
    from util import pipeline_cfg
    f = _load()
    enc = make_encoder(f["W"], pipeline_cfg(f["o"]), torch.float16)
    mns = enc.cfg.get("max_num_segments", 24)
    idx = encode.frame_indices(enc.cfg, 40, 9, 30)
    differ_decoded = differ_table = stored_not_lossless = 0
    moved, margins = [], []
    for seed in range(args.videos):
        vid = video(f["o"], seed).cuda()
        fs = enc.export_features(vid, vid + 0.01, f["size"])
        plain, cs = enc.compact_features(fs), enc.compact_features(fs, gaps="auto")
        lossless = enc.sims_tensor(encode.feature_rows(enc, fs, idx)[1], len(idx)).tolist()
        decoded = enc.sims_tensor(encode.feature_rows(enc, plain, idx)[1], len(idx)).tolist()
        stored = features.stored_sims(cs, idx)
        want = seg.select_segments(lossless, mns)
        differ_decoded += seg.select_segments(decoded, mns) != want
        differ_table += stored is None or seg.select_segments(stored, mns) != want
        stored_not_lossless += stored != lossless
        moved.append(max(abs(a - b) for a, b in zip(lossless, decoded)))
        order = sorted(lossless)
        margins.append(order[mns] - order[mns - 1])
    return {"engine": "tests/test_hip_feature_store.py (towers 48/64 wide, fp16)", "videos": args.videos, "frames": 40,
            "frames_kept": len(idx), "gaps": cs.gaps, "decoded_selections_differ": int(differ_decoded),
            "table_selections_differ": int(differ_table), "stored_values_not_the_lossless_ones": int(stored_not_lossless),
            "sims_moved_max": float(max(moved)), "sims_moved_median": float(statistics.median(moved)),
            "rank_margin_min": float(min(margins)), "rank_margin_median": float(statistics.median(margins))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[512, 1000])
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--exports", type=int, default=5, help="timed exports per form (at least 5)")
    ap.add_argument("--steps", type=int, default=10, help="timed encode_features calls per set")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--videos", type=int, default=60, help="synthetic videos on the reduced engine (at least 50)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.exports < 5:
        ap.error("--exports: at least 5 timed exports per form")
    if args.videos < 50:
        ap.error("--videos: at least 50")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_gap_sims.py measures on a GPU; none is visible")
    import tdc_video_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    res = {"tool": "bench_gap_sims", "device": torch.cuda.get_device_name(dev), "K": args.K, "H": args.hidden,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16", "gaps": "auto"},
           "exports": args.exports, "steps": args.steps, "warmup": args.warmup,
           "full_size": full_size(args, torch, dev), "reduced_engine": reduced_engine(args, torch)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
