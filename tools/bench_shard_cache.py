"""What the frame cache of the frame-sharded path (dist.ShardedVideoEncoder.encode_video(cache=...)) saves: a one-GPU
rehearsal of a world-8 job - eight ranks as threads of one process, each with its own engine and cache, exchanging through
the tests' in-process transport (tests/util.ThreadComm) - at bench.py's geometry (T = 512, K = 144, H = 3584, fp16 connector
/ Q-Former, bf16 towers, fp16 residual stream).  The ranks share one chip, so the wall times are NOT a multi-GPU latency: the
towers of the eight ranks run one after another on the same device, and the transport is a host copy.

  cold  every rank with an empty cache (cleared before each call): towers + connector on every frame, stored
  warm  a second question (other prompt_ids and n_text_tokens) on the same video: every frame a hit

Wall time of one call (all ranks joined, device synchronised), median of --reps after --warmup calls; per-rank info["cache"]
of the last call of each leg; the tower launches (engine.tower calls, all ranks) per call.  Every result is checked
torch.equal against the uncached serial encode.  Prints one JSON object; --out writes it too."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))         # the tests' helpers import from there


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cache-bytes", type=int, default=1 << 30, help="per rank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_cache_threads.json"))
    args = ap.parse_args()
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd.dist import ShardedVideoEncoder
    from tdc_video_amd.pipeline import VideoEncoder
    from test_hip_dist2 import run_threads
    dev = torch.device("cuda", 0)
    world, T, H, K = args.world, args.frames, 3584, 144
    engines = []
    for _ in range(world + 1):                              # the last one: the serial reference
        gen = torch.Generator(device=dev).manual_seed(0)
        sd = bench.random_state_dict(H, K, dev, gen)
        e = VideoEncoder(sd, bench.model_cfg(H, K, T), dtype=torch.float16, device=dev, tower_dtype=torch.bfloat16,
                         tower_res_dtype=torch.float16)
        e.two_streams = T // world <= 128                    # the mixin's default (tdc_side_stream)
        del sd
        e.tower_calls = 0
        tower = e.tower

        def counted(name, px, _e=e, _tower=tower):
            _e.tower_calls += 1
            return _tower(name, px)
        e.tower = counted
        engines.append(e)
    ref = engines.pop()
    torch.cuda.empty_cache()
    vs = bench.synth_video(0, T, 384, dev, torch.bfloat16)
    vd = bench.synth_video(0, T, 378, dev, torch.bfloat16, seed=4321)
    q1 = [101] + list(range(2000, 2010)) + [102]
    q2 = [101, 3000, 3001, 3002, 3003, 102]
    shards = [ShardedVideoEncoder(e, r, world, comm=None) for r, e in enumerate(engines)]
    plans = [sh.frame_plan(T, budget_text_len=64, frame_cap=T) for sh in shards]
    local = [(vs[p["lo"]:p["hi"]].contiguous(), vd[p["lo"]:p["hi"]].contiguous()) for p in plans]
    caches = [e.new_cache(args.cache_bytes) for e in engines]
    infos = [{} for _ in range(world)]

    def call(prompt, n_text):
        def rank(r, comm):
            shards[r].comm = comm
            return shards[r].encode_video(local[r][0], local[r][1], T, (384, 384), n_text, prompt,
                                          sample_indices=plans[r]["sample_indices"], cache=caches[r], info=infos[r])
        out = run_threads(world, rank)
        torch.cuda.synchronize()
        return out

    def timed(prompt, n_text, setup=None):
        ms, launches, out = [], [], None
        for i in range(args.warmup + args.reps):
            if setup is not None:
                setup()
            torch.cuda.synchronize()
            n0 = sum(e.tower_calls for e in engines)
            t0 = time.perf_counter()
            out = call(prompt, n_text)
            if i >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
                launches.append(sum(e.tower_calls for e in engines) - n0)
        return round(statistics.median(ms), 2), launches, out

    want1 = ref.encode_video(vs, vd, (384, 384), budget_text_len=64, n_text_tokens=64, prompt_ids=q1, frame_cap=T)
    want2 = ref.encode_video(vs, vd, (384, 384), budget_text_len=64, n_text_tokens=40, prompt_ids=q2, frame_cap=T)
    torch.cuda.synchronize()
    res = dict(note="one-GPU rehearsal: %d ranks as threads sharing ONE MI355X (in-process transport); not a multi-GPU "
                    "latency" % world, world=world, frames=T, K=K, H=H, cache_bytes_per_rank=args.cache_bytes, reps=args.reps,
               warmup=args.warmup)
    res["cold_ms"], res["cold_tower_launches_per_call"], got = timed(q1, 64, lambda: [c.clear() for c in caches])
    assert all(torch.equal(g, want1) for g in got), "cold cached sharded call differs from the serial encode"
    res["cold_cache"] = [dict(i["cache"]) for i in infos]
    res["warm_ms"], res["warm_tower_launches_per_call"], got = timed(q2, 40)
    assert all(torch.equal(g, want2) for g in got), "warm cached sharded call differs from the serial encode"
    res["warm_cache"] = [dict(i["cache"]) for i in infos]
    res["warm_frames_encoded_all_ranks"] = [i["cache"]["frames_encoded"] for i in infos]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
