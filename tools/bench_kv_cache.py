"""What the kept cross-attention K/V (FrameCache(kv_bytes=...), `config.tdc_kv_cache_bytes`) saves a
later question about a cached video, at the bench geometry: bench.py's weights and synthetic video (model_cfg,
random_state_dict, synth_video; T = 512, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual stream), K = 144 and
K = 16, two caches in one process - one with kv_bytes = 0 (the parent commit's code path), one with a K/V budget.

  a  second_off    a second question, warm frames, kv_bytes = 0              the baseline
  b  second_hit    the same question, warm frames, its K/V entry kept        the K/V GEMM and the enc gather are not launched
  c  first_off     the first call on a video (empty cache), kv_bytes = 0
     first_fill    the same call, filling the K/V entry
     warm_fill     warm frames, the K/V entry dropped (kv_clear): the fill alone, against a

The routes alternate inside one process; each figure is the median of --reps timed rounds after --warmup, device events around
the call.  Per route: ms, every sample, torch.cuda.max_memory_allocated of one run; per K: the entry's bytes.  The spread a
difference is judged by is the run-to-run spread (max - min) of the baseline route within the same run.  Every result is
checked torch.equal against the kv_bytes = 0 one.

Without --step the tool is the driver: one process per K, each under its own `timeout -k 10`, chained with `&&`; the parts
are merged into --out (default profiles/kv_cache.json)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (144, 16)
FIRST = [101] + list(range(2000, 2010)) + [102]                  # the question that fills: 12 BERT ids
SECOND = [101] + list(range(3000, 3029)) + [102]                 # the later question: 31


def step(K, T, reps, warmup, out):
    import torch
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd.pipeline import VideoEncoder
    dev = torch.device("cuda", 0)
    H = 3584
    gen = torch.Generator(device=dev).manual_seed(0)
    sd = bench.random_state_dict(H, K, dev, gen)
    enc = VideoEncoder(sd, bench.model_cfg(H, K, T), dtype=torch.float16, device=dev, tower_dtype=torch.bfloat16,
                       tower_res_dtype=torch.float16)
    enc.two_streams = T <= 128
    del sd
    torch.cuda.empty_cache()
    vs = bench.synth_video(0, T, 384, dev, torch.bfloat16)
    vd = bench.synth_video(0, T, 378, dev, torch.bfloat16, seed=4321)
    off, on = enc.new_cache(8 << 30), enc.new_cache(8 << 30, kv_bytes=4 << 30)

    def ask(cache, prompt, info=None):
        return enc.encode_video(vs, vd, (384, 384), 64, 64 + len(prompt), prompt, frame_cap=T, cache=cache, info=info)

    def warm(cache):
        info = {}
        ask(cache, FIRST, info)
        assert not info["cache"]["bypassed"]
        return info

    def second_off():
        return ask(off, SECOND)

    def second_hit():
        return ask(on, SECOND)

    def warm_fill():
        on.kv_clear()
        return ask(on, SECOND)

    def first_off():
        off.clear()
        return ask(off, SECOND)

    def first_fill():
        on.clear()
        return ask(on, SECOND)
    routes = [("second_off", second_off), ("second_hit", second_hit), ("warm_fill", warm_fill), ("first_off", first_off),
              ("first_fill", first_fill)]
    entry = warm(on)["cache"]["kv"]
    warm(off)
    assert entry["state"] == "filled", entry
    info = {}
    want = ask(on, SECOND, info)
    assert info["cache"]["kv"]["state"] == "hit", info["cache"]["kv"]
    ms = {n: [] for n, _ in routes}
    for r in range(warmup + reps):
        for name, fn in routes:                                   # the routes alternate
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            got = fn()
            b.record()
            torch.cuda.synchronize()
            assert torch.equal(got, want), (K, name)
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
        warm(off)                                                 # first_off / first_fill left SECOND's state: both caches warm,
        ask(on, FIRST)                                            # the K/V entry kept, for the next round's second_* routes
    row = {}
    for name, fn in routes:
        warm(off)
        ask(on, FIRST)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        v = ms[name]
        row[name] = {"ms": round(statistics.median(v), 3), "ms_all": [round(x, 3) for x in v],
                     "spread_ms": round(max(v) - min(v), 3),
                     "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 3)}

    def gate(base, new):
        sp = row[base]["spread_ms"]
        d = row[base]["ms"] - row[new]["ms"]
        return {"baseline": base, "route": new, "saved_ms": round(d, 3), "baseline_spread_ms": sp,
                "not_slower_beyond_spread": bool(-d <= sp), "gain_beyond_spread": bool(d > sp)}
    res = {"K": K, "frames": T, "device": torch.cuda.get_device_name(dev), "reps": reps, "warmup": warmup,
           "kv_entry": {"frames": entry["frames"], "rows_per_frame": on.rows_per_frame, "bytes": entry["bytes"]},
           "routes": row, "gates": {"b_hit_vs_a": gate("second_off", "second_hit"),
                                    "c_first_fill_vs_first_off": gate("first_off", "first_fill"),
                                    "c_warm_fill_vs_a": gate("second_off", "warm_fill")}}
    print("K=%d " % K + " ".join("%s %.2f ms" % (n, row[n]["ms"]) for n, _ in routes) + " entry %d B" % entry["bytes"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None, help="run one K in this process (what the driver starts)")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds of one K's process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_cache.json"))
    args = ap.parse_args()
    if args.step is not None:
        return step(args.step, args.frames, args.reps, args.warmup, args.out)
    parts = [args.out + ".K%d.part" % K for K in KS]
    me = os.path.abspath(__file__)
    # one GPU step per K, each under its own time limit, chained: a step that fails or runs out of time starts nothing after it
    chain = " && ".join("timeout -k 10 %d %s %s --step %d --frames %d --reps %d --warmup %d --out %s"
                        % (args.step_timeout, sys.executable, me, K, args.frames, args.reps, args.warmup, p)
                        for K, p in zip(KS, parts))
    rc = subprocess.run(["bash", "-c", chain], cwd=ROOT).returncode
    if rc != 0:
        sys.exit(rc)
    res = {"setting": {"frames": args.frames, "H": 3584, "dtype": "float16", "tdc_tower_dtype": "bfloat16",
                       "tdc_tower_res_dtype": "float16", "prompt_lens": [len(FIRST), len(SECOND)],
                       "spread": "max - min of the baseline route's samples in the same run"}, "K": {}}
    for K, p in zip(KS, parts):
        with open(p) as f:
            res["K"][str(K)] = json.loads(f.read())
        os.remove(p)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
