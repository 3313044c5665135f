"""What encode_video(aux=...) (the reference's three aux outputs, `config.tdc_return_aux`) costs a call at
the bench geometry: bench.py's weights and synthetic video (model_cfg, random_state_dict, synth_video; H = 3584, K = 144, fp16
connector / Q-Former, bf16 towers, fp16 residual stream), T = 224 and T = 512.

  off   encode_video(...)           the call as it always was: the baseline
  on    encode_video(..., aux={})   + three caller-owned keep buffers while the connector runs, three tdc_gather_rows launches

The two routes alternate inside one process; each figure is the median of --reps timed rounds after --warmup, device events
around the call.  Per route: ms, every sample, torch.cuda.max_memory_allocated of one run; for `on` the bytes of the three
outputs.  The spread a difference is judged by is the run-to-run spread (max - min) of the `off` route within the same run.
The visual tokens of `on` are checked torch.equal against those of `off`.

Without --step the tool is the driver: one process per T, each under its own `timeout -k 10`, chained with `&&`; the parts
are merged into --out (default profiles/aux_outputs.json)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = (224, 512)
PROMPT = [101] + list(range(2000, 2010)) + [102]


def step(T, K, reps, warmup, out):
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

    def off():
        return enc.encode_video(vs, vd, (384, 384), 64, 64 + len(PROMPT), PROMPT, frame_cap=T), None

    def on():
        d = {}
        return enc.encode_video(vs, vd, (384, 384), 64, 64 + len(PROMPT), PROMPT, frame_cap=T, aux=d), d
    routes = [("off", off), ("on", on)]
    want, _ = off()
    ms = {n: [] for n, _ in routes}
    for r in range(warmup + reps):
        for name, fn in routes:                                   # the routes alternate
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            got, d = fn()
            b.record()
            torch.cuda.synchronize()
            assert torch.equal(got, want), (T, name)
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
            del got, d
    row, out_bytes = {}, None
    for name, fn in routes:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        got, d = fn()
        torch.cuda.synchronize()
        v = ms[name]
        row[name] = {"ms": round(statistics.median(v), 3), "ms_all": [round(x, 3) for x in v], "spread_ms": round(max(v) - min(v), 3),
                     "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 3)}
        if d is not None:
            nb = lambda t: t.numel() * t.element_size()
            out_bytes = {"features": [nb(t) for t in d["features"]], "masks": [nb(t) for t in d["masks"]],
                         "global_context": nb(d["global_context"]), "windows": int(d["global_context"].shape[0])}
        del got, d
    sp = row["off"]["spread_ms"]
    extra = row["on"]["ms"] - row["off"]["ms"]
    res = {"frames": T, "K": K, "device": torch.cuda.get_device_name(dev), "reps": reps, "warmup": warmup, "routes": row,
           "output_bytes": out_bytes,
           "gate": {"baseline": "off", "route": "on", "extra_ms": round(extra, 3), "baseline_spread_ms": sp,
                    "extra_share_of_step": round(extra / row["off"]["ms"], 5), "within_spread": bool(extra <= sp)}}
    print("T=%d off %.2f ms on %.2f ms (+%.2f, spread of off %.2f) outputs %d B" % (
        T, row["off"]["ms"], row["on"]["ms"], extra, sp, sum(out_bytes["features"]) + out_bytes["global_context"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None, help="run one T in this process (what the driver starts)")
    ap.add_argument("--K", type=int, default=144)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds of one T's process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_outputs.json"))
    args = ap.parse_args()
    if args.step is not None:
        return step(args.step, args.K, args.reps, args.warmup, args.out)
    parts = [args.out + ".T%d.part" % T for T in FRAMES]
    me = os.path.abspath(__file__)
    # one GPU step per T, each under its own time limit, chained: a step that fails or runs out of time starts nothing after it
    chain = " && ".join("timeout -k 10 %d %s %s --step %d --K %d --reps %d --warmup %d --out %s"
                        % (args.step_timeout, sys.executable, me, T, args.K, args.reps, args.warmup, p)
                        for T, p in zip(FRAMES, parts))
    rc = subprocess.run(["bash", "-c", chain], cwd=ROOT).returncode
    if rc != 0:
        sys.exit(rc)
    res = {"setting": {"H": 3584, "K": args.K, "dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16",
                       "image_size": [384, 384], "spread": "max - min of the `off` route's samples in the same run"}, "frames": {}}
    for T, p in zip(FRAMES, parts):
        with open(p) as f:
            res["frames"][str(T)] = json.loads(f.read())
        os.remove(p)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
