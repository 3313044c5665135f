"""What one multi-prompt compressor pass (VideoEncoder.encode_video_prompts, `config.tdc_batch_prompts`)
costs per question against P sequential cached encode_video calls, at the bench geometry: bench.py's weights and synthetic
video (model_cfg, random_state_dict, synth_video; T = 512, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream), a WARM frame cache in both variants, K = 144 and K = 16, P = 1, 2, 4, 8 questions with ragged BERT lengths 6 .. 40.

  sequential   P x encode_video(cache=c)            the behaviour with the key off
  multi        1 x encode_video_prompts(cache=c)    at pad_fraction 0, 1/4 and 1

The variants alternate inside one process; each figure is the median of --reps timed rounds after --warmup, device events
around the whole variant.  Per variant: ms per question, torch.cuda.max_memory_allocated of one run, and the launch counts
of one run (ops.profile_start/stop).  Every multi result is checked torch.equal against its sequential one.

Without --step the tool is the driver: one process per K, each under its own `timeout -k 10`, chained with `&&`; the parts
are merged into --out (default profiles/multi_prompt.json)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (144, 16)
PS = (1, 2, 4, 8)
LENS = (6, 40, 12, 31, 9, 24, 17, 36)            # BERT prompt lengths of questions 0 .. 7 (CLS and SEP included)
PADS = (0.0, 0.25, 1.0)


def questions(P):
    return [dict(budget_text_len=64, n_text_tokens=64 + 5 * i, prompt_ids=[101] + list(range(2000 + 50 * i, 2000 + 50 * i + n - 2))
                 + [102]) for i, n in enumerate(LENS[:P])]


def step(K, T, reps, warmup, out):
    import torch
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops
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
    cache = enc.new_cache(8 << 30)
    info = {}
    enc.encode_video(vs, vd, (384, 384), 64, 64, questions(1)[0]["prompt_ids"], frame_cap=T, cache=cache, info=info)   # warms it
    assert not info["cache"]["bypassed"]
    res = {"K": K, "frames": T, "device": torch.cuda.get_device_name(dev), "reps": reps, "warmup": warmup, "P": {}}
    for P in PS:
        qs = questions(P)

        def sequential():
            return [enc.encode_video(vs, vd, (384, 384), q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"], frame_cap=T,
                                     cache=cache) for q in qs]

        def multi(pad, infos=None):
            return enc.encode_video_prompts(vs, vd, (384, 384), qs, frame_cap=T, cache=cache, max_prompts=8, pad_fraction=pad,
                                            infos=infos)
        variants = [("sequential", sequential)] + [("multi_pad_%g" % p, (lambda p=p: multi(p))) for p in PADS]
        ms = {n: [] for n, _ in variants}
        outs = {}
        for r in range(warmup + reps):
            for name, fn in variants:                             # the variants alternate
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                outs[name] = fn()
                b.record()
                torch.cuda.synchronize()
                if r >= warmup:
                    ms[name].append(a.elapsed_time(b))
            for name, _ in variants[1:]:
                assert all(torch.equal(x, y) for x, y in zip(outs[name], outs["sequential"])), (K, P, name)
        row = {}
        for name, fn in variants:
            outs.clear()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev)
            ops.profile_start()
            fn()
            torch.cuda.synchronize()
            recs = ops.profile_stop()
            med = statistics.median(ms[name])
            row[name] = {"ms_per_question": round(med / P, 3), "ms": round(med, 3), "ms_all": [round(v, 3) for v in ms[name]],
                         "max_memory_allocated_gb": round(peak / 1e9, 3), "launches": len(recs),
                         "gemm_launches": sum(1 for x in recs if x["kind"] == "gemm")}
        for pad in PADS:
            infos = [{} for _ in qs]
            multi(pad, infos)
            n = "multi_pad_%g" % pad
            row[n]["group_sizes"] = [i["prompts"]["group_size"] for i in infos]
            row[n]["pad_rows"] = sum(i["prompts"]["pad_rows"] for i in infos)
            row[n]["speedup"] = round(row["sequential"]["ms"] / row[n]["ms"], 3)
        res["P"][str(P)] = row
        print("K=%d P=%d " % (K, P) + " ".join("%s %.2f ms/q" % (n, row[n]["ms_per_question"]) for n, _ in variants), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None, help="run one K in this process (what the driver starts)")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds of one K's process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_prompt.json"))
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
                       "tdc_tower_res_dtype": "float16", "prompt_lens": list(LENS), "frame_cache": "warm"}, "K": {}}
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
