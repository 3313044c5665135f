"""What `config.tdc_batch_frames` (VideoEncoder.encode_batch: every sample of a call in one tower and connector pass) does to the
cost of a batched mixin call, at the bench geometry: bench.py's weights, stub LM and synthetic video (model_cfg,
random_state_dict, build_mixin_lm, synth_video; K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream, tdc_frame_cap = 512).  The same prepare_inputs_labels_for_multimodal call runs with the key off (0: per sample) and on
(the case's frame total), the two modes alternating in one process, timed with device events after warm-up, median of --reps:

  a  16 single images, image_size square / 16:9 / 9:16 in turn     batched image QA
  b  8 clips x 16 frames (T <= 25: no Q-Former)                    short clips
  c  4 videos x 64 frames, each with its own prompt                short videos
  d  2 videos x 256 frames                                         the no-gain control

Per case and mode: ms per call, images or a1-selected frames per second, torch.cuda.max_memory_allocated of one call, and the
tower GEMM launches of one call (ops.profile_start/stop, launches issued inside VideoEncoder.tower).  Every pair of outputs
is checked torch.equal.  Prints one JSON object; --out writes it too."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOWER_TAG = 77          # profile tag of the launches issued inside VideoEncoder.tower
CASES = {"a": (16, 1), "b": (8, 16), "c": (4, 64), "d": (2, 256)}     # samples, frames per sample (1: single images)
SIZES = [(384, 384), (360, 640), (640, 360)]


def inputs(case, dev, dtype):
    """(input_ids, images, image_sizes, prompts) of one case"""
    import bench
    B, T = CASES[case]
    ids = torch.arange(100, 165, device=dev)
    ids[14] = -200                                                       # IMAGE_TOKEN_INDEX
    ids = ids[None].repeat(B, 1)
    if T == 1:
        vs = bench.synth_video(0, B, 384, dev, dtype, scene_len=1)
        vd = bench.synth_video(0, B, 378, dev, dtype, seed=4321, scene_len=1)
        return ids, [vs, vd], [SIZES[i % 3] for i in range(B)], None
    vs = [bench.synth_video(i * T, (i + 1) * T, 384, dev, dtype, seed=1234 + i) for i in range(B)]
    vd = [bench.synth_video(i * T, (i + 1) * T, 378, dev, dtype, seed=4321 + i) for i in range(B)]
    prompts = [[101] + list(range(2000 + 7 * i, 2010 + 7 * i)) + [102] for i in range(B)]
    return ids, [vs, vd], [(384, 384)] * B, prompts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops
    dev = torch.device("cuda", 0)
    H, K = 3584, 144
    gen = torch.Generator(device=dev).manual_seed(0)
    sd = bench.random_state_dict(H, K, dev, gen)
    extra = {"tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16", "tdc_frame_cap": 512}
    lm = bench.build_mixin_lm(bench.model_cfg(H, K, 512), sd, dev, torch.float16, extra)
    m = lm.get_model()
    eng = m.tdc_engine(device=dev, dtype=torch.float16)
    del sd
    torch.cuda.empty_cache()
    tower = eng.tower

    def tagged_tower(name, px):
        ops.profile_tag(TOWER_TAG)
        try:
            return tower(name, px)
        finally:
            ops.profile_tag(0)
    eng.tower = tagged_tower
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "setting": dict(extra, dtype="float16", H=H, K=K), "cases": {}}
    for case in args.cases:
        B, T = CASES[case]
        ids, images, sizes, prompts = inputs(case, dev, torch.bfloat16)
        n = B * T
        kw = dict(image_sizes=sizes)
        if prompts is not None:
            kw.update(video_indices=[None] * B, prompts=prompts, audios=[None] * B)

        def call(on):
            m.config.tdc_batch_frames = n if on else 0
            with torch.no_grad():
                return lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, images, **kw)
        ms = {False: [], True: []}
        outs = {}
        for r in range(args.warmup + args.reps):
            for on in (False, True):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                outs[on] = call(on)
                b.record()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    ms[on].append(a.elapsed_time(b))
            equal = all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(outs[False], outs[True]))
            assert equal, "case %s: batched output differs from per-sample output" % case
        row = {"samples": B, "frames_per_sample": T, "equal": True}
        for on in (False, True):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            call(on)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev)
            ops.profile_start()
            call(on)
            torch.cuda.synchronize()
            recs = ops.profile_stop()
            tg = [r for r in recs if r["kind"] == "gemm" and r["tag"] == TOWER_TAG]
            med = statistics.median(ms[on])
            row["on" if on else "off"] = {
                "ms": round(med, 3), ("images_per_s" if T == 1 else "frames_per_s"): round(n / med * 1e3, 1),
                "max_memory_allocated_gb": round(peak / 1e9, 3), "tower_gemm_launches": len(tg),
                "tower_gemm_rows": sum(r["M"] for r in tg), "gemm_launches": sum(1 for r in recs if r["kind"] == "gemm"),
                "ms_all": [round(v, 3) for v in ms[on]]}
        row["speedup"] = round(row["off"]["ms"] / row["on"]["ms"], 3)
        res["cases"][case] = row
        del images, outs
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
