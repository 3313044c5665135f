"""Encode from decoded PCM audio measured: what tdc_pcm_resample costs, what it uploads, and what the
audio-on step costs when it is fed audio={"audio_pcm": ...} instead of the pre-resampled audio={"audio_wav": ...}.

One engine with bench.py's geometry and types (K = 144, H = 3584, fp16 connector / Q-Former, bf16 towers, fp16 residual
stream), a random audio_proj and a random BEATs of the iter3 architecture (tools/bench_beats.py), as the audio test of
tests/test_hip_video_cache.py builds them.  The video is bench.py's synthetic one at one frame per second of audio (--seconds,
default 600: ten minutes), frame cap 224.  Tracks of that duration, tones under noise:
  s16_48k    48 kHz stereo int16, interleaved (a decoder's packed format), channel 0
  f32_44k    44.1 kHz stereo float32, planar, channel 0
each from pinned host memory and device-resident.  Per track and residence:
  resample   audio.resample of the whole track alone, device events, median of --steps: ms, GB/s (the bytes of the addressed
             channel read plus 4 bytes per output written), and for the pinned track the bytes uploaded beside the bytes of
             the fp32 16 kHz waveform a caller would upload instead
  step       encode_video(audio={"audio_pcm": pcm}) against encode_video(audio={"audio_wav": wav}), alternating inside one
             process, --steps (>= 10) timed steps after --warmup rounds: median, min, max; spread_ms = max - min of the waveform
             route's steps; the two outputs are asserted torch.equal
  host       scipy.signal.resample_poly(channel 0 as float32, L, M) of the same track, one timed run: what a caller did
             before (another filter than the definition's: it is there for its time, not its values)
Nothing is required of the numbers: the tool records them.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=144, help="context_token_num (the reference's default: 16)")
    ap.add_argument("--hidden", type=int, default=3584)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=int, default=600, help="duration of the track and frames of the video")
    ap.add_argument("--cap", type=int, default=224)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 timed steps")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pcm_audio.py measures on a GPU; none is visible")
    import numpy as np
    import scipy.signal
    import bench
    import tdc_video_amd  # noqa: F401
    from bench_beats import random_beats_state
    from tdc_video_amd import audio
    from tdc_video_amd import weights as Wt
    from tdc_video_amd.beats import BEATS_ITER3_CFG, BeatsEncoder
    from tdc_video_amd.pipeline import VideoEncoder
    dev = torch.device("cuda", 0)
    K, H, T0 = args.K, args.hidden, args.seconds
    gen = torch.Generator(device=dev).manual_seed(0)
    sd = bench.random_state_dict(H, K, dev, gen)
    cfg = dict(bench.model_cfg(H, K, T0), audio_input=True)
    enc = VideoEncoder(sd, cfg, dtype=torch.float16, device=dev, tower_dtype=torch.bfloat16, tower_res_dtype=torch.float16)
    del sd
    enc.c.audio_proj = Wt.make_lin(torch.randn(H, 768, device=dev, generator=gen) * 0.02, torch.zeros(H, device=dev), enc.dtype, dev)
    enc.beats = BeatsEncoder(random_beats_state(BEATS_ITER3_CFG), BEATS_ITER3_CFG, dtype=enc.dtype, device=dev)
    enc.two_streams = False
    torch.cuda.empty_cache()
    prompt_ids = [101] + list(range(2000, 2010)) + [102]
    vs = bench.synth_video(0, T0, 384, dev, torch.float16, scene_len=5)
    vd = bench.synth_video(0, T0, 378, dev, torch.float16, seed=4321, scene_len=5)

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

    def track(sr, planar, as_int16):
        """[n, 2] (or planar [2, n]) on the device: two tones per channel under noise, amplitude below 0.5"""
        n = T0 * sr
        t = torch.arange(n, device=dev, dtype=torch.float64) / sr
        ch = [(0.3 * torch.sin(2 * torch.pi * (220.0 + 110.0 * c) * t) + 0.1 * torch.sin(2 * torch.pi * 3100.0 * t)).float()
              + 0.03 * torch.randn(n, device=dev, generator=gen) for c in range(2)]
        a = torch.stack(ch, 0 if planar else 1)
        return (a * 32767).round().clamp(-32768, 32767).to(torch.int16).contiguous() if as_int16 else a.contiguous()

    def encode(au):
        return enc.encode_video(vs, vd, (384, 384), budget_text_len=64, n_text_tokens=64, prompt_ids=prompt_ids, audio=au,
                                frame_cap=args.cap)

    tracks = []
    for name, sr, planar, as_int16 in (("s16_48k", 48000, False, True), ("f32_44k", 44100, True, False)):
        data = track(sr, planar, as_int16)
        kw = {"layout": "planar"} if planar else {}
        L, M, Kt, _ = audio.resample_tables(sr, dev)
        src = {"device": data, "pinned": pinned(data)}
        rec = {"track": name, "sample_rate": sr, "channels": 2, "layout": "planar" if planar else "interleaved",
               "dtype": str(data.dtype).replace("torch.", ""), "seconds": T0, "L": L, "M": M, "taps": 2 * Kt,
               "track_bytes": data.numel() * data.element_size()}
        wav = audio.resample(audio.PcmAudio(data, sr, **kw))
        rec["n_out"] = int(wav.shape[1])
        rec["waveform_fp32_bytes"] = int(wav.shape[1]) * 4
        moved = data.shape[1 if planar else 0] * data.element_size() + int(wav.shape[1]) * 4
        for res, d in src.items():
            pcm = audio.PcmAudio(d, sr, **kw)
            ms, st = [], {}
            for r in range(args.warmup + args.steps):
                t, out = timed_ms(lambda: audio.resample(pcm, stats=st))
                assert torch.equal(out, wav)
                if r >= args.warmup:
                    ms.append(t)
            med = statistics.median(ms)
            rec["resample_" + res] = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                      "gb_per_s": round(moved / (med * 1e-3) / 1e9, 1), "uploaded_bytes": st["uploaded_bytes"],
                                      "uploaded_over_waveform_fp32": round(st["uploaded_bytes"] / (int(wav.shape[1]) * 4), 3)}
        routes = {"wav": lambda: encode({"audio_wav": wav}),
                  "pcm_device": lambda: encode({"audio_pcm": audio.PcmAudio(src["device"], sr, **kw)}),
                  "pcm_pinned": lambda: encode({"audio_pcm": audio.PcmAudio(src["pinned"], sr, **kw)})}
        ms, outs = {n: [] for n in routes}, {}
        for r in range(args.warmup + args.steps):
            for n, fn in routes.items():
                t, outs[n] = timed_ms(fn)
                if r >= args.warmup:
                    ms[n].append(t)
        same = all(torch.equal(outs[n], outs["wav"]) for n in routes)
        assert same, "the PCM and waveform routes' outputs differ"
        rec["step"] = {n: {"ms_per_step": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
                       for n, v in ms.items()}
        rec["step"]["spread_ms"] = round(max(ms["wav"]) - min(ms["wav"]), 3)
        rec["step"]["pcm_device_minus_wav_ms"] = round(statistics.median(ms["pcm_device"]) - statistics.median(ms["wav"]), 3)
        rec["step"]["pcm_pinned_minus_wav_ms"] = round(statistics.median(ms["pcm_pinned"]) - statistics.median(ms["wav"]), 3)
        rec["step"]["outputs_bit_equal"] = same
        outs.clear()
        host = src["pinned"].numpy()
        x = host[0] if planar else host[:, 0]
        t0 = time.perf_counter()
        xf = x.astype(np.float32) / np.float32(32768.0) if as_int16 else np.ascontiguousarray(x)
        y = scipy.signal.resample_poly(xf, L, M)
        rec["host_resample_poly"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "n_out": int(len(y)), "threads": 1}
        tracks.append(rec)
        print("[bench_pcm_audio] %s done" % name, file=sys.stderr, flush=True)
        del data, src, wav, routes, host, x, xf, y
        torch.cuda.empty_cache()
    res = {"tool": "bench_pcm_audio", "device": torch.cuda.get_device_name(dev), "K": K, "H": H,
           "setting": {"dtype": "float16", "tdc_tower_dtype": "bfloat16", "tdc_tower_res_dtype": "float16"},
           "frames_in": T0, "frame_cap": args.cap, "steps": args.steps, "warmup": args.warmup, "tracks": tracks}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
