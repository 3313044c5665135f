"""GPU (-m gpu): the batched encode (`config.tdc_batch_frames`, VideoEncoder.encode_batch) on the tiny reference-fixture model.
Every comparison is torch.equal against the per-sample path: the towers do not depend on their batch, the similarity of a
pair is a fixed-order reduction and the connector works per frame, so a batch must change no bit.  The launch-count test
checks that a batch of B samples runs one tower pass per tower over the group's frames, not B passes."""
import numpy as np
import pytest
import torch

import synth
from test_hip_boundary import loaded_lm
from test_hip_pipeline import MIXED, make_encoder
from util import load_fixture, pipeline_cfg

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y)
        else:
            assert x == y


def _fixture_video(o):
    return torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))


def _spy(eng):
    """count VideoEncoder.tower calls per tower and encode_batch calls (sizes) on this engine"""
    calls, batches = {}, []
    tower, batch = eng.tower, eng.encode_batch

    def t(name, px):
        calls[name] = calls.get(name, 0) + 1
        return tower(name, px)

    def b(samples, *a, **k):
        batches.append(len(samples))
        return batch(samples, *a, **k)
    eng.tower, eng.encode_batch = t, b
    return calls, batches


def _video_batch():
    """three videos of different lengths (40 with BEATs audio, 27, 12: no Q-Former), their own prompts, one padded"""
    W, o = load_fixture("pipeline_T40_audio.npz")
    vid = _fixture_video(o)
    vids = [vid, vid[3:30].flip(0).contiguous(), (vid[5:17] * 0.7).contiguous()]
    ids = torch.from_numpy(o["input_ids"])
    ids2 = torch.cat([ids[:, :-2], ids[:, -1:], torch.zeros(1, 1, dtype=ids.dtype)], 1)      # one token shorter + a pad
    am = torch.ones(3, ids.shape[1], dtype=torch.long)
    am[1, -1] = 0
    pid = [int(i) for i in o["prompt_ids"]]
    wins = synth.beats_windows(torch.from_numpy(o["audio_wav"].astype(np.float32)))
    size = tuple(int(v) for v in o["image_size"])
    args = dict(images=[vids, [v + 0.01 for v in vids]], image_sizes=[size] * 3, video_indices=[None] * 3,
                prompts=[pid, pid[:5] + pid[-1:], pid[:3] + pid[-1:]], audios=[{"beats_windows": wins}, None, None])
    all_ids = torch.cat([ids, ids2, ids])
    return W, o, all_ids, am, args


def _call(lm, ids, am, args):
    pos = torch.arange(ids.shape[1])[None].repeat(ids.shape[0], 1)
    return lm.prepare_inputs_labels_for_multimodal(ids, pos, am, None, ids.clone(), args["images"],
                                                   image_sizes=args["image_sizes"], video_indices=args["video_indices"],
                                                   prompts=args["prompts"], audios=args["audios"])


@pytest.mark.parametrize("side", ["right", "left"])
def test_mixin_batch_of_videos_equals_per_sample(side):
    W, o, ids, am, args = _video_batch()
    lm = loaded_lm(W, o, tokenizer_padding_side=side, audio_input=True)
    off = _call(lm, ids, am, args)
    lm.get_model().config.tdc_batch_frames = 512
    calls, batches = _spy(lm.get_model().tdc_engine())
    on = _call(lm, ids, am, args)
    _same(on, off)
    assert batches == [3] and calls == {"dino": 1, "siglip": 1}
    assert len(on[8]) == 40 + 27 + 12
    n = [int(v) for v in on[2].sum(1)]
    assert len(set(n)) > 1                                   # the samples differ in length: padding is exercised


def test_mixin_batch_of_single_images_mixed_sizes():
    W, o = load_fixture("pipeline_T10_land.npz")
    lm = loaded_lm(W, o)
    vid = _fixture_video(o)
    ims = torch.stack([vid[1], vid[4] * 0.5, vid[7], vid[9] + 0.1])
    sizes = [(384, 384), (360, 640), (640, 360), (200, 200)]
    ids = torch.from_numpy(o["input_ids"]).repeat(4, 1)
    args = dict(image_sizes=sizes)
    off = lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [ims, ims + 0.01], **args)
    lm.get_model().config.tdc_batch_frames = 16
    calls, batches = _spy(lm.get_model().tdc_engine())
    on = lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [ims, ims + 0.01], **args)
    _same(on, off)
    assert batches == [4] and calls == {"dino": 1, "siglip": 1}
    assert len({tuple(s) for s in on[8]}) == 3               # square / landscape / portrait rows differ per frame


def test_ceiling_below_one_sample():
    """a ceiling of 39 frames: the 40-frame sample runs alone on the per-sample path, the 27 + 12 frames as one group"""
    W, o, ids, am, args = _video_batch()
    lm = loaded_lm(W, o, audio_input=True)
    off = _call(lm, ids, am, args)
    lm.get_model().config.tdc_batch_frames = 39
    calls, batches = _spy(lm.get_model().tdc_engine())
    on = _call(lm, ids, am, args)
    _same(on, off)
    assert batches == [2] and calls == {"dino": 2, "siglip": 2}


def test_one_tower_pass_per_tower_launch_count():
    """under ops.profile_start/stop the batched call's tower GEMMs are exactly one pass of each tower over the group's
    frames (same launches, same M), where the per-sample path issues one pass per sample"""
    from tdc_video_amd import ops, pipeline
    W, o, ids, am, args = _video_batch()
    lm = loaded_lm(W, o, audio_input=True)
    eng = lm.get_model().tdc_engine()
    m = lm.get_model()
    cap = m.tdc_frame_cap()
    plans = [pipeline.frame_indices(eng.cfg, v.shape[0], lm._budget_text_len(ids[i]), cap)
             for i, v in enumerate(args["images"][0])]
    px_s = pipeline.gather_frames(args["images"][0], plans, eng.dev)
    px_d = pipeline.gather_frames(args["images"][1], plans, eng.dev)
    eng.two_streams = False

    def gemms(fn):
        torch.cuda.synchronize()
        ops.profile_start()
        fn()
        torch.cuda.synchronize()
        return [(r["M"], r["N"], r["K"]) for r in ops.profile_stop() if r["kind"] == "gemm"]
    one_pass = gemms(lambda: (eng.tower("dino", px_d), eng.tower("siglip", px_s)))
    n = len(one_pass)
    assert n > 0 and sum(mm for mm, _, _ in one_pass) > 0
    m.config.tdc_batch_frames = 512
    on = gemms(lambda: _call(lm, ids, am, args))
    assert sorted(on[:n]) == sorted(one_pass)                # both towers, once, over all 79 frames
    m.config.tdc_batch_frames = 0
    off = gemms(lambda: _call(lm, ids, am, args))
    assert sorted(off[:n]) != sorted(one_pass)               # the per-sample path: three smaller passes


def _near_tied_video(enc, shape, eps):
    """T = 52 frames whose adjacent pairs are exact duplicates (similarity 1), hard cuts between unrelated images, and the pair
    (X, Y) twice: two EXACTLY equal similarities at the decisive rank (24 / 25 of 51) - the selection band of the refinement.
    Y's distance to X is chosen so that the cuts lie below and the duplicates above the tie by more than 2 eps."""
    from tdc_video_amd import segment as seg
    dev = enc.dev
    g = torch.Generator(device=dev).manual_seed(91)
    img = lambda: torch.rand(shape, device=dev, generator=g) * 2 - 1
    X, Z = img(), img()
    R = [img() for _ in range(22)]
    for a in np.linspace(0.05, 1.2, 24):
        Y = float(np.cos(a)) * X + float(np.sin(a)) * Z
        frames = [X, X, Y, Y] + [r for r in R[:11] for _ in (0, 1)] + [X, X, Y, Y] + [r for r in R[11:] for _ in (0, 1)]
        vid = torch.stack(frames)
        sims = enc.sims_tensor(enc.tower("dino", vid), vid.shape[0]).cpu().tolist()
        band = seg.selection_band(sims, 24, eps)
        if band == [1, 27] and seg.band_allowed(band, len(sims) + 1, enc.selection_max_fraction):
            return vid
    raise AssertionError("no near-tied construction found")


def test_selection_refinement_inside_a_batch():
    W, o = load_fixture("pipeline_T40.npz")
    enc = make_encoder(W, pipeline_cfg(o), MIXED)           # bf16 DINOv2 operands: the refinement is on
    assert enc.selection_eps is not None
    enc.selection_eps = 1e-4
    vid = _fixture_video(o)
    near = _near_tied_video(enc, tuple(vid.shape[1:]), enc.selection_eps)
    size = tuple(int(v) for v in o["image_size"])
    pid = [int(i) for i in o["prompt_ids"]]
    samples = [dict(px_siglip=v.cuda(), px_dino=(v + 0.01).cuda() if v is not near else v, image_size=size,
                    budget_text_len=9, n_text_tokens=8, prompt_ids=pid, audio=None, video_index=None, splice=None)
               for v in (vid, near, vid[:20])]
    want, wi = [], []
    for s in samples:
        wi.append({})
        want.append(enc.encode_video(s["px_siglip"], s["px_dino"], size, 9, 8, pid, info=wi[-1]))
    assert wi[1].get("refined_pairs") == [1, 27], wi[1]
    infos = [{} for _ in samples]
    got = enc.encode_batch(samples, infos=infos)
    for g_, w, i, w_i in zip(got, want, infos, wi):
        assert torch.equal(g_, w)
        assert i == w_i


def test_engine_encode_batch_equals_encode_video():
    """VideoEncoder.encode_batch with info dicts == encode_video per sample (BEATs-window audio on one sample, a1 cut on
    another, a 12-frame clip without Q-Former), under both tower stream settings"""
    W, o = load_fixture("pipeline_T40_audio.npz")
    enc = make_encoder(W, pipeline_cfg(o), torch.float16)
    vid = _fixture_video(o).cuda()
    size = tuple(int(v) for v in o["image_size"])
    pid = [int(i) for i in o["prompt_ids"]]
    wins = synth.beats_windows(torch.from_numpy(o["audio_wav"].astype(np.float32)))
    samples = [dict(px_siglip=vid, px_dino=vid + 0.01, image_size=size, budget_text_len=9, n_text_tokens=8, prompt_ids=pid,
                    audio={"beats_windows": wins}, video_index=None, splice=None),
               dict(px_siglip=vid.flip(0).contiguous(), px_dino=vid.flip(0) + 0.01, image_size=size, budget_text_len=9,
                    n_text_tokens=5, prompt_ids=pid[:4], audio=None, video_index=None, splice=None),
               dict(px_siglip=vid[:12].cpu(), px_dino=(vid[:12] + 0.01).cpu(), image_size=size, budget_text_len=9,
                    n_text_tokens=8, prompt_ids=None, audio=None, video_index=None, splice=None)]
    cap = 33                                                  # a1 keeps 33 of the 40 frames
    want, wi = [], []
    for s in samples:
        wi.append({})
        want.append(enc.encode_video(s["px_siglip"].cuda(), s["px_dino"].cuda(), size, s["budget_text_len"],
                                     s["n_text_tokens"], s["prompt_ids"], audio=s["audio"], frame_cap=cap, info=wi[-1]))
    assert len(wi[0]["frame_indices"]) == 33
    for two in (False, True):
        enc.two_streams = two
        infos = [{} for _ in samples]
        got = enc.encode_batch(samples, frame_cap=cap, infos=infos)
        for g_, w, i, w_i in zip(got, want, infos, wi):
            assert torch.equal(g_, w)
            assert i == w_i
