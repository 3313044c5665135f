"""GPU (-m gpu): the multi-prompt compressor path on the tiny reference-fixture model - the engine whose
towers run head dim 16 / 12 and whose Q-Former runs K = 4 - and at the boundary (`config.tdc_batch_prompts`).  Every comparison
is torch.equal against the single-prompt calls."""
import numpy as np
import pytest
import torch

import synth
from test_hip_boundary import loaded_lm
from test_hip_pipeline import make_encoder
from util import load_fixture, pipeline_cfg

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y)
        else:
            assert x == y


@pytest.fixture(scope="module")
def fx():
    W, o = load_fixture("pipeline_T40_audio.npz")
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    wins = synth.beats_windows(torch.from_numpy(o["audio_wav"].astype(np.float32)))
    pid = [int(i) for i in o["prompt_ids"]]
    size = tuple(int(v) for v in o["image_size"])
    return W, o, vid, wins, pid, size


def _strip(info):
    return {k: v for k, v in info.items() if k not in ("prompts", "cache")}


# ------------------------------------------------------------------------------------------------ engine, small fixture
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("audio", [False, True])
def test_small_engine_encode_video_prompts(fx, dtype, audio):
    """encode_video_prompts == [encode_video(p)] with and without audio, a prompt whose budget_text_len shrinks the a1 selection
    (30 of 40 frames: its own group), P above max_prompts, every padding limit, a cold and a warm cache with per-prompt info
    equality, and xattn_mode 0 / 2 with the infos showing which path ran"""
    from tdc_video_amd import pipeline
    W, o, vid, wins, pid, size = fx
    enc = make_encoder(W, pipeline_cfg(o), dtype)
    vs, vd = vid.cuda(), (vid + 0.01).cuda()
    au = {"beats_windows": wins} if audio else None
    cfg = enc.cfg
    # (tokenizer_model_max_length - btl - inference_max_length) // tokens_per_frame == 30 frames
    tpf = (144 + (50 if cfg.get("audio_input", False) else 0) + enc.K * 7) // 8
    btl_long = cfg["tokenizer_model_max_length"] - cfg.get("inference_max_length", 16) - 30 * tpf
    assert len(pipeline.frame_indices(cfg, 40, btl_long, 224)) == 30 and len(pipeline.frame_indices(cfg, 40, 9, 224)) == 40
    qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid),
          dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:]),
          dict(budget_text_len=btl_long, n_text_tokens=8, prompt_ids=pid[:6] + pid[-1:]),
          dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid[1:6] + pid[-1:]),
          dict(budget_text_len=9, n_text_tokens=5000, prompt_ids=pid[:2] + pid[-1:])]           # a clipped emission

    def singles(cache=None):
        want, winfo = [], []
        for q in qs:
            winfo.append({})
            kw = {} if cache is None else {"cache": cache}
            want.append(enc.encode_video(vs, vd, size, q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"], audio=au,
                                         info=winfo[-1], **kw))
        return want, winfo
    want, winfo = singles()
    others = [0, 1, 3, 4]
    for max_prompts, pad in ((8, 1.0), (2, 1.0), (8, 0.25), (8, 0.0)):
        infos = [{} for _ in qs]
        got = enc.encode_video_prompts(vs, vd, size, qs, audio=au, infos=infos, max_prompts=max_prompts, pad_fraction=pad)
        for p in range(len(qs)):
            assert torch.equal(got[p], want[p]), (max_prompts, pad, p)
            assert _strip(infos[p]) == _strip(winfo[p]), (max_prompts, pad, p)
        sizes = [i["prompts"]["group_size"] for i in infos]
        assert max(sizes) <= max_prompts
        if pad == 1.0:
            assert [sizes[p] for p in others] == [min(4, max_prompts)] * 4
        if pad == 0.0:                                            # only equal lengths share a pass: prompts 1 and 3
            assert sizes == [1, 2, 1, 2, 1]
        assert sizes[2] == 1 and len(infos[2]["frame_indices"]) == 30                        # the a1 change took effect
        assert infos[2]["prompts"]["group"] not in {infos[p]["prompts"]["group"] for p in others}
    # a cold and a warm frame cache: per-prompt info as the cached single calls give it
    wcache = enc.new_cache(1 << 30)
    singles(wcache)
    want_c, winfo_c = singles(wcache)                             # warm single calls
    cache = enc.new_cache(1 << 30)
    for warm in (False, True):
        infos = [{} for _ in qs]
        got = enc.encode_video_prompts(vs, vd, size, qs, audio=au, infos=infos, cache=cache)
        for p in range(len(qs)):
            assert torch.equal(got[p], want[p]) and torch.equal(got[p], want_c[p]), (warm, p)
            assert _strip(infos[p]) == _strip(winfo_c[p]), (warm, p)
            assert infos[p]["cache"]["bypassed"] is False and infos[p]["cache"]["frames"] == len(infos[p]["frame_indices"])
        if warm:
            for p in range(len(qs)):
                assert infos[p]["cache"]["frames_encoded"] == 0 and infos[p]["cache"] == winfo_c[p]["cache"], p
    # xattn_mode 0: the shared pass; 2: one pass per prompt wherever the whole-block kernel takes the shape
    old = getattr(enc, "xattn_mode", 1)
    try:
        for mode in (0, 2):
            enc.xattn_mode = mode
            w, wi = singles()
            infos, oks = [{} for _ in qs], []
            ok = enc.multi_prompt_ok
            enc.multi_prompt_ok = lambda nf: oks.append(ok(nf)) or oks[-1]
            try:
                g = enc.encode_video_prompts(vs, vd, size, qs, audio=au, infos=infos, max_prompts=8, pad_fraction=1.0)
            finally:
                del enc.multi_prompt_ok
            for p in range(len(qs)):
                assert torch.equal(g[p], w[p]), (mode, p)
                assert _strip(infos[p]) == _strip(wi[p]), (mode, p)
            sizes = [i["prompts"]["group_size"] for i in infos]
            assert oks and len(set(oks)) == 1
            assert [sizes[p] for p in others] == ([4] * 4 if oks[0] else [1] * 4), (mode, oks)
            assert oks[0] or mode == 2
    finally:
        enc.xattn_mode = old


# ------------------------------------------------------------------------------------------------------------- the boundary
def _batch(fx, audio):
    """bsz = 4: the fixture video three times (samples 0, 1, 3; its own prompt each, one sample a token shorter and padded) and
    one other video (sample 2)"""
    W, o, vid, wins, pid, size = fx
    other = (vid[3:30].flip(0) * 0.7).contiguous()
    vids = [vid, vid.clone(), other, vid]
    ids = torch.from_numpy(o["input_ids"])
    ids2 = torch.cat([ids[:, :-2], ids[:, -1:], torch.zeros(1, 1, dtype=ids.dtype)], 1)      # one token shorter + a pad
    am = torch.ones(4, ids.shape[1], dtype=torch.long)
    am[1, -1] = 0
    au = (lambda: {"beats_windows": [w.clone() for w in wins]}) if audio else (lambda: None)
    args = dict(images=[vids, [v + 0.01 for v in vids]], image_sizes=[size] * 4, video_indices=[None] * 4,
                prompts=[pid, pid[:5] + pid[-1:], pid[:4] + pid[-1:], pid[:3] + pid[-1:]],
                audios=[au(), au(), None, au()])
    return torch.cat([ids, ids2, ids, ids]), am, args


def _call(lm, ids, am, args):
    pos = torch.arange(ids.shape[1])[None].repeat(ids.shape[0], 1)
    return lm.prepare_inputs_labels_for_multimodal(ids, pos, am, None, ids.clone(), args["images"],
                                                   image_sizes=args["image_sizes"], video_indices=args["video_indices"],
                                                   prompts=args["prompts"], audios=args["audios"])


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("audio", [False, True])
@pytest.mark.parametrize("cache_bytes", [0, 1 << 30])
def test_mixin_same_video_samples_share_one_pass(fx, side, audio, cache_bytes):
    W, o = fx[0], fx[1]
    ids, am, args = _batch(fx, audio)
    lm = loaded_lm(W, o, tokenizer_padding_side=side, audio_input=True, tdc_video_cache_bytes=cache_bytes)
    off = _call(lm, ids, am, args)
    m = lm.get_model()
    m.tdc_video_cache_clear()
    m.config.tdc_batch_prompts = 8
    eng = m.tdc_engine()
    seen, towers = [], []
    multi, tower = eng.encode_video_prompts, eng.tower

    def spy(px_s, px_d, image_size, prompts, **kw):
        r = multi(px_s, px_d, image_size, prompts, **kw)
        seen.append([dict(i) for i in kw["infos"]])
        return r

    def tspy(name, px):
        towers.append((name, px.shape[0]))
        return tower(name, px)
    eng.encode_video_prompts, eng.tower = spy, tspy
    on = _call(lm, ids, am, args)
    _same(on, off)
    assert len(seen) == 1 and len(seen[0]) == 3                  # samples 0, 1, 3 in one call; sample 2 on its own
    assert [i["prompts"]["group_size"] for i in seen[0]] == [3, 3, 3]
    assert len({i["prompts"]["group"] for i in seen[0]}) == 1
    for name in ("dino", "siglip"):                              # each video through the towers once
        assert sum(n for t, n in towers if t == name) == 40 + 27, towers
    assert len(on[8]) == 3 * 40 + 27
    assert len({int(v) for v in on[2].sum(1)}) > 1               # the samples differ in length: padding is exercised


def test_mixin_key_validation_and_forbidden_combinations(fx):
    W, o = fx[0], fx[1]
    ids, am, args = _batch(fx, False)
    for over, names in ((dict(tdc_batch_prompts=8, tdc_batch_frames=512), ("tdc_batch_prompts", "tdc_batch_frames")),
                        (dict(tdc_batch_prompts=8, tdc_shard_frames=True), ("tdc_batch_prompts", "tdc_shard_frames")),
                        (dict(tdc_batch_prompts=-1), ("tdc_batch_prompts",)),
                        (dict(tdc_batch_prompts=8, tdc_prompt_pad_fraction=1.5), ("tdc_prompt_pad_fraction",))):
        lm = loaded_lm(W, o, audio_input=True, **over)
        with pytest.raises(ValueError) as ei:
            _call(lm, ids, am, args)
        assert all(n in str(ei.value) for n in names), str(ei.value)
