"""CPU: encode from decoded uint8 frames (encode.*_frames_*) on the engine double of test_features, whose
`pixels_from_frames` is the oracle's process_frames: a1 runs first, only the kept frames are preprocessed, and everything
behind the pixels must be what the pixel path gives on the pixels of ALL frames - tokens, info, audio seconds, cache keys.
Plus the host-side checks of preprocess.preprocess_selected and the mixin's `config.tdc_frame_inputs`."""
import os
import sys

import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import encode, pipeline, preprocess
from tdc_video_amd.cache import FrameCache
from test_features import FeatureEngine, FeatureMixinEngine, Untouchable, feature_lm, same_tuple
from test_host_logic import build_stub_lm, tiny_config
from test_video_cache import _CacheMixin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import preprocess_oracle as po  # noqa: E402

SIZE = (4, 6)                                                     # the frames' own (H, W): the default image_size
TOWERS = (dict(R=2, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)),
          dict(R=2, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)))


def make_frames(T0, seed=5):
    """uint8 [T0, 4, 6, 3]: a new scene every five frames, small changes inside one (so a5 has something to rank)"""
    rng = np.random.RandomState(seed)
    out, base = [], None
    for t in range(T0):
        if t % 5 == 0:
            base = rng.randint(8, 248, (4, 6, 3))
        out.append(np.clip(base + rng.randint(-6, 7, (4, 6, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


class _Frames:
    """pixels_from_frames by the oracle (fp16 values, handed on as fp32 like the double's other pixels); records every idx"""

    def pixels_from_frames(self, frames, idx=None):
        fr = frames.numpy() if torch.is_tensor(frames) else np.asarray(frames)
        if not hasattr(self, "asked"):
            self.asked = []
        self.asked.append(None if idx is None else list(idx))
        kept = fr if idx is None else fr[list(idx)]
        return tuple(torch.from_numpy(po.process_frames(kept, t["R"], t["mean"], t["std"]).astype(np.float32)) for t in TOWERS)


class FrameEngine(_Frames, FeatureEngine):
    pass


class CachedFrameEngine(_Frames, _CacheMixin, FeatureEngine):
    pass


def both(eng, frames, cap=224, audio=None, prompt=(1, 2, 3), btl=4, n_text=4, video_index=None, cache=None):
    """(pixel result on the pixels of ALL frames, its info), (frames result, its info)"""
    ps, pd = _Frames.pixels_from_frames(eng, frames, None)
    eng.asked = []
    wi, gi = {}, {}
    want = pipeline.encode_video_with(eng, ps, pd, SIZE, btl, n_text, list(prompt), audio, cap, None, None, video_index, wi)
    got = encode.encode_frames_with(eng, frames, btl, n_text, list(prompt), audio, cap, None, video_index, gi, cache)
    return (want, wi), (got, gi)


def shared(gi, wi):
    assert set(gi) - set(wi) == {"frames_in", "frames_resized"} and set(wi) <= set(gi)
    assert {k: gi[k] for k in wi} == wi


# ------------------------------------------------------------------------------------------------ bitwise equality
@pytest.mark.parametrize("T0,cap,kept", [(40, 224, 40), (40, 30, 30), (20, 224, 20)])
def test_encode_frames_equals_encode_video(T0, cap, kept):
    eng = FrameEngine(N=5)
    frames = make_frames(T0)
    (want, wi), (got, gi) = both(eng, frames, cap)
    assert torch.equal(got, want)
    shared(gi, wi)
    assert gi["frames_in"] == T0 and gi["frames_resized"] == kept == len(gi["frame_indices"])
    # the engine was asked for exactly the a1 indices, once
    assert eng.asked == [encode.frame_indices(eng.cfg, T0, 4, cap)] and len(eng.asked[0]) == kept
    assert gi["seg_indices"] == list(range(20)) if T0 == 20 else len(gi["seg_indices"]) == 24
    # a torch tensor and the explicit image_size give the same
    again = encode.encode_frames_with(eng, torch.from_numpy(frames), 4, 4, [1, 2, 3], frame_cap=cap, image_size=SIZE)
    assert torch.equal(again, want)


def test_encode_frames_with_audio_and_video_index():
    eng = FrameEngine(N=5, audio_input=True)
    g = torch.Generator().manual_seed(2)
    audio = {"per_second": torch.rand(62, 2, eng.H, generator=g)}
    frames = make_frames(31)
    for cap, vi in ((224, None), (17, None), (224, [1, 0] * 31), (17, [1, 0] * 31)):
        (want, wi), (got, gi) = both(eng, frames, cap, audio=audio if vi else {"per_second": audio["per_second"][:31]},
                                     video_index=vi)
        assert torch.equal(got, want)
        shared(gi, wi)
        assert len(gi["frame_indices"]) == min(cap, 31) and gi["frame_indices"][-1] >= 29      # the video's own frame numbers


def test_encode_frames_prompts_equals_per_prompt_calls_with_one_front():
    eng = FrameEngine(K=3, H=8, N=5, max_len=400, max_num_segments=6)
    frames = make_frames(40)
    prompts = [dict(budget_text_len=4, n_text_tokens=4, prompt_ids=[5]),
               dict(budget_text_len=4, n_text_tokens=30, prompt_ids=[7, 8, 9, 10]),
               dict(budget_text_len=4, n_text_tokens=60, prompt_ids=list(range(20, 29)))]
    infos = [{} for _ in prompts]
    eng.asked, calls = [], eng.tower_calls
    got = encode.encode_frames_prompts_with(eng, frames, prompts, frame_cap=30, infos=infos, pad_fraction=1.0)
    kept = encode.frame_indices(eng.cfg, 40, 4, 30)               # the token budget keeps fewer than the cap
    assert eng.asked == [kept] and len(kept) < 30 and eng.tower_calls == calls + 2 and eng.multi_calls == 1
    for p, pr in enumerate(prompts):
        wi = {}
        want = encode.encode_frames_with(eng, frames, pr["budget_text_len"], pr["n_text_tokens"], pr["prompt_ids"], frame_cap=30,
                                         info=wi)
        assert torch.equal(got[p], want), p
        assert {k: v for k, v in infos[p].items() if k != "prompts"} == wi
    ps, pd = _Frames.pixels_from_frames(eng, frames, None)
    want_px = pipeline.encode_video_prompts_with(eng, ps, pd, SIZE, prompts, frame_cap=30, pad_fraction=1.0)
    assert all(torch.equal(a, b) for a, b in zip(got, want_px))


@pytest.mark.parametrize("slab", [7, 40, 256])
def test_export_features_from_frames_equals_export_features(slab):
    eng = FrameEngine(N=5)
    frames = make_frames(40)
    want = encode.export_features_with(eng, *_Frames.pixels_from_frames(eng, frames, None), SIZE)
    eng.asked = []
    got = encode.export_features_from_frames_with(eng, frames, slab=slab)
    assert torch.equal(got.siglip, want.siglip) and torch.equal(got.dino, want.dino)
    assert got.image_size == want.image_size == SIZE and got.signature == want.signature and got.frames == 40
    assert [i for a in eng.asked for i in a] == list(range(40)) and len(eng.asked) == -(-40 // slab)      # every frame, once
    # ... and the set encodes to what the frames do when a1 keeps every frame
    assert torch.equal(encode.encode_features_with(eng, got, 4, 4, [1, 2]), encode.encode_frames_with(eng, frames, 4, 4, [1, 2]))
    with pytest.raises(ValueError, match="store"):
        encode.export_features_from_frames_with(eng, frames, store="f8")


def test_one_image():
    eng = FrameEngine(N=5)
    frames = make_frames(3)
    ps, pd = _Frames.pixels_from_frames(eng, frames[1:2], None)
    X, sizes = eng.connector(eng.tower("siglip", ps), eng.tower("dino", pd), 1, [SIZE])
    info = {}
    got = encode.encode_frames_with(eng, frames[1:2], None, 4, None, info=info, image=True)
    assert torch.equal(got, X[:, :eng.H]) and info == {"final_size": sizes, "frames_in": 1, "frames_resized": 1}
    with pytest.raises(ValueError, match="one frame"):
        encode.encode_frames_with(eng, frames, None, 4, None, image=True)


def test_dropped_frames_are_never_read():
    """the frames a1 drops overwritten with other bytes: the same tokens"""
    eng = FrameEngine(N=5)
    frames = make_frames(40)
    want = encode.encode_frames_with(eng, frames, 4, 4, [1, 2], frame_cap=30)
    kept = set(encode.frame_indices(eng.cfg, 40, 4, 30))
    other = frames.copy()
    for t in range(40):
        if t not in kept:
            other[t] = 255 - other[t]
    assert len(kept) == 30 and not np.array_equal(other, frames)
    assert torch.equal(encode.encode_frames_with(eng, other, 4, 4, [1, 2], frame_cap=30), want)
    other[sorted(kept)[3]] ^= 1                                   # a kept frame does count
    assert not torch.equal(encode.encode_frames_with(eng, other, 4, 4, [1, 2], frame_cap=30), want)


# ------------------------------------------------------------------------------------------------ the frame cache
def test_frame_cache_serves_frames_and_pixels_alike():
    """through a FrameCache: the uncached bits, audio by the video's own seconds (a1 does not run again on the selected set),
    every kept frame reused on the second call, and a video asked first through pixels hits when asked through frames"""
    eng = CachedFrameEngine(N=5, audio_input=True)
    frames = make_frames(45)
    g = torch.Generator().manual_seed(2)
    audio = {"per_second": torch.rand(45, 2, eng.H, generator=g)}
    c = FrameCache(1 << 30)
    (want, wi), (got, gi) = both(eng, frames, 33, audio=audio, cache=c)
    assert torch.equal(got, want)
    assert gi["cache"]["frames_encoded"] == 33 and {k: gi[k] for k in wi} == wi
    i2 = {}
    again = encode.encode_frames_with(eng, frames.copy(), 4, 4, [1, 2, 3], audio, 33, info=i2, cache=c)
    assert torch.equal(again, want)
    assert i2["cache"]["frames_encoded"] == 0 and i2["cache"]["frames_hit"] == i2["cache"]["frames"] == 33
    assert i2["frame_indices"] == wi["frame_indices"] and i2["frames_resized"] == 33
    # pixels first, frames second
    c2 = FrameCache(1 << 30)
    ps, pd = _Frames.pixels_from_frames(eng, frames, None)
    first = pipeline.encode_video_with(eng, ps, pd, SIZE, 4, 4, [1, 2, 3], audio, 33, cache=c2)
    i3 = {}
    assert torch.equal(encode.encode_frames_with(eng, frames, 4, 4, [1, 2, 3], audio, 33, info=i3, cache=c2), first)
    assert i3["cache"]["frames_encoded"] == 0 and i3["cache"]["frames_hit"] == 33
    # a budget below one video: bypassed, the uncached bits
    i4 = {}
    small = encode.encode_frames_with(eng, frames, 4, 4, [1, 2, 3], audio, 33, info=i4, cache=FrameCache(64))
    assert torch.equal(small, want) and i4["cache"]["bypassed"]


# ------------------------------------------------------------------------------------------------ host-side checks
def test_indices_and_frames_are_checked_on_the_host_before_any_launch():
    frames = make_frames(6)
    for idx in ([0, 6], [-1, 2], [2, 1], [1, 1], []):
        with pytest.raises(ValueError, match="idx"):
            preprocess.preprocess_selected(frames, idx, TOWERS)   # no GPU here: raised before one would be needed
    assert preprocess.check_indices([0, 2, 5], 6) == [0, 2, 5] and preprocess.check_indices(None, 6) is None
    assert preprocess.check_indices(list(range(6)), 6) is None    # every frame kept: the frames stay where they lie
    for bad in (frames.astype(np.int32), frames[..., :2], frames[0], np.zeros((0, 4, 6, 3), np.uint8)):
        with pytest.raises(ValueError, match="frames"):
            preprocess.preprocess_selected(bad, None, TOWERS)
    assert preprocess.check_frames(frames[:, ::-1]).shape == (6, 4, 6, 3)          # a flipped view is copied, not refused
    assert preprocess.check_frames(list(frames)).shape == (6, 4, 6, 3)
    with pytest.raises(ValueError, match="slab"):
        preprocess.preprocess_selected(frames, None, TOWERS, slab=0)
    assert encode.frames_size(frames) == (6, (4, 6)) and encode.frames_size(list(frames), (8, 9)) == (6, (8, 9))


# ------------------------------------------------------------------------------------------------ the mixin
def test_config_key_validates_and_names_itself():
    m = lambda **kw: build_stub_lm(tiny_config(**kw)).get_model()
    assert m().tdc_frame_inputs() is False and m(tdc_frame_inputs=None).tdc_frame_inputs() is False
    assert m(tdc_frame_inputs=False).tdc_frame_inputs() is False and m(tdc_frame_inputs=True).tdc_frame_inputs() is True
    for bad in (1, 0, "yes", 2.5):
        with pytest.raises(ValueError, match="tdc_frame_inputs"):
            m(tdc_frame_inputs=bad).tdc_frame_inputs()
    assert m(tdc_frame_inputs=True, tdc_video_cache_bytes=1 << 30).tdc_frame_inputs() is True
    assert m(tdc_frame_inputs=False, tdc_batch_frames=512).tdc_frame_inputs() is False


def call(lm, images, n=1, prompts=None):
    ids = torch.tensor([[11, 12, -200, 13, 14, 15]] * n)
    with torch.inference_mode():
        return lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, images, image_sizes=[SIZE] * n,
                                                       video_indices=[None] * n, prompts=prompts or [[1, 2]] * n,
                                                       audios=[None] * n)


@pytest.mark.parametrize("other,v", [("tdc_feature_inputs", True), ("tdc_shard_frames", True), ("tdc_batch_frames", 512),
                                     ("tdc_shard_cache_bytes", 1 << 30), ("tdc_batch_prompts", 4)])
def test_forbidden_combinations_raise_before_any_engine_call(other, v):
    lm = feature_lm(tdc_frame_inputs=True, **{other: v})
    lm.get_model()._tdc_encoder = Untouchable()
    with pytest.raises(ValueError) as ei:
        call(lm, [[torch.from_numpy(make_frames(30))], None])
    assert "tdc_frame_inputs" in str(ei.value) and other in str(ei.value)


class FrameMixinEngine(_Frames, FeatureMixinEngine):
    def encode_frames(self, frames, *a, **kw):
        return encode.encode_frames_with(self, frames, *a, **kw)


def test_mixin_frame_inputs_give_the_pixel_calls_tuple():
    vids = [make_frames(90), make_frames(30, seed=9)]
    lm = feature_lm()
    eng = lm.get_model()._tdc_encoder = FrameMixinEngine(K=3, H=8)
    px = [_Frames.pixels_from_frames(eng, v, None) for v in vids]
    want = call(lm, [[p[0] for p in px], [p[1] for p in px]], 2, [[1, 2], [3, 4, 5]])
    lm.get_model().config.tdc_frame_inputs = True
    eng.asked = []
    same_tuple(call(lm, [[torch.from_numpy(v) for v in vids], None], 2, [[1, 2], [3, 4, 5]]), want)
    assert [len(a) for a in eng.asked] == [37, 30] and len(want[8]) == 37 + 30          # config.tdc_frame_cap = 37
    same_tuple(call(lm, [list(vids), [None, None]], 2, [[1, 2], [3, 4, 5]]), want)      # numpy arrays, images[1] ignored
    # single images: one uint8 [bsz, H, W, 3] tensor
    ims = make_frames(3, seed=11)
    lm.get_model().config.tdc_frame_inputs = False
    ip = _Frames.pixels_from_frames(eng, ims, None)
    want_im = call(lm, [ip[0], ip[1]], 3)
    lm.get_model().config.tdc_frame_inputs = True
    same_tuple(call(lm, [torch.from_numpy(ims), None], 3), want_im)
