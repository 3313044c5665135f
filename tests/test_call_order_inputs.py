"""CPU: the engine call ORDER of the entries test_call_order.py does not reach - the exports, the encode from stored tower
features (lossless and compact), from decoded frames, through the kept cross-attention K/V, and the mixin's branches over the
three input kinds - pinned to tests/golden/call_order_inputs.json as test_call_order.py pins the pixel paths.  The recording
proxy, its argument description and the comparison are test_call_order's; the recorded names are its RECORDED plus the
feature, frame and K/V protocol.  tests/golden/make_call_order_inputs.py wrote the fixture on the commit that introduced this
test; it is not regenerated when the orchestration is reorganised.  Every case asserts the branch it is there for, so that a
case cannot silently record another one."""
import json
import os

import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import encode
from tdc_video_amd.cache import FrameCache, engine_signature
from tdc_video_amd.features import FeatureSet
from test_call_order import FRAME_BYTES, RECORDED, assert_same_log, record
from test_dist_gloo import make_video
from test_feature_store import CompactEngine, CompactMixinEngine
from test_features import SIZE, FeatureEngine, FeatureMixinEngine, NoisyFeatureEngine, call, feature_lm, pixels
from test_frame_inputs import CachedFrameEngine, FrameEngine, FrameMixinEngine, make_frames
from test_gap_sims import GapEngine
from test_kv_cache import ENTRY40, KVEngine
from test_shard_cache import CMixinEngine
from test_video_cache import CFake, _CacheMixin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_order_inputs.json")
NAMES = RECORDED + ("pixels_from_frames", "feature_rows", "decode_feature_rows", "quantize_feature_rows", "gap_sims_tensor",
                    "kv_cache_ok", "kv_alloc", "beats_windows", "audio_tokens")
LEN33 = 16 + 4 + 20 * 33                     # tokenizer_model_max_length at which a 4-token budget keeps 33 frames, a 44-token one 31
# the first two share the a1 selection; the third's text is long enough to leave fewer frames (test_call_order._prompts)
PROMPTS = [dict(budget_text_len=4, n_text_tokens=6, prompt_ids=[1, 2]),
           dict(budget_text_len=4, n_text_tokens=7, prompt_ids=[3, 4, 5]),
           dict(budget_text_len=44, n_text_tokens=8, prompt_ids=[6])]


def rec(eng):
    log = []
    return record(eng, log, NAMES), log


def take(log):
    out = list(log)
    del log[:]
    return out


def names(log):
    return [c[0] for c in log]


class CachedFrameMixinEngine(_CacheMixin, FrameMixinEngine):
    def new_cache(self, nbytes):
        return FrameCache(nbytes, engine_signature(self))


# ------------------------------------------------------------------------------------------------ exports
def _exports():
    out = {}
    ps, pd = pixels(40)
    eng, log = rec(FeatureEngine(N=5))
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    assert fs.store == "f16" and fs.frames == 40
    out["export_lossless_T40"] = take(log)
    eng, log = rec(GapEngine(N=5))
    cs = encode.export_features_with(eng, ps, pd, SIZE, store="e4m3", gaps="auto")
    assert cs.store == "e4m3" and cs.gaps == 2
    out["export_e4m3_gaps_auto_T40"] = take(log)
    eng, log = rec(FrameEngine(N=5))
    fs = encode.export_features_from_frames_with(eng, make_frames(40), slab=16)
    assert fs.frames == 40 and [len(a) for a in eng.asked] == [16, 16, 8]
    out["export_from_frames_T40_slab16"] = take(log)
    eng, log = rec(CompactEngine(N=5))
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    del log[:]
    cs = encode.compact_features_with(eng, fs)
    assert cs.store == "e4m3" and cs.gaps == 1
    out["compact_of_lossless_T40"] = take(log)
    return out


# ------------------------------------------------------------------------------------------------ stored tower features
def _feature_case(eng, T0, cap, make=None):
    """one encode_features_with call over the set make(eng, lossless set of T0 frames) -> (log, info)"""
    eng, log = rec(eng)
    ps, pd = pixels(T0)
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    if make is not None:
        fs = make(eng, fs)
    del log[:]
    info = {}
    encode.encode_features_with(eng, fs, 4, 6, [1, 2], None, cap, None, None, info)
    return log, info


def _features():
    out = {}
    log, info = _feature_case(FeatureEngine(N=5), 40, 30)
    assert len(info["frame_indices"]) == 30 and len(info["seg_indices"]) == 24 and "sims_tensor" in names(log)
    out["features_T40_cap30"] = log
    log, info = _feature_case(FeatureEngine(N=5), 8, 30)
    assert info["frame_indices"] == info["seg_indices"] == list(range(8)) and "sims_tensor" not in names(log)
    out["features_T8_passthrough"] = log
    log, info = _feature_case(GapEngine(N=5), 40, 30, lambda e, fs: encode.compact_features_with(e, fs, gaps="auto"))
    assert info["selection_sims"] == "stored" and len(info["frame_indices"]) == 30 and "sims_tensor" not in names(log)
    out["features_compact_gap_table_T40_cap30"] = log
    log, info = _feature_case(CompactEngine(N=5), 40, 30, encode.compact_features_with)
    assert info["selection_sims"] == "decoded" and len(info["frame_indices"]) == 30
    assert [n for n in names(log) if n in ("sims_tensor", "mark", "fetch")] == ["sims_tensor", "mark", "fetch"]
    out["features_compact_no_table_T40_cap30"] = log
    log, info = _feature_case(NoisyFeatureEngine(N=5), 40, 30)
    assert info["refine_unavailable_pairs"] > 0 and info["refined_pairs"] == [] and "precise_dino" not in names(log)
    out["features_refine_unavailable_T40_cap30"] = log
    eng, log = rec(FeatureEngine(N=5))
    ps, pd = pixels(1)
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    del log[:]
    info = {}
    encode.encode_features_with(eng, fs, None, 6, None, info=info, image=True)
    assert list(info) == ["final_size"] and names(log) == ["connector"]
    out["features_image"] = take(log)
    eng, log = rec(FeatureEngine(K=3, H=8, N=5, max_len=LEN33))
    ps, pd = pixels(40)
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    del log[:]
    infos = [{} for _ in PROMPTS]
    encode.encode_features_prompts_with(eng, fs, PROMPTS, None, 224, None, infos, 8, 1.0)
    assert [len(i["frame_indices"]) for i in infos] == [33, 33, 31]
    assert [i["prompts"]["group_size"] for i in infos] == [2, 2, 1]
    out["features_prompts_3"] = take(log)
    return out


# ------------------------------------------------------------------------------------------------ decoded frames
def _frames():
    out = {}
    for name, T0, kept, segs in (("frames_T40_cap30", 40, 30, 24), ("frames_T8_passthrough", 8, 8, 8)):
        eng, log = rec(FrameEngine(N=5))
        info = {}
        encode.encode_frames_with(eng, make_frames(T0), 4, 6, [1, 2], None, 30, None, None, info)
        assert info["frames_in"] == T0 and info["frames_resized"] == kept == len(info["frame_indices"])
        assert len(info["seg_indices"]) == segs and [len(a) for a in eng.asked] == [kept]
        out[name] = take(log)
    for name, cls in (("frames_image", FrameEngine), ("frames_image_cached", CachedFrameEngine)):
        eng, log = rec(cls(N=5))
        cache = FrameCache(1 << 30, engine_signature(eng)) if name.endswith("cached") else None
        info = {}
        encode.encode_frames_with(eng, make_frames(1), None, 6, None, info=info, cache=cache, image=True)
        assert sorted(info) == ["final_size", "frames_in", "frames_resized"] and eng.asked == [None]
        assert ("fingerprint" in names(log)) == (cache is not None) and (cache is None or len(cache) == 1)
        out[name] = take(log)
    frames = make_frames(40)
    for name, nbytes in (("", 1 << 30), ("_bypass", 2 * FRAME_BYTES)):                 # test_call_order._cached, from frames
        eng, log = rec(CachedFrameEngine(N=5))
        cache = FrameCache(nbytes, engine_signature(eng))
        for state in ("cold", "warm"):
            info = {}
            encode.encode_frames_with(eng, frames, 4, 6, [1, 2], None, 30, None, None, info, cache)
            assert info["cache"]["bypassed"] == bool(name) and info["frames_resized"] == 30
            if not name:
                assert info["cache"]["frames_encoded"] == (30 if state == "cold" else 0)
            assert names(log).count("pixels_from_frames") == 1
            out["frames_cached_T40_cap30_" + state + name] = take(log)
            if name:
                break
    for name, cls in (("frames_prompts_3", FrameEngine), ("frames_prompts_3_cached", CachedFrameEngine)):
        eng, log = rec(cls(K=3, H=8, N=5, max_len=LEN33))
        cache = FrameCache(1 << 30, engine_signature(eng)) if name.endswith("cached") else None
        infos = [{} for _ in PROMPTS]
        encode.encode_frames_prompts_with(eng, frames, PROMPTS, None, 224, None, infos, cache, 8, 1.0)
        assert [len(i["frame_indices"]) for i in infos] == [33, 33, 31] and [len(a) for a in eng.asked] == [33, 31]
        assert [i["prompts"]["group_size"] for i in infos] == [2, 2, 1] and all(("cache" in i) == (cache is not None) for i in infos)
        out[name] = take(log)
    return out


# ------------------------------------------------------------------------------------------------ the kept K/V
def _kept_kv():
    out = {}
    vid = make_video(40)

    def one(eng, cache, prompt):
        info = {}
        encode.encode_video_with(eng, vid, vid, SIZE, 4, 4 + len(prompt), list(prompt), None, 10 ** 6, None, None, None, info,
                                 cache)
        return info["cache"]["kv"]
    eng, log = rec(KVEngine(K=3, H=8, N=5))
    cache = FrameCache(1 << 30, kv_bytes=1 << 20)
    assert one(eng, cache, (1, 2)) == dict(state="filled", frames=15, bytes=ENTRY40)
    out["kv_video_filled"] = take(log)
    assert one(eng, cache, (5, 6, 7)) == dict(state="hit", frames=15, bytes=ENTRY40)
    out["kv_video_hit"] = take(log)
    eng, log = rec(KVEngine(K=3, H=8, N=5))
    assert one(eng, FrameCache(1 << 30, kv_bytes=ENTRY40 - 1), (1, 2)) == dict(state="bypassed", frames=15, bytes=ENTRY40)
    assert all("kv" not in c[2] for c in log if c[0] == "compress_frames")
    out["kv_below_one_entry_bypassed"] = take(log)
    eng, log = rec(CFake(N=5))
    assert one(eng, FrameCache(1 << 30, kv_bytes=1 << 20), (1, 2)) == dict(state="unsupported", frames=15, bytes=0)
    out["kv_unsupported_engine"] = take(log)
    # two groups over the same distinct frames: the first fills the entry, the second hits it (test_kv_cache)
    eng, log = rec(KVEngine(K=3, H=8, N=5, max_len=400, max_num_segments=6))
    prompts = [dict(budget_text_len=4, n_text_tokens=6, prompt_ids=[1, 2 + i]) for i in range(4)]
    infos = [{} for _ in prompts]
    encode.encode_video_prompts_with(eng, vid, vid, SIZE, prompts, None, 224, None, infos,
                                     FrameCache(1 << 30, kv_bytes=1 << 20), 2, 1.0)
    assert [i["cache"]["kv"]["state"] for i in infos] == ["filled", "filled", "hit", "hit"]
    assert [i["prompts"]["group_size"] for i in infos] == [2, 2, 2, 2]
    out["kv_prompt_groups_filled_then_hit"] = take(log)
    return out


# ------------------------------------------------------------------------------------------------ the mixin
def _mixin_case(eng, images, n=1, prompts=None, **cfg):
    """prepare_inputs_labels_for_multimodal on the stub LM with the recorded engine -> (log, the 10-tuple, the engine)"""
    lm = feature_lm(**cfg)
    eng, log = rec(eng)
    lm.get_model()._tdc_encoder = eng
    images = images(eng, log) if callable(images) else images
    del log[:]
    return log, call(lm, images, n, prompts), eng


def _mixin():
    out = {}
    vid, im = make_video(40), make_video(1)
    log, got, _ = _mixin_case(FeatureMixinEngine(K=3, H=8), [[vid], [vid + 0.5]])
    assert len(got[8]) == 37 and names(log).count("tower") == 2 and "compress_frames" in names(log)      # config.tdc_frame_cap
    out["mixin_pixels_video_T40_cap37"] = log
    log, got, _ = _mixin_case(FeatureMixinEngine(K=3, H=8), [im, im + 0.5])
    assert len(got[8]) == 1 and names(log) == ["tower", "tower", "connector"]
    out["mixin_pixels_image"] = log
    log, got, _ = _mixin_case(CMixinEngine(K=3, H=8), [im, im + 0.5], tdc_video_cache_bytes=1 << 30)
    assert len(got[8]) == 1 and names(log)[:2] == ["fingerprint", "fingerprint"]
    out["mixin_pixels_image_cached"] = log

    def one_set(T0):
        return lambda eng, log: [[encode.export_features_with(eng, *pixels(T0), SIZE)], [None]]
    log, got, eng = _mixin_case(FeatureMixinEngine(K=3, H=8), one_set(40), tdc_feature_inputs=True)
    assert len(got[8]) == 37 and "tower" not in names(log) and "sims_tensor" in names(log)
    out["mixin_features_video_T40_cap37"] = log

    def image_set(eng, log):
        fs = encode.export_features_with(eng, *pixels(1), SIZE)
        return [fs.siglip, fs.dino]
    log, got, _ = _mixin_case(FeatureMixinEngine(K=3, H=8), image_set, tdc_feature_inputs=True)
    assert len(got[8]) == 1 and names(log) == ["connector"]
    out["mixin_features_image"] = log

    def one_video_thrice(eng, log):
        fs = encode.export_features_with(eng, *pixels(40), SIZE)
        clone = FeatureSet(fs.siglip.clone(), fs.dino.clone(), SIZE, fs.signature)
        return [[fs, clone, fs], [None] * 3]
    log, got, eng = _mixin_case(CompactMixinEngine(K=3, H=8), one_video_thrice, 3, [[1, 2], [3, 4, 5], [6]],
                                tdc_feature_inputs=True, tdc_batch_prompts=4)
    assert eng.prompt_calls == [3] and len(got[8]) == 3 * 37 and names(log).count("connector") == 1
    out["mixin_features_batch_prompts_3"] = log
    frames = torch.from_numpy(make_frames(40))
    log, got, eng = _mixin_case(CachedFrameMixinEngine(K=3, H=8), [[frames], None], tdc_frame_inputs=True,
                                tdc_video_cache_bytes=1 << 30)
    assert len(got[8]) == 37 and [len(a) for a in eng.asked] == [37] and "fingerprint" in names(log)
    out["mixin_frames_video_cached_T40_cap37"] = log
    log, got, eng = _mixin_case(FrameMixinEngine(K=3, H=8), [frames[:1], None], tdc_frame_inputs=True)
    assert len(got[8]) == 1 and eng.asked == [None] and names(log) == ["pixels_from_frames", "tower", "tower", "connector"]
    out["mixin_frames_image"] = log
    return out


def run_cases():
    """-> {case: call log}; T0 = 40 under a frame cap of 30 (the mixin's config: 37): a1 drops frames and a5 segments
    (max_num_segments is 24); T0 = 8 passes through; T0 = 1 is an image"""
    out = {}
    for part in (_exports, _features, _frames, _kept_kv, _mixin):
        got = part()
        assert not set(got) & set(out)
        out.update(got)
    return json.loads(json.dumps(out))          # tuples -> lists, as the fixture holds them


@pytest.fixture(scope="module")
def logs():
    return run_cases()


with open(GOLDEN) as _f:
    WANT = json.load(_f)


def test_the_fixture_holds_every_case(logs):
    assert sorted(logs) == sorted(WANT) and len(WANT) == 33


@pytest.mark.parametrize("case", sorted(WANT))
def test_call_order(logs, case):
    assert_same_log(case, logs[case], WANT[case])


def test_the_feature_front_reads_the_similarities_as_the_pixel_front_does(logs):
    """lossless rows: sims_tensor, mark, fetch - and no tower anywhere in a call from features"""
    n = names(logs["features_T40_cap30"])
    i = n.index("sims_tensor")
    assert n[i:i + 3] == ["sims_tensor", "mark", "fetch"] and "tower" not in n


def test_a_hit_hands_compress_frames_a_kept_buffer_and_allocates_none(logs):
    fill, hit = logs["kv_video_filled"], logs["kv_video_hit"]
    assert "kv_alloc" in names(fill) and "kv_alloc" not in names(hit)
    for log in (fill, hit):
        assert [c[2] for c in log if c[0] == "compress_frames"] == [{"kv": "KeptKV"}]
