"""CPU: the batched encode (`config.tdc_batch_frames`, pipeline.encode_batch_with) on the engine test double of
test_dist_gloo: every sample of a batch must come out exactly as its own encode_video_with call (tokens and info), with one
tower call per tower for the whole group; the mixin's key on / off must give the same 10-tuple."""
import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import pipeline, segment as seg
from test_dist_gloo import FakeEngine, MixinEngine, NoisyEngine, make_video
from test_host_logic import build_stub_lm, tiny_config


def count_towers(eng):
    """spy: eng.tower counts its calls per tower name"""
    calls = {}
    tower = eng.tower

    def spy(name, px):
        calls[name] = calls.get(name, 0) + 1
        return tower(name, px)
    eng.tower = spy
    return calls


def sample(vid, audio=None, video_index=None, prompt=(1, 2), btl=4, n_text=4):
    return dict(px_siglip=vid, px_dino=vid + 0.5, image_size=(384, 384), budget_text_len=btl, n_text_tokens=n_text,
                prompt_ids=list(prompt), audio=audio, video_index=video_index, splice=None)


def single(eng, s, cap, info=None):
    return pipeline.encode_video_with(eng, s["px_siglip"], s["px_dino"], s["image_size"], s["budget_text_len"],
                                      s["n_text_tokens"], s["prompt_ids"], s["audio"], cap, None, s["splice"],
                                      s["video_index"], info)


def check_batch(eng, samples, cap):
    """encode_batch_with == encode_video_with per sample, tokens and info; -> the infos"""
    want, want_info = [], []
    for s in samples:
        want_info.append({})
        want.append(single(eng, s, cap, want_info[-1]))
    calls = count_towers(eng)
    infos = [{} for _ in samples]
    got = pipeline.encode_batch_with(eng, samples, cap, infos)
    assert calls == {"dino": 1, "siglip": 1}
    assert len(got) == len(samples)
    for g, w, i, wi in zip(got, want, infos, want_info):
        assert torch.equal(g, w)
        assert i == wi
    return infos


# ------------------------------------------------------------------------------------------------ config key
def test_config_key_validation():
    assert build_stub_lm(tiny_config()).get_model().tdc_batch_frames() == 0                       # absent: off
    assert build_stub_lm(tiny_config(tdc_batch_frames=None)).get_model().tdc_batch_frames() == 0
    assert build_stub_lm(tiny_config(tdc_batch_frames=0)).get_model().tdc_batch_frames() == 0
    assert build_stub_lm(tiny_config(tdc_batch_frames=512)).get_model().tdc_batch_frames() == 512
    for bad in (-1, "512", 3.5, True):
        with pytest.raises(ValueError, match="tdc_batch_frames"):
            build_stub_lm(tiny_config(tdc_batch_frames=bad)).get_model().tdc_batch_frames()


def test_config_key_ignored_under_sharding_and_the_frame_cache():
    assert build_stub_lm(tiny_config(tdc_batch_frames=512, tdc_shard_frames=True)).get_model().tdc_batch_frames() == 0
    assert build_stub_lm(tiny_config(tdc_batch_frames=512, tdc_video_cache_bytes=1 << 30)).get_model() \
        .tdc_batch_frames() == 0
    assert build_stub_lm(tiny_config(tdc_batch_frames=512, tdc_video_cache_bytes=0)).get_model().tdc_batch_frames() == 512


# ------------------------------------------------------------------------------------------------ grouping plan
def test_batch_groups_greedy_in_order():
    assert pipeline.batch_groups([10, 20, 30, 5, 5], 35) == [[0, 1], [2, 3], [4]]
    assert pipeline.batch_groups([10, 100, 10, 10], 64) == [[0], [1], [2, 3]]            # oversize sample alone
    assert pipeline.batch_groups([1] * 16, 16) == [list(range(16))]                        # images count 1
    assert pipeline.batch_groups([1] * 5, 2) == [[0, 1], [2, 3], [4]]
    assert pipeline.batch_groups([8, 8], 16) == [[0, 1]]                                   # the ceiling itself fits
    assert pipeline.batch_groups([], 16) == []
    # a change of pixel geometry starts a new group
    assert pipeline.batch_groups([1, 1, 1, 1], 16, ["a", "a", "b", "a"]) == [[0, 1], [2], [3]]


# ------------------------------------------------------------------------------------------------ engine level
def test_encode_batch_equals_per_sample_calls():
    """T = 20 (no Q-Former), 40 with per-second audio, 90 sub-sampled by a1 to the cap, 31 with a video_index"""
    eng = FakeEngine(N=5)
    cap = 50
    g = torch.Generator().manual_seed(11)
    audio = {"per_second": torch.rand(40, 2, eng.H, generator=g)}
    vi = [1, 0] * 31
    samples = [sample(make_video(20) * 0.5), sample(make_video(40) + 1.0, audio=audio, prompt=(3, 4, 5)),
               sample(make_video(90) - 0.25, n_text=9), sample(make_video(31) + 2.0, video_index=vi)]
    infos = check_batch(eng, samples, cap)
    assert [len(i["frame_indices"]) for i in infos] == [20, 40, 50, 31]
    assert infos[0]["seg_indices"] == list(range(20)) and len(infos[1]["seg_indices"]) == 24


def test_encode_batch_images_and_one_frame_videos():
    eng = MixinEngine(K=3, H=8)
    ims = make_video(3)
    samples = [dict(sample(ims[j:j + 1]), image=True) for j in range(3)] + [sample(ims[1:2])]
    infos = [{} for _ in samples]
    calls = count_towers(eng)
    got = pipeline.encode_batch_with(eng, samples, 224, infos)
    assert calls == {"dino": 1, "siglip": 1}
    for j in range(3):
        X, sizes = eng.connector(eng.tower("siglip", ims[j:j + 1]), eng.tower("dino", ims[j:j + 1] + 0.5), 1, [(384, 384)])
        assert torch.equal(got[j], X[:, :eng.H]) and infos[j] == {"final_size": sizes}
    want_info = {}
    assert torch.equal(got[3], single(eng, samples[3], 224, want_info)) and infos[3] == want_info


def test_cross_sample_pair_does_not_reach_a5():
    """the pair across the boundary of two samples has the lowest similarity of the group: it would be a segment boundary
    if it leaked into either sample's a5"""
    eng = FakeEngine(N=5)
    a = make_video(30) + 1.0                       # positive pixels
    b = -(make_video(30) + 1.0).flip(0)            # negative: cos-sim ~ -1 against a's last frame
    samples = [sample(a), dict(sample(b), px_dino=b - 0.5)]
    feats = eng.tower("dino", torch.cat([a + 0.5, b - 0.5]))
    sims = eng.sims_tensor(feats, 60).tolist()
    assert min(range(59), key=lambda k: sims[k]) == 29 and sims[29] < -0.9
    assert 29 in seg.select_segments(sims, 24)     # the hazard: over the concatenation the cross pair is picked
    infos = check_batch(eng, samples, 224)
    assert all(max(i["seg_indices"]) < 29 for i in infos)


def test_refinement_inside_a_batch():
    """a near-tied sample under the perturbed tower: its band is refined on its own pixels, batched as alone"""
    eng = NoisyEngine(N=5)
    samples = [sample(make_video(40) + 3.0), sample(make_video(61)), sample(make_video(12))]
    infos = check_batch(eng, samples, 224)
    assert infos[1]["refined_pairs"], "the case must refine a band"


# ------------------------------------------------------------------------------------------------ the mixin
class BatchMixinEngine(MixinEngine):
    """MixinEngine with encode_batch (pipeline.encode_batch_with) and per-name tower counts"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.calls = {}
        self.batches = []

    def tower(self, name, px):
        self.calls[name] = self.calls.get(name, 0) + 1
        return super().tower(name, px)

    def encode_batch(self, samples, frame_cap=224, infos=None):
        self.batches.append(len(samples))
        return pipeline.encode_batch_with(self, samples, frame_cap, infos)


def mixin_call(batch_frames, videos, ids, prompts, images=False):
    torch.manual_seed(3)
    lm = build_stub_lm(tiny_config(hidden_size=8, context_token_num=3, tdc_frame_cap=37, tokenizer_model_max_length=10 ** 9,
                                   tdc_batch_frames=batch_frames))
    eng = lm.get_model()._tdc_encoder = BatchMixinEngine(K=3, H=8)
    n = len(videos)
    px = torch.cat(videos) if images else videos
    with torch.inference_mode():
        out = lm.prepare_inputs_labels_for_multimodal(ids, None, (ids != 0).long(), None, ids.clone(), [px, px],
                                                      image_sizes=[(384, 384)] * n, video_indices=[None] * n,
                                                      prompts=prompts, audios=[None] * n)
    return out, eng


def assert_same_tuple(a, b):
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert isinstance(y, torch.Tensor) and torch.equal(x, y)
        else:
            assert x == y or (x is None and y is None)


def test_mixin_key_on_equals_key_off_videos():
    videos = [make_video(90), make_video(30) + 1.0]
    ids = torch.tensor([[11, 12, -200, 13, 14, 15], [11, -200, 13, 14, 0, 0]])
    prompts = [[1, 2], [3, 4, 5]]
    off, e_off = mixin_call(0, videos, ids, prompts)
    on, e_on = mixin_call(512, videos, ids, prompts)
    assert_same_tuple(on, off)
    assert len(on[8]) == 37 + 30
    assert e_off.calls == {"dino": 2, "siglip": 2} and e_off.batches == []
    assert e_on.calls == {"dino": 1, "siglip": 1} and e_on.batches == [2]


def test_mixin_key_on_equals_key_off_images():
    ims = [make_video(4)[j:j + 1] + j for j in range(4)]
    ids = torch.tensor([[11, -200, 13]] * 4)
    off, e_off = mixin_call(0, ims, ids, None, images=True)
    on, e_on = mixin_call(16, ims, ids, None, images=True)
    assert_same_tuple(on, off)
    assert e_off.calls == {"dino": 4, "siglip": 4}
    assert e_on.calls == {"dino": 1, "siglip": 1} and e_on.batches == [4]


def test_mixin_ceiling_below_a_sample_and_bsz_one_stay_per_sample():
    videos = [make_video(90), make_video(30) + 1.0, make_video(20) - 1.0]
    ids = torch.tensor([[11, -200, 13]] * 3)
    prompts = [[1, 2]] * 3
    off, _ = mixin_call(0, videos, ids, prompts)
    on, eng = mixin_call(50, videos, ids, prompts)            # 37 frames alone; 30 + 20 together
    assert_same_tuple(on, off)
    assert eng.batches == [2] and eng.calls == {"dino": 2, "siglip": 2}
    one, eng1 = mixin_call(512, videos[:1], ids[:1], prompts[:1])
    assert eng1.batches == [] and torch.equal(one[4][0], off[4][0][:one[4].shape[1]])


def test_mixin_key_on_raises_like_key_off():
    videos = [make_video(30), make_video(30)]
    ids = torch.tensor([[11, -200, 13], [11, -200, 13]])
    for bf in (0, 512):
        with pytest.raises(RuntimeError, match="bert_tokenizer"):
            mixin_call(bf, videos, ids, [[1, 2], "a string prompt"])
    ids2 = torch.tensor([[11, -200, 13], [-200, 12, -200]])
    for bf in (0, 512):
        with pytest.raises(IndexError):
            mixin_call(bf, videos, ids2, [[1, 2], [1, 2]])
