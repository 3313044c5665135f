"""CPU: encode from stored tower features (features.FeatureSet, encode.*_features_*) on the engine
double of test_dist_gloo - the orchestration must give, from an exported set, exactly what the pixel path gives: tokens, info,
selected segments.  Plus the stored form itself (save / load, signature) and the mixin's `config.tdc_feature_inputs`."""
import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import encode, features, pipeline
from tdc_video_amd.cache import fingerprint_rows_host
from test_dist_gloo import FakeEngine, MixinEngine, NoisyEngine, make_video
from test_host_logic import build_stub_lm, tiny_config
from test_multi_prompt import MultiEngine

SIZE = (384, 384)
FeatureSet, tower_signature = features.FeatureSet, features.tower_signature


def tower_weights(H):
    return {"siglip": {"w": torch.arange(1, H + 1).float() * 0.5, "kind": "siglip"},
            "dino": {"w": torch.arange(1, H + 1).float(), "kind": "dino"}}


class FeatureEngine(MultiEngine):
    """the double with tower WEIGHTS (FakeEngine's constants as tensors the signature can fingerprint) and a connector weight;
    counts tower calls"""

    def __init__(self, *a, conn_w=1.0, **kw):
        super().__init__(*a, **kw)
        self.towers = tower_weights(self.H)
        self.conn_w = conn_w
        self.tower_calls = 0

    def tower(self, name, px):
        self.tower_calls += 1
        B = px.shape[0]
        base = px.reshape(B, -1)[:, : self.P].reshape(B * self.P, 1)
        return base * self.towers[name]["w"][None]

    def connector(self, sig, dino, T, sizes, keep=None):
        X, fs = super().connector(sig, dino, T, sizes, keep)
        return X * self.conn_w, fs


class NoisyFeatureEngine(NoisyEngine):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.towers = tower_weights(self.H)


def pixels(T0):
    vid = make_video(T0)
    return vid, vid + 0.5


def both(eng, T0, cap=224, audio=None, prompt=(1, 2, 3), btl=4, n_text=4, video_index=None):
    """(pixel result, its info), (feature result, its info) of one video"""
    ps, pd = pixels(T0)
    wi, gi = {}, {}
    want = pipeline.encode_video_with(eng, ps, pd, SIZE, btl, n_text, list(prompt), audio, cap, None, None, video_index, wi)
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    assert fs.frames == T0 and fs.image_size == SIZE
    n = eng.tower_calls if hasattr(eng, "tower_calls") else None
    got = encode.encode_features_with(eng, fs, btl, n_text, list(prompt), audio, cap, None, video_index, gi)
    if n is not None:
        assert eng.tower_calls == n, "the feature path ran a tower"
    return (want, wi), (got, gi), fs


# ------------------------------------------------------------------------------------------------ bitwise equality
@pytest.mark.parametrize("T0,cap,kept", [(40, 224, 40), (40, 30, 30), (20, 224, 20)])
def test_encode_features_equals_encode_video(T0, cap, kept):
    eng = FeatureEngine(N=5)
    (want, wi), (got, gi), fs = both(eng, T0, cap)
    assert torch.equal(got, want)
    assert gi == wi
    assert gi["final_size"] == wi["final_size"] and gi["seg_indices"] == wi["seg_indices"]
    assert len(gi["frame_indices"]) == kept
    if T0 == 20:                                                  # <= max_num_segments + 1: the unsegmented branch
        assert gi["seg_indices"] == list(range(20))
    else:
        assert len(gi["seg_indices"]) == 24
    assert tuple(fs.siglip.shape) == (T0, eng.P, eng.H) and tuple(fs.dino.shape) == (T0, eng.P, eng.H)
    assert torch.equal(fs.dino.reshape(-1, eng.H), FakeEngine.tower(eng, "dino", pixels(T0)[1]))


def test_encode_features_with_audio_and_video_index():
    eng = FeatureEngine(N=5, audio_input=True)
    g = torch.Generator().manual_seed(2)
    audio = {"per_second": torch.rand(62, 2, eng.H, generator=g)}
    for cap, vi in ((224, None), (17, None), (224, [1, 0] * 31), (17, [1, 0] * 31)):
        (want, wi), (got, gi), _ = both(eng, 31, cap, audio=audio if vi else {"per_second": audio["per_second"][:31]},
                                        video_index=vi)
        assert torch.equal(got, want) and gi == wi


def test_encode_features_prompts_equals_per_prompt_calls():
    eng = FeatureEngine(K=3, H=8, N=5, max_len=400, max_num_segments=6)
    ps, pd = pixels(40)
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    prompts = [dict(budget_text_len=4, n_text_tokens=4, prompt_ids=[5]),
               dict(budget_text_len=4, n_text_tokens=30, prompt_ids=[7, 8, 9, 10]),
               dict(budget_text_len=4, n_text_tokens=60, prompt_ids=list(range(20, 29)))]
    infos = [{} for _ in prompts]
    calls = eng.tower_calls
    got = encode.encode_features_prompts_with(eng, fs, prompts, infos=infos, pad_fraction=1.0)
    assert eng.tower_calls == calls and eng.multi_calls == 1
    for p, pr in enumerate(prompts):
        wi = {}
        want = encode.encode_features_with(eng, fs, pr["budget_text_len"], pr["n_text_tokens"], pr["prompt_ids"], info=wi)
        assert torch.equal(got[p], want), p
        assert {k: v for k, v in infos[p].items() if k != "prompts"} == wi
        # ... which is the pixel path's multi-prompt result too
    want_px = pipeline.encode_video_prompts_with(eng, ps, pd, SIZE, prompts, pad_fraction=1.0)
    assert all(torch.equal(a, b) for a, b in zip(got, want_px))


def test_image_set_runs_the_connector_only():
    eng = FeatureEngine(N=5)
    ps, pd = pixels(3)
    fs = encode.export_features_with(eng, ps[1:2], pd[1:2], SIZE)
    info = {}
    got = encode.encode_features_with(eng, fs, None, 4, None, info=info, image=True)
    X, sizes = eng.connector(eng.tower("siglip", ps[1:2]), eng.tower("dino", pd[1:2]), 1, [SIZE])
    assert torch.equal(got, X[:, :eng.H]) and info == {"final_size": sizes}
    with pytest.raises(ValueError, match="one-frame"):
        encode.encode_features_with(eng, encode.export_features_with(eng, ps, pd, SIZE), None, 4, None, image=True)


# ------------------------------------------------------------------------------------------------ the stored form
def test_save_load_round_trip(tmp_path):
    eng = FeatureEngine(N=5)
    ps, pd = pixels(12)
    fs = encode.export_features_with(eng, ps, pd, (360, 640))
    path = str(tmp_path / "video.tdcfeat")
    fs.save(path)
    d = torch.load(path, weights_only=True)                       # a plain dict: tensors, ints, strings
    assert sorted(d) == ["dino", "format", "image_size", "siglip", "signature"]
    assert isinstance(d["signature"], str) and d["image_size"] == [360, 640] and isinstance(d["format"], int)
    back = FeatureSet.load(path)
    assert torch.equal(back.siglip, fs.siglip) and torch.equal(back.dino, fs.dino)
    assert back.siglip.dtype == fs.siglip.dtype and back.image_size == (360, 640) and back.signature == fs.signature
    assert back.nbytes == fs.nbytes == 2 * 12 * eng.P * eng.H * 4
    a = encode.encode_features_with(eng, fs, 4, 4, [1, 2])
    assert torch.equal(encode.encode_features_with(eng, back, 4, 4, [1, 2]), a)
    host = fs.cpu()
    assert torch.equal(host.siglip, fs.siglip) and host.to("cpu") is host and host.signature == fs.signature
    # a view keeps only its own bytes in the file
    part = FeatureSet(fs.siglip[:2], fs.dino[:2], fs.image_size, fs.signature)
    part.save(path)
    assert FeatureSet.load(path).siglip.untyped_storage().nbytes() == 2 * eng.P * eng.H * 4
    torch.save({"format": 99}, path)
    with pytest.raises(ValueError, match="FeatureSet file"):
        FeatureSet.load(path)


def test_feature_set_refuses_mismatched_tensors():
    x = torch.zeros(3, 4, 8)
    for s, d in ((x, torch.zeros(2, 4, 8)), (x, torch.zeros(3, 5, 8)), (x[0], x[0]), (x, x.half())):
        with pytest.raises(ValueError):
            FeatureSet(s, d, SIZE)
    assert FeatureSet(x, torch.zeros(3, 4, 6), SIZE).frames == 3  # the towers' widths differ


def test_signature_follows_the_towers_and_nothing_behind_them():
    a, b, c = FeatureEngine(N=5), FeatureEngine(N=5), FeatureEngine(N=5, conn_w=1.5, K=4)
    b.towers["dino"]["w"][3] += 1.0                               # one element of one tower weight
    ps, pd = pixels(30)
    fs = encode.export_features_with(a, ps, pd, SIZE)
    assert fs.signature == tower_signature(a) == tower_signature(c) != tower_signature(b)
    with pytest.raises(ValueError) as ei:
        encode.encode_features_with(b, fs, 4, 4, [1])
    assert tower_signature(a) in str(ei.value) and tower_signature(b) in str(ei.value)
    with pytest.raises(ValueError):
        encode.encode_features_prompts_with(b, fs, [dict(budget_text_len=4, n_text_tokens=4, prompt_ids=[1])])
    # a different connector and context_token_num: the set passes, and the result is that engine's own
    got = encode.encode_features_with(c, fs, 4, 4, [1])
    assert torch.equal(got, pipeline.encode_video_with(c, ps, pd, SIZE, 4, 4, [1]))
    assert not torch.equal(got, encode.encode_features_with(a, fs, 4, 4, [1]))
    # check_signature=False: an engine without tower weights encodes the set; asked to check, it says why it cannot
    d = FeatureEngine(N=5)
    d.towers = {}
    assert torch.equal(encode.encode_features_with(d, fs, 4, 4, [1], check_signature=False),
                       encode.encode_features_with(a, fs, 4, 4, [1]))
    with pytest.raises(ValueError, match="no tower weights"):
        encode.encode_features_with(d, fs, 4, 4, [1])
    # every other field of the signature
    for attr, v in (("dtype", torch.float16), ("tower_res_dtype", torch.float16), ("out_grid", [24, 24])):
        e2 = FeatureEngine(N=5)
        setattr(e2, attr, v)
        assert tower_signature(e2) != tower_signature(a), attr
    for k, v in (("dtype", torch.bfloat16), ("fp8", 2), ("fused", True)):
        e2 = FeatureEngine(N=5)
        e2.towers["siglip"][k] = v
        assert tower_signature(e2) != tower_signature(a), k


def test_weight_fingerprint_is_the_cache_fingerprint():
    """the signature's tensor fingerprints are fingerprint_rows_host's (the device kernel's bits)"""
    _tensor_fp = features._tensor_fp
    w = torch.arange(1, 9).float()
    a, b = fingerprint_rows_host(w.numpy().view("uint8"))[0]
    assert _tensor_fp(None, w) == (int(a), int(b))


# ------------------------------------------------------------------------------------------------ selection refinement
def test_refinement_is_reported_unavailable():
    eng = NoisyFeatureEngine(N=5)
    (want, wi), (got, gi), _ = both(eng, 61)
    assert wi["refined_pairs"], "the case must have a band to refine"
    assert gi["refined_pairs"] == [] and gi["refine_unavailable_pairs"] == len(wi["refined_pairs"])
    # the stored similarities ranked as they are: what the engine selects with the refinement off
    off = NoisyFeatureEngine(N=5)
    off.selection_eps = None
    oi = {}
    ps, pd = pixels(61)
    plain = pipeline.encode_video_with(off, ps, pd, SIZE, 4, 4, [1, 2, 3], info=oi)
    assert gi["seg_indices"] == oi["seg_indices"] and torch.equal(got, plain)


def test_empty_band_gives_the_pixel_paths_info():
    eng = NoisyFeatureEngine(N=5)
    ps = torch.rand(40, 3, 2, 2, generator=torch.Generator().manual_seed(4))    # unrelated frames: the decisive ranks lie apart
    wi, gi = {}, {}
    want = pipeline.encode_video_with(eng, ps, ps + 0.5, SIZE, 4, 4, [1, 2], info=wi)
    assert wi["refined_pairs"] == [] and "refine_skipped_pairs" not in wi
    fs = encode.export_features_with(eng, ps, ps + 0.5, SIZE)
    got = encode.encode_features_with(eng, fs, 4, 4, [1, 2], info=gi)
    assert torch.equal(got, want) and gi == wi and "refine_unavailable_pairs" not in gi


# ------------------------------------------------------------------------------------------------ the mixin
class Untouchable:
    """an engine no call may reach"""

    def __getattr__(self, name):
        raise AssertionError("the engine was touched: %s" % name)


ARCH8 = dict(siglip=dict(D=8, layers=1, mlp=16, n_pos=81, heads=2), dino=dict(D=8, layers=1, mlp=16, n_pos=25, heads=2))


def feature_lm(**over):
    torch.manual_seed(3)
    return build_stub_lm(tiny_config(hidden_size=8, context_token_num=3, tdc_frame_cap=37, tokenizer_model_max_length=10 ** 9,
                                     tdc_tower_archs=ARCH8, **over))


def call(lm, images, n=1, prompts=None):
    ids = torch.tensor([[11, 12, -200, 13, 14, 15]] * n)
    with torch.inference_mode():
        return lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, images, image_sizes=[SIZE] * n,
                                                       video_indices=[None] * n, prompts=prompts or [[1, 2]] * n,
                                                       audios=[None] * n)


def test_config_key_validates_and_names_itself():
    m = lambda **kw: build_stub_lm(tiny_config(**kw)).get_model()
    assert m().tdc_feature_inputs() is False and m(tdc_feature_inputs=None).tdc_feature_inputs() is False
    assert m(tdc_feature_inputs=False).tdc_feature_inputs() is False and m(tdc_feature_inputs=True).tdc_feature_inputs() is True
    for bad in (1, 0, "yes", 2.5):
        with pytest.raises(ValueError, match="tdc_feature_inputs"):
            m(tdc_feature_inputs=bad).tdc_feature_inputs()
    assert m(tdc_feature_inputs=True, tdc_batch_prompts=4).tdc_feature_inputs() is True
    assert m(tdc_feature_inputs=False, tdc_batch_frames=512).tdc_feature_inputs() is False


@pytest.mark.parametrize("other,v", [("tdc_shard_frames", True), ("tdc_batch_frames", 512), ("tdc_video_cache_bytes", 1 << 30),
                                     ("tdc_shard_cache_bytes", 1 << 30)])
def test_forbidden_combinations_raise_before_any_engine_call(other, v):
    lm = feature_lm(tdc_feature_inputs=True, **{other: v})
    lm.get_model()._tdc_encoder = Untouchable()
    x = torch.zeros(30, 4, 8)
    with pytest.raises(ValueError) as ei:
        call(lm, [[x], [x]])
    assert "tdc_feature_inputs" in str(ei.value) and other in str(ei.value)


def test_wrong_feature_width_raises_before_any_engine_call():
    lm = feature_lm(tdc_feature_inputs=True)
    lm.get_model()._tdc_encoder = Untouchable()
    good, bad = torch.zeros(30, 4, 8), torch.zeros(30, 4, 16)
    for images, name in (([[bad], [good]], "SigLIP"), ([[good], [bad]], "DINOv2"),
                         ([[FeatureSet(good, bad, SIZE)], [None]], "DINOv2")):
        with pytest.raises(ValueError) as ei:
            call(lm, images)
        assert "tdc_feature_inputs" in str(ei.value) and name in str(ei.value) and "16" in str(ei.value)
    with pytest.raises(ValueError, match="must be None"):
        call(lm, [[FeatureSet(good, good, SIZE)], [good]])
    with pytest.raises(ValueError, match="FeatureSet or"):
        call(lm, [[good], [None]])


class FeatureMixinEngine(MixinEngine):
    """MixinEngine with tower weights and the feature entries (as VideoEncoder forwards them)"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.towers = tower_weights(self.H)
        self.tower_calls = 0

    def tower(self, name, px):
        self.tower_calls += 1
        return super().tower(name, px)

    def encode_features(self, fs, *a, **kw):
        return encode.encode_features_with(self, fs, *a, **kw)


def same_tuple(a, b):
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y)
        else:
            assert x == y


def test_mixin_feature_inputs_give_the_pixel_calls_tuple():
    vids = [make_video(90), make_video(30) + 1.0]
    lm = feature_lm()
    eng = lm.get_model()._tdc_encoder = FeatureMixinEngine(K=3, H=8)
    want = call(lm, [vids, vids], 2, [[1, 2], [3, 4, 5]])
    sets = [encode.export_features_with(eng, v, v, SIZE) for v in vids]
    lm.get_model().config.tdc_feature_inputs = True
    n = eng.tower_calls
    same_tuple(call(lm, [[s.siglip for s in sets], [s.dino for s in sets]], 2, [[1, 2], [3, 4, 5]]), want)   # tensor pairs
    same_tuple(call(lm, [sets, [None, None]], 2, [[1, 2], [3, 4, 5]]), want)                                  # FeatureSets
    assert eng.tower_calls == n and len(want[8]) == 37 + 30
    # a FeatureSet of other towers is refused; the same rows as bare tensors carry no signature to compare
    other = FeatureSet(sets[0].siglip, sets[0].dino, SIZE, "towers of another day")
    with pytest.raises(ValueError, match="another day"):
        call(lm, [[other, sets[1]], [None, None]], 2, [[1, 2], [3, 4, 5]])
    # single images: two [bsz, tokens, width] tensors
    ims = make_video(3)
    lm.get_model().config.tdc_feature_inputs = False
    want_im = call(lm, [ims, ims], 3)
    im_sets = encode.export_features_with(eng, ims, ims, SIZE)
    lm.get_model().config.tdc_feature_inputs = True
    same_tuple(call(lm, [im_sets.siglip, im_sets.dino], 3), want_im)
