"""CPU: the compact feature store (features.FeatureSet with store = "e4m3") on the engine double of
test_features, its quantiser and decoder written with torch.float8_e4m3fn: the stored form (format 2, nbytes, validation), the
selection from the stored similarities when a1 keeps every frame and from the decoded rows when it does not, and compact sets
through the mixin's `config.tdc_feature_inputs` and its `tdc_batch_prompts` grouping."""
import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import encode, features
from tdc_video_amd.cache import fingerprint_rows_host
from test_features import SIZE, FeatureEngine, FeatureMixinEngine, call, feature_lm, pixels
from test_dist_gloo import make_video

FeatureSet = features.FeatureSet


class _Compact:
    """what an engine adds for compact sets (VideoEncoder: tdc_quantize_rows_fp8 / tdc_gather_rows with scales), on the host"""
    sims_calls = 0

    def sims_tensor(self, dino, T):
        self.sims_calls += 1
        return super().sims_tensor(dino, T)

    def quantize_feature_rows(self, rows, D):
        x = rows[:, :D].float()
        amax = x.abs().amax(1)
        scale = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
        return (x * (1.0 / scale)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), scale

    def decode_feature_rows(self, x8, scale, idx, dtype):
        if idx is not None:
            sel = torch.tensor(idx)
            x8, scale = x8[sel], scale[sel]
        T, P, D = x8.shape
        return (x8.reshape(T * P, D).view(torch.float8_e4m3fn).float() * scale.reshape(T * P, 1)).to(dtype)


class CompactEngine(_Compact, FeatureEngine):
    pass


def sets(eng, T0, size=SIZE):
    ps, pd = pixels(T0)
    fs = encode.export_features_with(eng, ps, pd, size)
    return fs, encode.compact_features_with(eng, fs), (ps, pd)


# ------------------------------------------------------------------------------------------------ the stored form
def test_compact_set_holds_bytes_scales_and_the_exact_similarities():
    eng = CompactEngine(N=5)
    fs, cs, (ps, pd) = sets(eng, 12)
    assert fs.store == "f16" and cs.store == "e4m3" and cs.rows_dtype == torch.float32 and cs.signature == fs.signature
    assert cs.siglip.dtype == cs.dino.dtype == torch.uint8 and cs.siglip.shape == fs.siglip.shape
    assert cs.siglip_scale.dtype == torch.float32 and tuple(cs.siglip_scale.shape) == tuple(cs.dino_scale.shape) == (12, eng.P)
    assert torch.equal(cs.sims, eng.sims_tensor(fs.dino.reshape(-1, eng.H), 12)) and cs.sims.dtype == torch.float32
    # the two routes give the same bytes
    ex = encode.export_features_with(eng, ps, pd, SIZE, store="e4m3")
    for k, t in cs.tensors().items():
        assert torch.equal(getattr(ex, k), t), k
    assert features.is_feature_set(cs) and features.is_feature_set(fs) and encode.compact_features_with(eng, cs) is cs
    with pytest.raises(ValueError, match="store"):
        encode.export_features_with(eng, ps, pd, SIZE, store="fp4")
    # one frame: no similarities
    one = encode.export_features_with(eng, ps[:1], pd[:1], SIZE, store="e4m3")
    assert one.sims is None and one.frames == 1


def test_nbytes_is_everything_the_set_holds():
    T0, P, Ds, Dd = 3, 5, 1152, 1536
    lossless = FeatureSet(torch.zeros(T0, P, Ds, dtype=torch.float16), torch.zeros(T0, P, Dd, dtype=torch.float16), SIZE)
    cs = FeatureSet(torch.zeros(T0, P, Ds, dtype=torch.uint8), torch.zeros(T0, P, Dd, dtype=torch.uint8), SIZE, None,
                    torch.ones(T0, P), torch.ones(T0, P), torch.zeros(T0 - 1), torch.float16)
    assert cs.nbytes == T0 * P * (Ds + Dd) + 8 * T0 * P + 4 * (T0 - 1)
    assert cs.nbytes <= 0.51 * lossless.nbytes
    assert lossless.nbytes == 2 * T0 * P * (Ds + Dd)


def test_format_2_round_trip_and_format_1_still_loads(tmp_path):
    eng = CompactEngine(N=5)
    fs, cs, _ = sets(eng, 12, (360, 640))
    path = str(tmp_path / "video.tdcfeat")
    cs.save(path)
    d = torch.load(path, weights_only=True)                       # a plain dict: tensors, ints, strings
    assert d["format"] == 2 and d["store"] == "e4m3" and d["rows_dtype"] == "float32" and d["siglip"].dtype == torch.uint8
    assert sorted(d) == ["dino", "dino_scale", "format", "image_size", "rows_dtype", "siglip", "siglip_scale", "signature",
                         "sims", "store"]
    back = FeatureSet.load(path)
    assert back.store == "e4m3" and back.rows_dtype == cs.rows_dtype and back.image_size == (360, 640)
    assert back.signature == cs.signature and back.nbytes == cs.nbytes
    for k, t in cs.tensors().items():
        assert torch.equal(getattr(back, k), t) and getattr(back, k).dtype == t.dtype, k
    assert torch.equal(encode.encode_features_with(eng, back, 4, 4, [1, 2]), encode.encode_features_with(eng, cs, 4, 4, [1, 2]))
    host = cs.cpu()
    assert host.store == "e4m3" and torch.equal(host.dino_scale, cs.dino_scale) and host.to("cpu") is host
    # a one-frame compact set (no similarities) round-trips too
    one = encode.compact_features_with(eng, FeatureSet(fs.siglip[:1], fs.dino[:1], SIZE, fs.signature))
    one.save(path)
    assert FeatureSet.load(path).sims is None
    # lossless sets are still format 1, and a format-1 file written by the parent's save() still loads
    fs.save(path)
    assert torch.load(path, weights_only=True)["format"] == 1
    torch.save(dict(format=1, siglip=fs.siglip.clone(), dino=fs.dino.clone(), image_size=[360, 640], signature=fs.signature), path)
    old = FeatureSet.load(path)
    assert old.store == "f16" and torch.equal(old.siglip, fs.siglip) and old.sims is None and old.nbytes == fs.nbytes


def test_compact_set_refuses_wrong_scales_and_byte_types():
    b, sc = torch.zeros(3, 4, 8, dtype=torch.uint8), torch.ones(3, 4)
    assert FeatureSet(b, b, SIZE, None, sc, sc, torch.zeros(2), torch.float16).store == "e4m3"
    bad = [dict(siglip_scale=torch.ones(3, 5)), dict(dino_scale=torch.ones(4, 3)), dict(siglip_scale=None),
           dict(dino_scale=sc.double()), dict(sims=torch.zeros(3)), dict(rows_dtype=torch.int8), dict(rows_dtype=None)]
    for over in bad:
        kw = dict(siglip_scale=sc, dino_scale=sc, sims=torch.zeros(2), rows_dtype=torch.float16)
        kw.update(over)
        with pytest.raises(ValueError):
            FeatureSet(b, b, SIZE, None, **kw)
    for s, d in ((b.to(torch.int8), b), (b, b.half()), (b.half(), b.half())):           # scales with anything but uint8 bytes
        with pytest.raises(ValueError):
            FeatureSet(s, d, SIZE, None, sc, sc, None, torch.float16)
    with pytest.raises(ValueError):                                                     # bytes without scales
        FeatureSet(b, b, SIZE)


# ------------------------------------------------------------------------------------------------ the selection
def test_all_frames_kept_selects_from_the_stored_similarities():
    eng = CompactEngine(N=5)
    fs, cs, _ = sets(eng, 40)
    wi, gi = {}, {}
    want = encode.encode_features_with(eng, fs, 4, 4, [1, 2, 3], info=wi)
    calls, towers = eng.sims_calls, eng.tower_calls
    got = encode.encode_features_with(eng, cs, 4, 4, [1, 2, 3], info=gi)
    assert eng.sims_calls == calls and eng.tower_calls == towers, "a5 or a tower ran on a compact set with every frame kept"
    assert gi["selection_sims"] == "stored" and "selection_sims" not in wi
    assert gi["seg_indices"] == wi["seg_indices"] and len(gi["seg_indices"]) == 24
    assert gi["frame_indices"] == wi["frame_indices"] and gi["final_size"] == wi["final_size"] and got.shape == want.shape
    assert torch.allclose(got, want, rtol=0.07, atol=0.0)          # e4m3: 2^-4 relative per element, all of one sign here


def test_subsampled_frames_select_from_the_decoded_rows():
    eng = CompactEngine(N=5)
    fs, cs, _ = sets(eng, 40)
    gi = {}
    calls = eng.sims_calls
    got = encode.encode_features_with(eng, cs, 4, 4, [1, 2, 3], frame_cap=30, info=gi)
    assert eng.sims_calls == calls + 1 and gi["selection_sims"] == "decoded" and len(gi["frame_indices"]) == 30
    assert got.shape == encode.encode_features_with(eng, fs, 4, 4, [1, 2, 3], frame_cap=30).shape
    # a short video is not segmented at all: no similarities are read, no key is reported
    si = {}
    short = encode.compact_features_with(eng, FeatureSet(fs.siglip[:20], fs.dino[:20], SIZE, fs.signature))
    encode.encode_features_with(eng, short, 4, 4, [1], info=si)
    assert "selection_sims" not in si and si["seg_indices"] == list(range(20))


def test_image_and_prompts_forms_take_compact_sets():
    eng = CompactEngine(K=3, H=8, N=5, max_len=400, max_num_segments=6)
    fs, cs, (ps, pd) = sets(eng, 40)
    prompts = [dict(budget_text_len=4, n_text_tokens=4, prompt_ids=[5]),
               dict(budget_text_len=4, n_text_tokens=30, prompt_ids=[7, 8, 9, 10]),
               dict(budget_text_len=4, n_text_tokens=60, prompt_ids=list(range(20, 29)))]
    infos = [{} for _ in prompts]
    got = encode.encode_features_prompts_with(eng, cs, prompts, infos=infos, pad_fraction=1.0)
    assert eng.multi_calls == 1
    for p, pr in enumerate(prompts):
        wi = {}
        want = encode.encode_features_with(eng, cs, pr["budget_text_len"], pr["n_text_tokens"], pr["prompt_ids"], info=wi)
        assert torch.equal(got[p], want), p
        assert {k: v for k, v in infos[p].items() if k != "prompts"} == wi and wi["selection_sims"] == "decoded"    # a1 drops frames
    one = encode.export_features_with(eng, ps[1:2], pd[1:2], SIZE, store="e4m3")
    info = {}
    im = encode.encode_features_with(eng, one, None, 4, None, info=info, image=True)
    sig, dino = encode.feature_rows(eng, one)
    X, sizes = eng.connector(sig, dino, 1, [SIZE])
    assert torch.equal(im, X[:, :eng.H]) and info == {"final_size": sizes}


# ------------------------------------------------------------------------------------------------ the mixin
class CompactMixinEngine(_Compact, FeatureMixinEngine):
    """FeatureMixinEngine with the compact entries, the multi-prompt entry and a host fingerprint (same_features_key)"""
    prompt_calls = None

    def fingerprint(self, px, rows, row_bytes=None, row_stride=None):
        b = px.contiguous().view(-1).view(torch.uint8).numpy()
        return [tuple(int(v) for v in fingerprint_rows_host(b[r * row_stride:r * row_stride + row_bytes])[0]) for r in rows]

    def multi_prompt_ok(self, Nf):
        return False                            # FakeEngine.compress_frames has no multi form: every group runs compress_with

    def encode_features_prompts(self, fs, prompts, **kw):
        self.prompt_calls = (self.prompt_calls or []) + [len(prompts)]
        return encode.encode_features_prompts_with(self, fs, prompts, **kw)


def same_tuple(a, b):
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y)
        else:
            assert x == y


def test_mixin_takes_compact_sets_and_groups_their_prompts():
    vids = [make_video(90), make_video(30) + 1.0]
    lm = feature_lm(tdc_feature_inputs=True)
    eng = lm.get_model()._tdc_encoder = CompactMixinEngine(K=3, H=8)
    csets = [encode.export_features_with(eng, v, v, SIZE, store="e4m3") for v in vids]
    n = eng.tower_calls
    got = call(lm, [csets, [None, None]], 2, [[1, 2], [3, 4, 5]])
    assert eng.tower_calls == n and len(got[8]) == 37 + 30
    # what the engine gives for each set on its own (frame cap 37: the 90-frame set decodes, the 30-frame one reads its sims)
    for i, (cs, pid) in enumerate(zip(csets, ([1, 2], [3, 4, 5]))):
        one = call(lm, [[cs], [None]], 1, [pid])
        assert torch.equal(got[4][i, :one[4].shape[1]], one[4][0])
    # a compact set of other towers is refused
    other = FeatureSet(csets[0].siglip, csets[0].dino, SIZE, "towers of another day", csets[0].siglip_scale,
                       csets[0].dino_scale, csets[0].sims, csets[0].rows_dtype)
    with pytest.raises(ValueError, match="another day"):
        call(lm, [[other, csets[1]], [None, None]], 2, [[1, 2], [3, 4, 5]])
    # config.tdc_batch_prompts: the same compact video twice (once as equal tensors in another allocation) is ONE group; the
    # same bytes under other scales are another video
    cs = csets[1]
    clone = FeatureSet(cs.siglip.clone(), cs.dino.clone(), SIZE, cs.signature, cs.siglip_scale.clone(), cs.dino_scale.clone(),
                       cs.sims.clone(), cs.rows_dtype)
    scaled = FeatureSet(cs.siglip, cs.dino, SIZE, cs.signature, cs.siglip_scale * 2.0, cs.dino_scale, cs.sims, cs.rows_dtype)
    prompts = [[1, 2], [3, 4, 5], [6]]
    off = call(lm, [[cs, clone, scaled], [None] * 3], 3, prompts)
    lm.get_model().config.tdc_batch_prompts = 4
    same_tuple(call(lm, [[cs, clone, scaled], [None] * 3], 3, prompts), off)
    assert eng.prompt_calls == [2]
    assert encode.same_features_key(eng, cs, 4, 37) == encode.same_features_key(eng, clone, 4, 37) \
        != encode.same_features_key(eng, scaled, 4, 37)
