"""CPU: the gap table of a compact feature set (features.FeatureSet.gap_sims, `gaps=` of the exports) on
the engine doubles of test_features / test_feature_store: what the table holds, how `gaps` is read, the bound on a1's gaps that
makes "auto" enough, the stored form (format 3), the selection it protects under frame sub-sampling - on a double whose tower is
not rank one, so that the e4m3 rounding really moves the similarities -, FeatureSet.clip and the mixin."""
import math

import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import encode, features, segment as seg
from test_feature_store import CompactEngine, CompactMixinEngine, same_tuple
from test_features import SIZE, call, feature_lm, pixels
from test_frame_inputs import _Frames, make_frames

FeatureSet = features.FeatureSet


class _Rank2:
    """a tower that is not rank one: the rows of two frames are no multiples of each other, every token row has its own scale
    and the e4m3 rounding moves the cosines (FeatureEngine's base * w has cosine 1 between any two rows)"""

    def tower(self, name, px):
        self.tower_calls += 1
        B = px.shape[0]
        base = px.reshape(B, -1)[:, : self.P].reshape(B * self.P, 1)
        w = self.towers[name]["w"][None]
        return base * w + torch.sin(3 * base + 0.7 * w)


class GapEngine(_Rank2, CompactEngine):
    pass


class GapFrameEngine(_Frames, _Rank2, CompactEngine):
    pass


def random_video(seed, T0=40):
    px = torch.rand(T0, 3, 2, 2, generator=torch.Generator().manual_seed(seed))
    return px, px + 0.5


def pair_value(eng, dino, a, b):
    """cos(f_a, f_b) as sims_tensor gives it for the two frames laid adjacent"""
    return eng.sims_tensor(torch.cat([dino[a], dino[b]], 0), 2)[0]


# ------------------------------------------------------------------------------------------------ 1: what the table holds
def test_table_holds_the_pair_similarities_of_the_original_rows():
    eng = GapFrameEngine(N=5)
    frames = make_frames(40)
    ps, pd = _Frames.pixels_from_frames(eng, frames, None)
    fs = encode.export_features_with(eng, ps, pd, (4, 6))
    for gaps, G in (("auto", 2), (5, 5)):
        cs = encode.export_features_with(eng, ps, pd, (4, 6), store="e4m3", gaps=gaps)
        assert cs.gaps == G and tuple(cs.gap_sims.shape) == (G, 39) and cs.gap_sims.dtype == torch.float32
        assert torch.equal(cs.gap_sims[0], cs.sims) and torch.equal(cs.sims, eng.sims_tensor(fs.dino.reshape(-1, eng.H), 40))
        for g in range(1, G + 1):
            for i in range(39):
                want = pair_value(eng, fs.dino, i, i + g) if i + g < 40 else torch.tensor(0.0)
                assert cs.gap_sims[g - 1, i].item() == want.item(), (g, i)
        # the three export routes give the same set, table included
        for other in (encode.compact_features_with(eng, fs, gaps=gaps),
                      encode.export_features_from_frames_with(eng, frames, store="e4m3", slab=16, gaps=gaps)):
            assert sorted(other.tensors()) == sorted(cs.tensors()) and "gap_sims" in other.tensors()
            for k, t in cs.tensors().items():
                assert torch.equal(getattr(other, k), t), k
    # without `gaps` the set is today's: no table, the other tensors unchanged
    plain = encode.export_features_with(eng, ps, pd, (4, 6), store="e4m3")
    assert plain.gap_sims is None and plain.gaps == 1 and "gap_sims" not in plain.tensors()
    for k, t in plain.tensors().items():
        assert torch.equal(getattr(cs, k), t), k


# ------------------------------------------------------------------------------------------------ 2: the `gaps` argument
def test_gaps_argument():
    eng = GapEngine(N=5)
    for T0 in (2, 26, 27, 40, 53):
        ps, pd = pixels(T0)
        cs = encode.export_features_with(eng, ps, pd, SIZE, store="e4m3", gaps="auto")
        assert cs.gaps == min(T0 - 1, math.ceil(T0 / 26)), T0
    ps, pd = pixels(12)
    assert encode.export_features_with(eng, ps, pd, SIZE, store="e4m3", gaps=3).gaps == 3
    assert encode.export_features_with(eng, ps, pd, SIZE, store="e4m3", gaps=500).gaps == 11          # clipped to T0 - 1
    small = GapEngine(N=5, max_num_segments=6)                                                        # "auto" reads the engine's cfg
    assert encode.export_features_with(small, ps, pd, SIZE, store="e4m3", gaps="auto").gaps == math.ceil(12 / 8)
    for bad in (0, -1, 2.0, "all", True):
        with pytest.raises(ValueError, match="gaps"):
            encode.export_features_with(eng, ps, pd, SIZE, store="e4m3", gaps=bad)
    for gaps in ("auto", 2):
        with pytest.raises(ValueError, match="gaps"):
            encode.export_features_with(eng, ps, pd, SIZE, store="f16", gaps=gaps)
        with pytest.raises(ValueError, match="gaps"):
            encode.export_features_with(eng, ps, pd, SIZE, gaps=gaps)
    # one frame: no table, no similarities
    one = encode.export_features_with(eng, ps[:1], pd[:1], SIZE, store="e4m3", gaps="auto")
    assert one.gap_sims is None and one.sims is None and one.gaps == 0
    # a compact set cannot gain gaps: its 16-bit rows are gone
    c2 = encode.export_features_with(eng, ps, pd, SIZE, store="e4m3", gaps=2)
    assert encode.compact_features_with(eng, c2) is c2 and encode.compact_features_with(eng, c2, gaps=2) is c2
    with pytest.raises(ValueError, match="gap"):
        encode.compact_features_with(eng, c2, gaps=3)
    c1 = encode.export_features_with(eng, ps, pd, SIZE, store="e4m3")
    assert encode.compact_features_with(eng, c1, gaps=1) is c1
    with pytest.raises(ValueError, match="gap"):
        encode.compact_features_with(eng, c1, gaps=2)


# ------------------------------------------------------------------------------------------------ 3: the a1 gap bound
def test_auto_covers_every_gap_a1_can_make():
    """a5 ranks the kept frames only when m > max_num_segments + 1 = 25 of them are kept; the neighbours of
    uniform_indices(T0, m) lie at most ceil(T0 / m) <= ceil(T0 / 26) apart"""
    cfg = dict(max_num_segments=24)
    for T0 in (27, 28, 40, 51, 52, 53, 100, 224, 225, 260, 512, 777, 1000, 1200):
        G = encode.auto_gaps(cfg, T0)
        assert G == math.ceil(T0 / 26)
        for m in range(26, T0 + 1):
            idx = seg.uniform_indices(T0, m)
            assert max(b - a for a, b in zip(idx[:-1], idx[1:])) <= G, (T0, m)
            assert min(b - a for a, b in zip(idx[:-1], idx[1:])) >= 1, (T0, m)


# ------------------------------------------------------------------------------------------------ 4: the stored form
def test_format_3_round_trip_and_older_formats(tmp_path):
    eng = GapEngine(N=5)
    ps, pd = pixels(12)
    fs = encode.export_features_with(eng, ps, pd, (360, 640))
    cs = encode.compact_features_with(eng, fs, gaps=3)
    plain = encode.compact_features_with(eng, fs)
    path = str(tmp_path / "video.tdcfeat")
    cs.save(path)
    d = torch.load(path, weights_only=True)
    assert d["format"] == 3 and d["store"] == "e4m3" and tuple(d["gap_sims"].shape) == (3, 11)
    assert sorted(d) == ["dino", "dino_scale", "format", "gap_sims", "image_size", "rows_dtype", "siglip", "siglip_scale",
                         "signature", "sims", "store"]
    back = FeatureSet.load(path)
    assert back.gaps == 3 and back.store == "e4m3" and back.image_size == (360, 640) and back.signature == cs.signature
    assert back.nbytes == cs.nbytes == plain.nbytes + 4 * 3 * 11
    for k, t in cs.tensors().items():
        assert torch.equal(getattr(back, k), t) and getattr(back, k).dtype == t.dtype, k
    host = cs.cpu()
    assert host.gaps == 3 and torch.equal(host.gap_sims, cs.gap_sims) and host.to("cpu") is host
    # no table: format 2 with its keys, and such a file loads with one gap
    plain.save(path)
    d = torch.load(path, weights_only=True)
    assert d["format"] == 2 and "gap_sims" not in d
    back = FeatureSet.load(path)
    assert back.gaps == 1 and back.gap_sims is None and torch.equal(back.sims, cs.sims)
    # format 1
    fs.save(path)
    assert torch.load(path, weights_only=True)["format"] == 1
    old = FeatureSet.load(path)
    assert old.store == "f16" and old.gaps == 0 and old.gap_sims is None


def test_constructor_validates_the_table():
    b, sc = torch.zeros(4, 3, 8, dtype=torch.uint8), torch.ones(4, 3)
    sims = torch.tensor([0.1, 0.2, 0.3])
    table = torch.stack([sims, torch.tensor([0.4, 0.5, 0.0])])
    ok = FeatureSet(b, b, SIZE, None, sc, sc, sims, torch.float16, gap_sims=table)
    assert ok.gaps == 2 and torch.equal(ok.sims, sims)
    only = FeatureSet(b, b, SIZE, None, sc, sc, None, torch.float16, gap_sims=table)                 # sims = row 0
    assert only.gaps == 2 and torch.equal(only.sims, sims)
    assert FeatureSet(b, b, SIZE, None, sc, sc, sims, torch.float16).gaps == 1
    assert FeatureSet(b, b, SIZE, None, sc, sc, None, torch.float16).gaps == 0
    bad = [torch.zeros(2, 4), torch.zeros(3), torch.zeros(0, 3), table.double(), table.tolist(),    # shape, type
           torch.stack([sims + 1e-3, table[1]])]                                                    # row 0 is not sims
    for t in bad:
        with pytest.raises(ValueError, match="gap_sims"):
            FeatureSet(b, b, SIZE, None, sc, sc, sims, torch.float16, gap_sims=t)
    x = torch.zeros(4, 3, 8)
    with pytest.raises(ValueError, match="lossless"):                                               # a table on a lossless set
        FeatureSet(x, x, SIZE, None, gap_sims=table)
    one = torch.zeros(1, 3, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="gap_sims"):                                               # one frame has no pairs
        FeatureSet(one, one, SIZE, None, torch.ones(1, 3), torch.ones(1, 3), None, torch.float16, gap_sims=torch.zeros(1, 0))


def test_stored_sims_reads_what_the_set_holds():
    b, sc = torch.zeros(6, 3, 8, dtype=torch.uint8), torch.ones(6, 3)
    table = torch.tensor([[.01, .12, .23, .34, .45], [.02, .13, .24, .35, 0.], [.03, .14, .25, 0., 0.]])
    cs = FeatureSet(b, b, SIZE, None, sc, sc, None, torch.float16, gap_sims=table)
    assert features.stored_sims(cs, [0, 1, 2, 3, 4, 5]) == table[0].tolist()
    assert features.stored_sims(cs, [0, 2, 3, 5]) == [table[1, 0].item(), table[0, 2].item(), table[1, 3].item()]
    assert features.stored_sims(cs, [1, 4]) == [table[2, 1].item()]
    assert features.stored_sims(cs, [0, 4]) is None and features.stored_sims(cs, [0, 1, 5]) is None     # a gap of 4
    plain = FeatureSet(b, b, SIZE, None, sc, sc, table[0], torch.float16)
    assert features.stored_sims(plain, list(range(6))) == table[0].tolist() and features.stored_sims(plain, [0, 2, 3]) is None
    assert features.stored_sims(FeatureSet(b, b, SIZE, None, sc, sc, None, torch.float16), list(range(6))) is None
    x = torch.zeros(6, 3, 8)
    assert features.stored_sims(FeatureSet(x, x, SIZE), list(range(6))) is None


# ------------------------------------------------------------------------------------------------ 5: the need, then the fix
SEED = 191      # of the seeds 0 .. 299, 54 select differently from the decoded rows at 40 -> 30 frames; this one by a wide move


def test_decoded_rows_flip_the_selection_and_the_table_restores_it():
    eng = GapEngine(N=5)
    ps, pd = random_video(SEED)
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    plain = encode.compact_features_with(eng, fs)
    cs = encode.compact_features_with(eng, fs, gaps="auto")
    assert cs.gaps == 2
    # the need: the rank boundary of the lossless similarities, and how far the decoded rows move the pairs that change sides
    idx = encode.frame_indices(eng.cfg, 40, 4, 30)
    lossless = eng.sims_tensor(encode.feature_rows(eng, fs, idx)[1], 30).tolist()
    decoded = eng.sims_tensor(encode.feature_rows(eng, plain, idx)[1], 30).tolist()
    order = sorted(range(29), key=lambda i: (lossless[i], i))
    margin = lossless[order[24]] - lossless[order[23]]
    flipped = set(seg.select_segments(lossless, 24)) ^ set(seg.select_segments(decoded, 24))
    assert flipped and margin > 1e-5
    assert max(abs(lossless[i] - decoded[i]) for i in flipped) > 10 * margin
    wi, pi, gi = {}, {}, {}
    want = encode.encode_features_with(eng, fs, 4, 4, [1, 2, 3], frame_cap=30, info=wi)
    encode.encode_features_with(eng, plain, 4, 4, [1, 2, 3], frame_cap=30, info=pi)
    assert pi["selection_sims"] == "decoded" and pi["frame_indices"] == wi["frame_indices"] == idx
    assert pi["seg_indices"] != wi["seg_indices"], "the set without a table was expected to select other key frames"
    # the fix
    calls, towers = eng.sims_calls, eng.tower_calls
    got = encode.encode_features_with(eng, cs, 4, 4, [1, 2, 3], frame_cap=30, info=gi)
    assert eng.sims_calls == calls and eng.tower_calls == towers, "a5 or a tower ran on a set that holds the similarities"
    assert gi["selection_sims"] == "stored" and gi["seg_indices"] == wi["seg_indices"] and len(gi["seg_indices"]) == 24
    assert gi["frame_indices"] == idx and gi["final_size"] == wi["final_size"] and got.shape == want.shape
    assert {k: v for k, v in gi.items() if k != "selection_sims"} == wi
    # every frame kept: the g = 1 case of the same lookup, as before
    ai, bi = {}, {}
    encode.encode_features_with(eng, cs, 4, 4, [1, 2, 3], info=ai)
    encode.encode_features_with(eng, fs, 4, 4, [1, 2, 3], info=bi)
    assert eng.sims_calls == calls + 1 and ai["selection_sims"] == "stored" and ai["seg_indices"] == bi["seg_indices"]
    # the prompts form shares the front
    prompts = [dict(budget_text_len=4, n_text_tokens=4, prompt_ids=[5]), dict(budget_text_len=4, n_text_tokens=9, prompt_ids=[7, 8])]
    infos = [{}, {}]
    calls = eng.sims_calls
    encode.encode_features_prompts_with(eng, cs, prompts, frame_cap=30, infos=infos)
    assert eng.sims_calls == calls and all(i["selection_sims"] == "stored" and i["seg_indices"] == wi["seg_indices"] for i in infos)


# ------------------------------------------------------------------------------------------------ 6: no table, no stored selection
def test_one_gap_does_not_cover_sub_sampling():
    eng = GapEngine(N=5)
    ps, pd = random_video(SEED)
    c1 = encode.export_features_with(eng, ps, pd, SIZE, store="e4m3", gaps=1)
    assert c1.gaps == 1 and tuple(c1.gap_sims.shape) == (1, 39)
    plain = encode.export_features_with(eng, ps, pd, SIZE, store="e4m3")
    gi, pi = {}, {}
    calls = eng.sims_calls
    got = encode.encode_features_with(eng, c1, 4, 4, [1, 2, 3], frame_cap=30, info=gi)
    assert eng.sims_calls == calls + 1 and gi["selection_sims"] == "decoded"
    assert torch.equal(got, encode.encode_features_with(eng, plain, 4, 4, [1, 2, 3], frame_cap=30, info=pi)) and gi == pi


# ------------------------------------------------------------------------------------------------ 7: clip
@pytest.mark.parametrize("lo,hi", [(0, 20), (20, 40), (7, 38), (5, 7), (12, 13), (0, 40)])
def test_clip_is_the_export_of_those_frames(lo, hi):
    eng = GapEngine(N=5)
    ps, pd = random_video(3)
    fs = encode.export_features_with(eng, ps, pd, (360, 640))
    part = fs.clip(lo, hi)
    want = encode.export_features_with(eng, ps[lo:hi], pd[lo:hi], (360, 640))
    assert part.store == "f16" and part.frames == hi - lo and part.image_size == (360, 640) and part.signature == fs.signature
    if hi - lo > 1:
        assert torch.equal(encode.encode_features_with(eng, part, 4, 4, [1, 2]), encode.encode_features_with(eng, want, 4, 4, [1, 2]))
    for gaps in (None, 1, 4):
        cs = encode.compact_features_with(eng, fs, gaps=gaps)
        cpart, cwant = cs.clip(lo, hi), encode.compact_features_with(eng, want, gaps=gaps)
        assert cpart.store == "e4m3" and cpart.image_size == (360, 640) and cpart.signature == fs.signature
        assert cpart.rows_dtype == cwant.rows_dtype and cpart.gaps == cwant.gaps
        assert sorted(cpart.tensors()) == sorted(cwant.tensors())
        for k, t in cwant.tensors().items():
            assert torch.equal(getattr(cpart, k), t), (gaps, k)


def test_clip_refuses_frames_outside_the_set():
    x = torch.zeros(4, 3, 8)
    fs = FeatureSet(x, x, SIZE)
    for lo, hi in ((-1, 2), (2, 2), (3, 5), (3, 1)):
        with pytest.raises(ValueError, match="clip"):
            fs.clip(lo, hi)


# ------------------------------------------------------------------------------------------------ 8: the mixin
class GapMixinEngine(_Rank2, CompactMixinEngine):
    """records the info of every encode_features call"""

    def encode_features(self, fs, *a, **kw):
        self.infos = getattr(self, "infos", []) + [kw.get("info")]
        return super().encode_features(fs, *a, **kw)


def test_mixin_selects_from_the_table_and_keeps_table_sets_apart():
    lm = feature_lm(tdc_feature_inputs=True)
    lm.get_model().config.tdc_frame_cap = 30
    eng = lm.get_model()._tdc_encoder = GapMixinEngine(K=3, H=8)
    ps, pd = random_video(SEED)
    fs = encode.export_features_with(eng, ps, pd, SIZE)
    plain = encode.compact_features_with(eng, fs)
    cs = encode.compact_features_with(eng, fs, gaps="auto")
    calls = eng.sims_calls
    want = call(lm, [[fs], [None]], 1)
    assert eng.sims_calls == calls + 1
    got = call(lm, [[cs], [None]], 1)
    assert eng.sims_calls == calls + 1, "a5 ran on a set that holds the similarities"
    other = call(lm, [[plain], [None]], 1)
    wi, gi, oi = eng.infos
    assert "selection_sims" not in wi and gi["selection_sims"] == "stored" and oi["selection_sims"] == "decoded"
    assert gi["seg_indices"] == wi["seg_indices"] != oi["seg_indices"] and len(gi["frame_indices"]) == 30
    assert len(got) == len(want) == 10 and got[4].shape == want[4].shape == other[4].shape and got[8] == want[8]
    # config.tdc_batch_prompts: equal bytes, one set with a table and one without, are two videos (they select differently)
    key = lambda s: encode.same_features_key(eng, s, 4, 30)
    clone = FeatureSet(cs.siglip.clone(), cs.dino.clone(), SIZE, cs.signature, cs.siglip_scale.clone(), cs.dino_scale.clone(),
                       cs.sims.clone(), cs.rows_dtype, cs.gap_sims.clone())
    assert key(cs) == key(clone) != key(plain) and key(plain) == key(encode.compact_features_with(eng, fs))
    prompts = [[1, 2], [3, 4, 5], [6]]
    off = call(lm, [[cs, plain, clone], [None] * 3], 3, prompts)
    lm.get_model().config.tdc_batch_prompts = 4
    same_tuple(call(lm, [[cs, plain, clone], [None] * 3], 3, prompts), off)
    assert eng.prompt_calls == [2], "the table set and its clone form the one group; the set without a table stays alone"
