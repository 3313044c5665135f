"""CPU: the content-keyed frame cache (tdc-video_amd/cache.py) - the fingerprint's host reference, FrameCache's bookkeeping and
the cached orchestration (pipeline.encode_video_cached) on the deterministic CPU engine doubles of test_dist_gloo.py: a cached
encode equals a fresh one bit for bit, whatever the cache already held."""
import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import pipeline
from tdc_video_amd.cache import FrameCache, engine_signature, fingerprint_rows_host, tensor_rows_host
from test_dist_gloo import CASES, FakeEngine, NoisyEngine, _case


# ------------------------------------------------------------------------------------------------ fingerprint (host reference)
def _row(n=2048, seed=0):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def test_fingerprint_deterministic_and_shape():
    r = np.stack([_row(seed=1), _row(seed=2)])
    a, b = fingerprint_rows_host(r), fingerprint_rows_host(r.copy())
    assert a.dtype == np.uint64 and a.shape == (2, 2)
    assert np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1])
    assert np.array_equal(fingerprint_rows_host(r[0]), a[:1])


def test_fingerprint_every_single_bit_flip_changes_it():
    r = _row()
    flips = np.repeat(r[None], r.size * 8, 0)
    bit = np.arange(r.size * 8)
    flips[bit, bit // 8] ^= (1 << (bit % 8)).astype(np.uint8)
    fp = fingerprint_rows_host(np.concatenate([r[None], flips], 0))
    as_pairs = {(int(x), int(y)) for x, y in fp}
    assert len(as_pairs) == fp.shape[0] == 16385            # all flips distinct from each other and from the row


def test_fingerprint_word_swap_and_trailing_zeros():
    r = _row()
    s = r.copy().view("<u8")
    s[[3, 17]] = s[[17, 3]]
    assert not np.array_equal(fingerprint_rows_host(r), fingerprint_rows_host(s.view(np.uint8)))
    short = _row(1001, seed=4)
    fps = {tuple(int(v) for v in fingerprint_rows_host(np.concatenate([short, np.zeros(z, np.uint8)]))[0])
           for z in range(0, 17)}
    assert len(fps) == 17                                     # length is part of the key, trailing zeros included


def test_fingerprint_of_tensor_rows_matches_bytes():
    x = torch.randn(5, 3, 4, 4).to(torch.bfloat16)
    b = tensor_rows_host(x, [4, 1])
    assert b.shape == (2, 3 * 4 * 4 * 2)
    assert np.array_equal(b[0], x[4].contiguous().view(torch.uint8).reshape(-1).numpy())


# ------------------------------------------------------------------------------------------------ CPU engine doubles
class _CacheMixin:
    """the three engine calls the cached path adds, on the host (VideoEncoder: tdc_fingerprint_rows / tdc_pair_cossim /
    tdc_gather_rows)"""
    def fingerprint(self, px, rows):
        return [(int(a), int(b)) for a, b in fingerprint_rows_host(tensor_rows_host(px, rows))]

    def slot_sims(self, slab, pairs, defer=False):
        a = torch.stack([slab[i].reshape(-1) for i, _ in pairs])
        b = torch.stack([slab[j].reshape(-1) for _, j in pairs])
        v = [torch.nn.functional.cosine_similarity(a[k:k + 1], b[k:k + 1], dim=1).item() for k in range(len(pairs))]
        return (lambda: v) if defer else v

    def sims_tensor(self, dino, T):
        f = dino.reshape(T, -1)
        return torch.stack([torch.nn.functional.cosine_similarity(f[k:k + 1], f[k + 1:k + 2], dim=1)[0]
                            for k in range(T - 1)])

    def compact_rows(self, src, idx, cols):
        return src[idx[:, 1].long(), :cols].clone()

    def tower(self, name, px):
        self.tower_frames = getattr(self, "tower_frames", 0) + px.shape[0]
        return super().tower(name, px)


class CFake(_CacheMixin, FakeEngine):
    pass


class CNoisy(_CacheMixin, NoisyEngine):
    pass


def _ccase(name):
    eng, vid, audio, cap = _case(name)
    c = (CNoisy if isinstance(eng, NoisyEngine) else CFake)(max_len=eng.cfg["tokenizer_model_max_length"], N=eng.N,
                                                            **{k: v for k, v in eng.cfg.items() if k not in
                                                               ("tokenizer_model_max_length", "context_token_num",
                                                                "hidden_size")})
    return c, vid, audio, cap


def _enc(eng, vid, audio, cap, cache=None, btl=4, prompt=(1, 2), info=None):
    if cache is None:
        return pipeline.encode_video_with(eng, vid, vid, (384, 384), budget_text_len=btl, n_text_tokens=4 + len(prompt),
                                          prompt_ids=list(prompt), audio=audio, frame_cap=cap, info=info)
    return pipeline.encode_video_cached(eng, cache, vid, vid, (384, 384), btl, 4 + len(prompt), list(prompt), audio, cap,
                                        info=info)


# ------------------------------------------------------------------------------------------------ FrameCache bookkeeping
def _rows(n, N=5, H=8, P=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n * N, H, generator=g), torch.rand(n * P, H, generator=g)


def test_framecache_bytes_lru_budget_and_sharing():
    fb = (5 * 8 + 4 * 8) * 4                          # one frame: X [5, 8] + DINOv2 [4, 8], fp32
    c = FrameCache(3 * fb + fb // 2)
    X, D = _rows(2)
    assert c.store(["a", "b"], X, D, [(1, 4)] * 2, pinned={"a", "b"})
    assert c.capacity == 3 and c.bytes == 2 * fb and len(c) == 2
    assert torch.equal(c.assemble(CFake(), ["b", "a", "b"]), torch.cat([X[5:], X[:5], X[5:]]))
    c.lookup(["a"])                                   # a becomes most recent: b is the LRU frame
    X2, D2 = _rows(2, seed=1)
    assert c.store(["c", "d"], X2, D2, [(1, 4)] * 2, pinned={"c", "d"})
    assert "b" not in c and {"a", "c", "d"} <= set(c._slots)
    st = c.stats()
    assert st["bytes"] == 3 * fb <= c.max_bytes and st["evictions"] == 1 and st["reserved_bytes"] <= c.max_bytes
    assert torch.equal(c.assemble(CFake(), ["a", "c", "d"]), torch.cat([X[:5], X2]))
    # a call whose distinct frames exceed the budget stores nothing
    X3, D3 = _rows(4, seed=2)
    assert not c.store(["e", "f", "g", "h"], X3, D3, [(1, 4)] * 4, pinned={"e", "f", "g", "h"})
    assert c.bytes == 3 * fb and not c.fits(["e", "f", "g", "h"]) and c.fits(["e", "e", "f"])
    # the running call's frames are never evicted
    assert c.store(["i"], *_rows(1, seed=3), [(1, 4)], pinned={"i", "a", "c"})
    assert "d" not in c and {"a", "c", "i"} <= set(c._slots)
    c.clear()
    assert len(c) == 0 and c.bytes == 0 and c.stats()["hits"] == 0


def test_framecache_identical_frames_share_a_slot():
    eng, vid, _, _ = _ccase("plain40")
    vid = vid.clone()
    vid[7] = vid[3]
    c = FrameCache(1 << 30)
    info = {}
    _enc(eng, vid, None, 10 ** 6, cache=c, info=info)
    assert info["cache"]["frames_encoded"] == 39 and len(c) == 39
    keys, _ = FrameCache.frame_keys(eng, vid, vid, [3, 7], (384, 384))
    assert keys[0] == keys[1] and c.slots(keys)[0] == c.slots(keys)[1]


def test_framecache_refuses_other_engine_settings():
    cache = FrameCache(1 << 20, engine_signature(CFake()))
    cache.bind(CFake())
    other = CFake()
    other.dtype = torch.float16
    with pytest.raises(ValueError):
        cache.bind(other)
    with pytest.raises(ValueError):
        FrameCache(0)


# ------------------------------------------------------------------------------------------------ cached orchestration
@pytest.mark.parametrize("name", sorted(CASES))
def test_cached_equals_fresh_and_repeat_encodes_nothing(name):
    eng, vid, audio, cap = _ccase(name)
    want = _enc(eng, vid, audio, cap)
    c = FrameCache(1 << 30)
    i1, i2 = {}, {}
    got = _enc(eng, vid, audio, cap, cache=c, info=i1)
    assert torch.equal(got, want)
    again = _enc(eng, vid.clone(), audio, cap, cache=c, info=i2)          # equal content, new tensor: hits
    assert torch.equal(again, want)
    assert i2["cache"]["frames_encoded"] == 0 and i2["cache"]["pairs_computed"] == 0
    assert i2["cache"]["frames_hit"] == i2["cache"]["frames"]
    ref = {}
    _enc(eng, vid, audio, cap, info=ref)
    for k in ("frame_indices", "seg_indices", "final_size", "n_visual"):
        assert i1[k] == ref[k] == i2[k], k


def test_prompts_that_change_the_frame_count():
    """two prompt lengths keep 60 and 58 frames of 90 (a1 budget): the second call encodes only the frames the first lacks"""
    eng = CFake(max_len=16 + 4 + 20 * 60)                           # 20 tokens per frame at K = 3
    _, vid, _, _ = _ccase("plain61")
    vid = torch.cat([vid, vid[:29] + 100.0])
    c = FrameCache(1 << 30)
    for btl, prompt in ((4, (1, 2)), (40, (5, 6, 7, 8, 9))):
        want = _enc(eng, vid, None, 10 ** 6, btl=btl, prompt=prompt)
        info = {}
        got = _enc(eng, vid, None, 10 ** 6, cache=c, btl=btl, prompt=prompt, info=info)
        assert torch.equal(got, want)
        if btl == 40:
            kept = len(info["frame_indices"])
            assert kept == 58 and 0 < info["cache"]["frames_encoded"] < kept


@pytest.mark.parametrize("name", ["refine61", "refine90_few"])
def test_refinement_band_from_cache(name):
    eng, vid, audio, cap = _ccase(name)
    ref = {}
    want = _enc(eng, vid, audio, cap, info=ref)
    assert ref["refined_pairs"], "the case must refine a band"
    c = FrameCache(1 << 30)
    for _ in range(2):
        info = {}
        assert torch.equal(_enc(eng, vid, audio, cap, cache=c, info=info), want)
        assert info["seg_indices"] == ref["seg_indices"] and info["refined_pairs"] == ref["refined_pairs"]
    assert info["cache"]["pairs_computed"] == 0                     # precise values of the band came from the cache


def test_eviction_sequence_a_b_a_is_exact():
    eng, vid_a, _, cap = _ccase("plain40")
    vid_b = vid_a + 50.0
    fb = (5 * 8 + 4 * 8) * 4
    c = FrameCache(60 * fb)                                          # 1.5 videos of 40 frames
    for v in (vid_a, vid_b, vid_a):
        info = {}
        assert torch.equal(_enc(eng, v, None, cap, cache=c, info=info), _enc(eng, v, None, cap))
        assert c.bytes <= c.max_bytes and c.stats()["reserved_bytes"] <= c.max_bytes
    assert c.stats()["evictions"] > 0


def test_budget_below_one_video_bypasses():
    eng, vid, _, cap = _ccase("plain40")
    fb = (5 * 8 + 4 * 8) * 4
    c = FrameCache(10 * fb)
    want = _enc(eng, vid, None, cap)
    for _ in range(2):
        info = {}
        assert torch.equal(_enc(eng, vid, None, cap, cache=c, info=info), want)
        assert info["cache"]["bypassed"]
    assert c.bytes <= c.max_bytes


# ------------------------------------------------------------------------------------------------ boundary: config key
def test_config_key_validation_and_off_states():
    from test_host_logic import build_stub_lm, tiny_config
    assert build_stub_lm(tiny_config()).get_model().tdc_video_cache() is None                     # absent: off
    assert build_stub_lm(tiny_config(tdc_video_cache_bytes=0)).get_model().tdc_video_cache() is None
    assert build_stub_lm(tiny_config(tdc_video_cache_bytes=1 << 30, tdc_shard_frames=True)).get_model() \
        .tdc_video_cache() is None                                                                # sharded: ignored
    for bad in (-1, 1.5, "1GB", True):
        with pytest.raises(ValueError):
            build_stub_lm(tiny_config(tdc_video_cache_bytes=bad)).get_model().tdc_video_cache()
    build_stub_lm(tiny_config()).get_model().tdc_video_cache_clear()                              # off: a no-op
