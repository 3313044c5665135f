"""CPU: the host side of the multi-prompt compressor path - grouping, the three index maps of a group,
compress_many_with / encode_video_prompts_with against per-prompt calls on an engine double."""
import random

import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import pipeline, segment as seg
from test_dist_gloo import FakeEngine, make_video


class MultiEngine(FakeEngine):
    """FakeEngine whose compress_frames also takes the multi-prompt form: per VIRTUAL frame the arithmetic of the single form
    on the distinct frame kv_src names, the query block qsrc names and the prompt frame_prompt names - and which counts what a
    shared pass is meant to save (frames gathered, key frames pooled, passes)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.passes, self.frames_gathered, self.keys_pooled, self.multi_calls = 0, 0, 0, 0

    @staticmethod
    def _text(ids):
        return 0.0 if ids is None else 0.125 * len(ids) + 1e-3 * sum(ids)

    def make_queries(self, Xf, N, Nf, key_rows):
        self.keys_pooled += len(key_rows)
        return super().make_queries(Xf, N, Nf, key_rows)

    def compress_frames(self, Xf, Nf, frame_rows, qtable, qsrc, prompt_ids, keep=None, multi=None):
        self.passes += 1
        self.frames_gathered += len(frame_rows)
        if multi is None:
            out = [qtable[q * self.K:(q + 1) * self.K] * 2.0 - Xf[f * Nf:(f + 1) * Nf].mean(0, keepdim=True) + self._text(prompt_ids)
                   for f, q in zip(frame_rows, qsrc)]
            return torch.cat(out, 0)
        self.multi_calls += 1
        assert len(multi["kv_src"]) == len(qsrc) == len(multi["frame_prompt"])
        out = []
        for u, q, p in zip(multi["kv_src"], qsrc, multi["frame_prompt"]):
            f = frame_rows[u]
            ids = prompt_ids[p]
            out.append(qtable[q * self.K:(q + 1) * self.K] * 2.0 - Xf[f * Nf:(f + 1) * Nf].mean(0, keepdim=True)
                       + self._text(ids if ids else None))
        return torch.cat(out, 0)


# ---------------------------------------------------------------------------------------------------------------- grouping
def test_prompt_groups_order_and_max_prompts():
    g = pipeline.prompt_groups([0] * 7, [5] * 7, [10] * 7, 16, 3)
    assert g == [[0, 1, 2], [3, 4, 5], [6]]
    assert pipeline.prompt_groups([0] * 3, [5] * 3, [10] * 3, 16, 1) == [[0], [1], [2]]      # every group of one: the old path
    with pytest.raises(ValueError):
        pipeline.prompt_groups([0], [5], [10], 16, 0)


def test_prompt_groups_split_on_a1_selection():
    g = pipeline.prompt_groups(["a", "b", "a", "b", "a"], [4] * 5, [6] * 5, 16, 8)
    assert g == [[0, 2, 4], [1, 3]]
    assert all(len({["a", "b", "a", "b", "a"][p] for p in grp}) == 1 for grp in g)


def test_prompt_groups_padding_limit():
    K, F = 16, 10
    lens = [6, 40, 6, 7]
    # 6 next to 40: pad 34 F of 2 * 56 F rows = 0.30 > 1/4 -> the long prompt opens its own group, and takes what follows it
    g = pipeline.prompt_groups([0] * 4, lens, [F] * 4, K, 8, 0.25)
    assert g[0] == [0]
    for grp in g:
        Lmax = max(lens[p] for p in grp)
        pad = sum((Lmax - lens[p]) * F for p in grp)
        assert pad <= 0.25 * sum((K + Lmax) * F for p in grp)
    assert pipeline.prompt_groups([0] * 4, lens, [F] * 4, K, 8, 1.0) == [[0, 1, 2, 3]]
    assert pipeline.prompt_groups([0] * 4, lens, [F] * 4, K, 8, 0.0) == [[0], [1], [2], [3]]
    assert pipeline.prompt_groups([0] * 3, [6, 6, 6], [F] * 3, K, 8, 0.0) == [[0, 1, 2]]       # no padding at all
    # the frame stride stays below the 256 query rows from which tdc_attention's AUTO form changes kernels
    assert pipeline.prompt_groups([0] * 2, [100, 112], [F] * 2, 144, 8, 1.0) == [[0], [1]]
    assert pipeline.prompt_groups([0] * 2, [100, 111], [F] * 2, 144, 8, 1.0) == [[0, 1]]


# -------------------------------------------------------------------------------------------------------------------- maps
def _random_plans(rng, n):
    T = rng.randint(6, 40)
    N, K = rng.choice([5, 9]), rng.choice([2, 3])
    cuts = sorted(rng.sample(range(1, T), rng.randint(1, min(8, T - 1))))
    seg_idx = [0] + cuts
    static = rng.random() < 0.7
    total = len(seg.emit_pairs(seg.emit_plan(T, N, K, seg_idx, 10 ** 9, static), N, K))
    budgets = [rng.choice([10 ** 9, max(1, total - rng.randint(0, total // 2)), max(1, total // 3)]) for _ in range(n)]
    return T, N, K, [seg.emit_plan(T, N, K, seg_idx, b, static) for b in budgets]


def test_prompt_maps_name_each_plans_own_frames_and_chunks():
    rng = random.Random(7)
    for _ in range(60):
        T, N, K, plans = _random_plans(rng, rng.randint(2, 5))
        # un-equal comp_frames too: drop a random tail of one plan's compressed frames (what a plan of a shorter video would hold)
        if plans[0]["comp_frames"]:
            cut = rng.randint(1, len(plans[0]["comp_frames"]))
            plans[0] = dict(comp_frames=plans[0]["comp_frames"][:cut], comp_chunk=plans[0]["comp_chunk"][:cut],
                            key_frames=plans[0]["key_frames"])
        m = pipeline.prompt_maps(plans)
        F = sum(len(pl["comp_frames"]) for pl in plans)
        assert len(m["kv_src"]) == len(m["qsrc"]) == len(m["frame_prompt"]) == F == m["offsets"][-1]
        assert m["enc_frames"] == sorted(set(m["enc_frames"])) and m["key_frames"] == sorted(set(m["key_frames"]))
        if F:
            assert 0 <= min(m["kv_src"]) and max(m["kv_src"]) < len(m["enc_frames"])
            assert 0 <= min(m["qsrc"]) and max(m["qsrc"]) < len(m["key_frames"])
            assert 0 <= min(m["frame_prompt"]) and max(m["frame_prompt"]) < len(plans)
        for p, pl in enumerate(plans):
            lo, hi = m["offsets"][p], m["offsets"][p + 1]
            assert hi - lo == len(pl["comp_frames"])
            for j in range(lo, hi):
                assert m["frame_prompt"][j] == p
                assert m["enc_frames"][m["kv_src"][j]] == pl["comp_frames"][j - lo]
                assert m["key_frames"][m["qsrc"][j]] == pl["key_frames"][pl["comp_chunk"][j - lo]]
        assert set(pipeline.prompt_maps(plans, learned=True)["qsrc"]) <= {0}


# --------------------------------------------------------------------------------------------- the double, end to end
def _prompts(n, rng, n_text=None):
    out = []
    for i in range(n):
        L = rng.randint(0, 9)
        out.append(dict(budget_text_len=4, n_text_tokens=rng.choice([4, 30, 60]) if n_text is None else n_text,
                        prompt_ids=[rng.randint(1, 50) for _ in range(L)]))
    return out


@pytest.mark.parametrize("cfg", [dict(), dict(add_static=False), dict(query_type="learned"), dict(text_input=False)])
def test_compress_many_equals_per_prompt_compress(cfg):
    rng = random.Random(3)
    T = 30
    eng = MultiEngine(K=3, H=8, N=5, max_len=200, **cfg)           # a small budget: the tails of most plans are clipped
    X = torch.rand(T * eng.N, eng.H)
    seg_idx = [0, 4, 5, 11, 20, 26]
    for audio in (None, torch.rand(T, 2, eng.H)):
        prompts = _prompts(6, rng)
        infos = [{} for _ in prompts]
        got = pipeline.compress_many_with(eng, X, T, eng.N, seg_idx, prompts, audio, infos, max_prompts=4, pad_fraction=1.0)
        for p, pr in enumerate(prompts):
            want_info = {}
            want = pipeline.compress_with(eng, X, T, eng.N, seg_idx, pipeline.text_prompt(eng.cfg, pr["prompt_ids"]),
                                          pipeline.visual_budget(eng.cfg, pr["n_text_tokens"]), audio, None, None, want_info)
            assert torch.equal(got[p], want), p
            assert {k: v for k, v in infos[p].items() if k != "prompts"} == want_info
            assert set(infos[p]["prompts"]) == {"group", "group_size", "pad_rows", "shared_kv_frames"}
        assert [i["prompts"]["group"] for i in infos] == [0, 0, 0, 0, 1, 1]
        assert infos[0]["prompts"]["group_size"] == 4


def test_shared_pass_gathers_and_pools_once():
    rng = random.Random(5)
    T = 30
    seg_idx = [0, 4, 5, 11, 20, 26]
    prompts = _prompts(5, rng, n_text=4)
    a, b = MultiEngine(K=3, H=8, N=5), MultiEngine(K=3, H=8, N=5)
    X = torch.rand(T * a.N, a.H)
    pipeline.compress_many_with(a, X, T, a.N, seg_idx, prompts, max_prompts=8, pad_fraction=1.0)
    for pr in prompts:
        pipeline.compress_with(b, X, T, b.N, seg_idx, pr["prompt_ids"], pipeline.visual_budget(b.cfg, pr["n_text_tokens"]))
    assert (a.passes, a.multi_calls) == (1, 1) and b.passes == 5
    assert a.frames_gathered * 5 == b.frames_gathered and a.keys_pooled * 5 == b.keys_pooled


def test_group_of_one_and_engines_without_the_form_take_the_old_path():
    T = 12
    seg_idx = [0, 5]
    eng = MultiEngine(K=3, H=8, N=5)
    X = torch.rand(T * eng.N, eng.H)
    one = [dict(n_text_tokens=4, prompt_ids=[3, 4])]
    infos = [{}]
    pipeline.compress_many_with(eng, X, T, eng.N, seg_idx, one, infos=infos)
    assert eng.multi_calls == 0 and infos[0]["prompts"]["group_size"] == 1 and infos[0]["prompts"]["pad_rows"] == 0
    eng.multi_prompt_ok = lambda nf: False                           # e.g. the whole-block cross-attention kernel
    two = one + [dict(n_text_tokens=4, prompt_ids=[5])]
    got = pipeline.compress_many_with(eng, X, T, eng.N, seg_idx, two)
    assert eng.multi_calls == 0
    assert torch.equal(got[1], pipeline.compress_with(eng, X, T, eng.N, seg_idx, [5], pipeline.visual_budget(eng.cfg, 4)))


def test_encode_video_prompts_equals_per_prompt_encode_video():
    T0 = 40
    vid = make_video(T0)
    eng = MultiEngine(K=3, H=8, N=5, max_len=400, max_num_segments=6)
    audio = dict(per_second=torch.rand(T0, 2, eng.H))
    rng = random.Random(11)
    prompts = _prompts(5, rng)
    prompts[3]["budget_text_len"] = 10 ** 6                          # a prompt long enough to change a1: its own selection
    for aud in (None, audio):
        infos = [{} for _ in prompts]
        got = pipeline.encode_video_prompts_with(eng, vid, vid, (2, 2), prompts, aud, 224, None, infos, None, 8, 1.0)
        sel = set()
        for p, pr in enumerate(prompts):
            want_info = {}
            want = pipeline.encode_video_with(eng, vid, vid, (2, 2), pr["budget_text_len"], pr["n_text_tokens"], pr["prompt_ids"],
                                              aud, 224, None, None, None, want_info)
            assert torch.equal(got[p], want), p
            assert {k: v for k, v in infos[p].items() if k != "prompts"} == want_info
            sel.add(tuple(want_info["frame_indices"]))
        if len(sel) > 1:
            assert infos[3]["prompts"]["group"] != infos[0]["prompts"]["group"] and infos[3]["prompts"]["group_size"] == 1


# ------------------------------------------------------------------------------------------------------------ the config keys
def test_config_keys_validate_and_name_themselves():
    from test_host_logic import build_stub_lm, tiny_config
    m = lambda **kw: build_stub_lm(tiny_config(**kw)).get_model()
    assert m().tdc_batch_prompts() == 0 and m(tdc_batch_prompts=None).tdc_batch_prompts() == 0     # absent: off
    assert m(tdc_batch_prompts=0).tdc_batch_prompts() == 0 and m(tdc_batch_prompts=8).tdc_batch_prompts() == 8
    for bad in (-1, 2.5, "8", True):
        with pytest.raises(ValueError, match="tdc_batch_prompts"):
            m(tdc_batch_prompts=bad).tdc_batch_prompts()
    assert m().tdc_prompt_pad_fraction() == 0.25
    assert m(tdc_prompt_pad_fraction=0).tdc_prompt_pad_fraction() == 0.0
    assert m(tdc_prompt_pad_fraction=1).tdc_prompt_pad_fraction() == 1.0
    assert m(tdc_prompt_pad_fraction=0.5).tdc_prompt_pad_fraction() == 0.5
    for bad in (-0.1, 1.5, "0.25", True):
        with pytest.raises(ValueError, match="tdc_prompt_pad_fraction"):
            m(tdc_prompt_pad_fraction=bad).tdc_prompt_pad_fraction()
    # the paths that do not compose: the error names both keys; with the key off the others stand as they are
    for other, v in (("tdc_shard_frames", True), ("tdc_batch_frames", 512)):
        with pytest.raises(ValueError) as ei:
            m(tdc_batch_prompts=4, **{other: v}).tdc_batch_prompts()
        assert "tdc_batch_prompts" in str(ei.value) and other in str(ei.value)
        assert m(tdc_batch_prompts=0, **{other: v}).tdc_batch_prompts() == 0
    assert m(tdc_batch_prompts=4, tdc_batch_frames=0).tdc_batch_prompts() == 4
    assert m(tdc_batch_prompts=4, tdc_video_cache_bytes=1 << 30).tdc_batch_prompts() == 4
