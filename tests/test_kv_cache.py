"""CPU: the kept cross-attention K/V of the frame cache - what names an entry, the budget of its own,
what the orchestration hands to compress_frames, and the config key.  The engine is the CPU double of test_video_cache.py with
the multi-prompt form of test_multi_prompt.py; its "K/V projection" is the gathered rows themselves, and a pass that takes a
ready buffer computes from that buffer alone, so a wrong or stale entry changes the result."""
import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import encode, pipeline
from tdc_video_amd.cache import FrameCache, KeptKV, fingerprint_rows_host
from test_dist_gloo import make_video
from test_multi_prompt import MultiEngine
from test_video_cache import CFake, _CacheMixin

SIZE = (384, 384)


class KVEngine(_CacheMixin, MultiEngine):
    dev = "cpu"
    kv_ok = True

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls, self.enc_gathers = [], 0

    def fingerprint(self, px, rows, row_bytes=None, row_stride=None):
        if row_bytes is None:
            return super().fingerprint(px, rows)
        b = px.detach().contiguous().view(-1).view(torch.uint8).numpy()
        return [(int(a), int(c)) for a, c in
                fingerprint_rows_host(np.stack([b[r * row_stride:r * row_stride + row_bytes] for r in rows]))]

    def kv_cache_ok(self, Nf):
        return self.kv_ok

    def kv_entry_bytes(self, U, Nf):
        return U * Nf * self.H * 4

    def kv_alloc(self, U, Nf):
        return torch.full((U * Nf, self.H), float("nan"))

    def compress_frames(self, Xf, Nf, frame_rows, qtable, qsrc, prompt_ids, keep=None, multi=None, kv=None):
        self.calls.append((len(frame_rows), multi is not None, None if kv is None else ("ready" if kv.ready else "fill")))
        if kv is None:
            self.enc_gathers += 1
            return super().compress_frames(Xf, Nf, frame_rows, qtable, qsrc, prompt_ids, keep, multi)
        assert type(kv).__name__ == KeptKV.__name__ and tuple(kv.buf.shape) == (len(frame_rows) * Nf, self.H)
        if not kv.ready:
            self.enc_gathers += 1
            kv.buf.copy_(torch.cat([Xf[f * Nf:(f + 1) * Nf] for f in frame_rows]))
        # everything behind the projection reads the kept rows alone: frame u of the buffer stands for frame_rows[u]
        return super().compress_frames(kv.buf, Nf, list(range(len(frame_rows))), qtable, qsrc, prompt_ids, keep, multi)


def _eng(**kw):
    return KVEngine(K=3, H=8, N=5, max_len=10 ** 9, **kw)


def _audio(T0, seed=11):
    return {"per_second": torch.rand(T0, 2, 8, generator=torch.Generator().manual_seed(seed))}


def _enc(eng, vid, cache=None, prompt=(1, 2), cap=10 ** 6, audio=None, size=SIZE, info=None, btl=4):
    return encode.encode_video_with(eng, vid, vid, size, btl, 4 + len(prompt), list(prompt), audio, cap, None, None, None,
                                    info, cache)


ENTRY40 = 15 * 5 * 8 * 4        # plain 40-frame video at max_num_segments 24: 25 static + 15 compressed frames of 5 rows


# ------------------------------------------------------------------------------------------------------------------- keys
def test_one_entry_per_video_and_selection():
    eng, vid = _eng(), make_video(40)
    c = FrameCache(1 << 30, kv_bytes=1 << 20)
    i1, i2 = {}, {}
    want1, want2 = _enc(eng, vid), _enc(eng, vid, prompt=(5, 6, 7))
    assert torch.equal(_enc(eng, vid, c, info=i1), want1)
    assert torch.equal(_enc(eng, vid.clone(), c, prompt=(5, 6, 7), info=i2), want2)      # another prompt, a re-decoded copy
    assert i1["cache"]["kv"] == dict(state="filled", frames=15, bytes=ENTRY40)
    assert i2["cache"]["kv"] == dict(state="hit", frames=15, bytes=ENTRY40)
    assert c.kv_stats() == dict(hits=1, misses=1, fills=1, evictions=0, bypassed=0, entries=1, bytes=ENTRY40, max_bytes=1 << 20)
    for name, kw in (("frame cap", dict(cap=30)), ("image_size", dict(size=(384, 380))), ("audio", dict(audio=_audio(40))),
                     ("other audio", dict(audio=_audio(40, seed=12)))):
        n, info = c.kv_stats()["entries"], {}
        assert torch.equal(_enc(eng, vid, c, info=info, **kw), _enc(eng, vid, **kw)), name
        assert info["cache"]["kv"]["state"] == "filled" and c.kv_stats()["entries"] == n + 1, name
        info = {}
        assert torch.equal(_enc(eng, vid, c, prompt=(9,), info=info, **kw), _enc(eng, vid, prompt=(9,), **kw)), name
        assert info["cache"]["kv"]["state"] == "hit" and c.kv_stats()["entries"] == n + 1, name
    # the same audio content in another tensor hits; two frames swapped name another entry
    info = {}
    _enc(eng, vid, c, audio={"per_second": _audio(40)["per_second"].clone()}, info=info)
    assert info["cache"]["kv"]["state"] == "hit"
    perm = vid.clone()
    perm[[30, 31]] = vid[[31, 30]]
    info = {}
    assert torch.equal(_enc(eng, perm, c, info=info), _enc(eng, perm))
    assert info["cache"]["kv"]["state"] == "filled"


def test_kv_key_covers_order_rows_size_and_audio():
    keys = ["a", "b", "c", "d"]
    base = encode.kv_key(encode.kv_store(None, keys, SIZE), [1, 2, 3], 5)
    assert base == encode.kv_key(encode.kv_store(None, list(keys), SIZE), [1, 2, 3], 5)
    others = [encode.kv_key(encode.kv_store(None, keys, SIZE), [1, 3, 2], 5),                    # a permuted frame
              encode.kv_key(encode.kv_store(None, keys, SIZE), [1, 2], 5),
              encode.kv_key(encode.kv_store(None, keys, SIZE), [1, 2, 3], 7),                    # rows per frame (audio rows)
              encode.kv_key(encode.kv_store(None, keys, (384, 380)), [1, 2, 3], 5),
              encode.kv_key(encode.kv_store(None, keys, SIZE, ("audio", (1, 0, 1))), [1, 2, 3], 5),
              encode.kv_key(encode.kv_store(None, ["a", "b", "c", "x"], SIZE), [1, 2, 3], 5)]
    assert len(set(others + [base])) == len(others) + 1
    assert others[4] != encode.kv_key(encode.kv_store(None, keys, SIZE, ("audio", (1, 1, 0))), [1, 2, 3], 5)


# ----------------------------------------------------------------------------------------------------------------- budget
def test_budget_lru_pinned_and_oversize():
    c = FrameCache(1 << 20, kv_bytes=100)
    bufs = {k: torch.zeros(1) for k in "abcd"}
    for k in "abc":
        assert c.kv_get(k) is None and c.kv_room(30)
        c.kv_put(k, bufs[k], 30)
    assert c.kv_get("a") is bufs["a"]                              # a becomes most recent: b is the LRU entry
    assert c.kv_room(40)                                           # 90 + 40 > 100: b leaves, a and c stay
    c.kv_put("d", bufs["d"], 40)
    assert c.kv_get("b") is None and c.kv_get("c") is bufs["c"] and c.kv_get("a") is bufs["a"]
    assert c.kv_stats()["bytes"] == 100 and c.kv_stats()["evictions"] == 1
    # the entries the running call uses are never evicted: d is the LRU entry, yet pinned - c leaves
    assert c.kv_room(30, pinned={"d"})
    assert c.kv_get("d") is bufs["d"] and c.kv_get("c") is None
    # an entry above the budget - or above what the pinned ones leave - is not stored, and evicts nothing
    before = c.kv_stats()
    assert not c.kv_room(101) and not c.kv_room(40, pinned={"a", "d"})
    after = c.kv_stats()
    assert after["entries"] == before["entries"] == 2 and after["bytes"] == before["bytes"] and after["bypassed"] == 2
    st = c.stats()
    assert "kv" not in st and st["bytes"] == 0 and c.bytes == 0    # the frame store does not know the K/V budget
    c.clear()
    assert c.kv_stats() == dict(hits=0, misses=0, fills=0, evictions=0, bypassed=0, entries=0, bytes=0, max_bytes=100)
    with pytest.raises(ValueError):
        FrameCache(1 << 20, kv_bytes=-1)


def test_budget_of_one_entry_refills_and_below_one_bypasses():
    eng, vid_a = _eng(), make_video(40)
    vid_b = vid_a + 50.0
    c = FrameCache(1 << 30, kv_bytes=ENTRY40 + ENTRY40 // 2)
    states = []
    for v in (vid_a, vid_b, vid_a, vid_a):
        info = {}
        assert torch.equal(_enc(eng, v, c, info=info), _enc(eng, v))
        states.append(info["cache"]["kv"]["state"])
        assert c.kv_stats()["bytes"] <= c.kv_max_bytes
    assert states == ["filled", "filled", "filled", "hit"] and c.kv_stats()["evictions"] == 2
    c = FrameCache(1 << 30, kv_bytes=ENTRY40 - 1)
    n = len(eng.calls)
    for _ in range(2):
        info = {}
        assert torch.equal(_enc(eng, vid_a, c, info=info), _enc(eng, vid_a))
        assert info["cache"]["kv"] == dict(state="bypassed", frames=15, bytes=ENTRY40)
    assert all(kv is None for _, _, kv in eng.calls[n:]) and c.kv_stats()["entries"] == 0


def test_kv_off_is_todays_cache():
    vid = make_video(40)
    runs = []
    for make in (lambda: FrameCache(1 << 30), lambda: FrameCache(1 << 30, None, 0), lambda: FrameCache(1 << 30, kv_bytes=0)):
        eng, c, infos = _eng(), make(), []
        for prompt in ((1, 2), (5, 6, 7)):
            info = {}
            _enc(eng, vid, c, prompt=prompt, info=info)
            infos.append(info)
        runs.append((eng.calls, eng.enc_gathers, c.stats(), infos, c.bytes, c.capacity))
    assert runs[0] == runs[1] == runs[2]
    assert all(kv is None for _, _, kv in runs[0][0]) and all("kv" not in i["cache"] for i in runs[0][3])
    # an engine of today (no kv= on compress_frames, no kv_cache_ok) behind a K/V budget: reported, and the plain path runs
    old = CFake()
    c = FrameCache(1 << 30, kv_bytes=1 << 20)
    info, ref = {}, {}
    want = pipeline.encode_video_with(old, vid, vid, SIZE, 4, 6, [1, 2], None, 10 ** 6, info=ref)
    assert torch.equal(pipeline.encode_video_cached(old, c, vid, vid, SIZE, 4, 6, [1, 2], None, 10 ** 6, info=info), want)
    assert info["cache"]["kv"] == dict(state="unsupported", frames=15, bytes=0) and c.kv_stats()["entries"] == 0
    assert {k: v for k, v in info.items() if k != "cache"} == ref


# ------------------------------------------------------------------------------------------------------------------ calls
def test_hit_hands_over_a_ready_buffer_and_gathers_nothing():
    eng, vid = _eng(), make_video(40)
    c = FrameCache(1 << 30, kv_bytes=1 << 20)
    ref, i1, i2 = {}, {}, {}
    want = _enc(eng, vid, info=ref)
    n, g = len(eng.calls), eng.enc_gathers
    assert torch.equal(_enc(eng, vid, c, info=i1), want)
    assert eng.calls[n:] == [(15, False, "fill")] and eng.enc_gathers == g + 1
    assert torch.equal(_enc(eng, vid, c, info=i2), want)
    assert eng.calls[n + 1:] == [(15, False, "ready")] and eng.enc_gathers == g + 1          # no enc gather on the hit
    for info in (i1, i2):
        assert {k: v for k, v in info.items() if k != "cache"} == ref
        assert {k: v for k, v in info["cache"].items() if k != "kv"}.keys() == \
            FrameCache.call_info(c.stats(), c.stats(), [], []).keys()
    # an engine that cannot take the form here (the whole-block kernel): "unsupported", the plain path, nothing stored
    eng.kv_ok = False
    c2 = FrameCache(1 << 30, kv_bytes=1 << 20)
    info = {}
    assert torch.equal(_enc(eng, vid, c2, info=info), want)
    assert info["cache"]["kv"]["state"] == "unsupported" and eng.calls[-1] == (15, False, None)
    # a video without compressed frames has no K/V
    info = {}
    _enc(_eng(), make_video(20), FrameCache(1 << 30, kv_bytes=1 << 20), info=info)
    assert info["cache"]["kv"] == dict(state="bypassed", frames=0, bytes=0)


def test_multi_prompt_groups_share_the_entry():
    vid = make_video(40)
    eng = KVEngine(K=3, H=8, N=5, max_len=400, max_num_segments=6)
    prompts = [dict(budget_text_len=4, n_text_tokens=6, prompt_ids=[1, 2 + i]) for i in range(4)]   # one plan: equal frames
    want = [encode.encode_video_with(eng, vid, vid, SIZE, p["budget_text_len"], p["n_text_tokens"], p["prompt_ids"])
            for p in prompts]
    plain = [{} for _ in prompts]
    encode.encode_video_prompts_with(eng, vid, vid, SIZE, prompts, infos=plain, cache=FrameCache(1 << 30), max_prompts=2,
                                     pad_fraction=1.0)
    c = FrameCache(1 << 30, kv_bytes=1 << 20)
    n = len(eng.calls)
    infos = [{} for _ in prompts]
    got = encode.encode_video_prompts_with(eng, vid, vid, SIZE, prompts, infos=infos, cache=c, max_prompts=2, pad_fraction=1.0)
    for p in range(4):
        assert torch.equal(got[p], want[p]), p
        assert {k: v for k, v in infos[p].items() if k != "cache"} == {k: v for k, v in plain[p].items() if k != "cache"}
    multi = [x for x in eng.calls[n:] if x[1]]
    assert len(multi) == 2 and multi[0][0] == multi[1][0]          # two groups over the same distinct frames: fill, then hit
    assert [x[2] for x in multi] == ["fill", "ready"]
    assert [i["cache"]["kv"]["state"] for i in infos] == ["filled", "filled", "hit", "hit"]
    # a later call with other prompts hits, whatever its grouping
    later = [dict(budget_text_len=4, n_text_tokens=7, prompt_ids=[3, 4, 5]), dict(budget_text_len=4, n_text_tokens=6, prompt_ids=[8])]
    want = [encode.encode_video_with(eng, vid, vid, SIZE, p["budget_text_len"], p["n_text_tokens"], p["prompt_ids"])
            for p in later]
    n = len(eng.calls)
    infos = [{} for _ in later]
    got = encode.encode_video_prompts_with(eng, vid, vid, SIZE, later, infos=infos, cache=c, max_prompts=8, pad_fraction=1.0)
    for p in range(len(later)):
        assert torch.equal(got[p], want[p]), p
    fills = c.kv_stats()["fills"]
    assert eng.calls[n:] and all(x[2] is not None for x in eng.calls[n:])
    got2 = encode.encode_video_prompts_with(eng, vid, vid, SIZE, later, cache=c, max_prompts=8, pad_fraction=1.0)
    assert c.kv_stats()["fills"] == fills and all(torch.equal(a, b) for a, b in zip(got, got2))


# ------------------------------------------------------------------------------------------------------------ the config key
def test_config_key_validates_and_names_itself():
    from test_host_logic import build_stub_lm, tiny_config
    m = lambda **kw: build_stub_lm(tiny_config(**kw)).get_model()
    assert m().tdc_kv_cache_bytes() == 0 and m(tdc_kv_cache_bytes=None).tdc_kv_cache_bytes() == 0
    assert m(tdc_kv_cache_bytes=0).tdc_kv_cache_bytes() == 0
    assert m(tdc_kv_cache_bytes=1 << 28, tdc_video_cache_bytes=1 << 30).tdc_kv_cache_bytes() == 1 << 28
    for bad in (-1, 1.5, "1GB", True):
        with pytest.raises(ValueError, match="tdc_kv_cache_bytes"):
            m(tdc_kv_cache_bytes=bad, tdc_video_cache_bytes=1 << 30).tdc_kv_cache_bytes()
        with pytest.raises(ValueError, match="tdc_kv_cache_bytes"):
            m(tdc_kv_cache_bytes=bad, tdc_video_cache_bytes=1 << 30).tdc_video_cache()
    with pytest.raises(ValueError) as ei:                           # it lives in the frame cache
        m(tdc_kv_cache_bytes=1 << 28).tdc_kv_cache_bytes()
    assert "tdc_kv_cache_bytes" in str(ei.value) and "tdc_video_cache_bytes" in str(ei.value)
    for other, v in (("tdc_shard_frames", True), ("tdc_shard_cache_bytes", 1 << 30), ("tdc_batch_frames", 512),
                     ("tdc_feature_inputs", True)):
        with pytest.raises(ValueError) as ei:
            m(tdc_kv_cache_bytes=1 << 28, tdc_video_cache_bytes=1 << 30, **{other: v}).tdc_kv_cache_bytes()
        assert "tdc_kv_cache_bytes" in str(ei.value) and other in str(ei.value)
        assert m(tdc_kv_cache_bytes=0, tdc_video_cache_bytes=1 << 30, **{other: v}).tdc_kv_cache_bytes() == 0
    for other, v in (("tdc_batch_prompts", 4), ("tdc_frame_inputs", True)):
        assert m(tdc_kv_cache_bytes=1 << 28, tdc_video_cache_bytes=1 << 30, **{other: v}).tdc_kv_cache_bytes() == 1 << 28


# -------------------------------------------------------------------------------------------------------------- the C ABI
def test_ctypes_struct_mirrors_the_header():
    import ctypes as C
    import os
    import re
    from tdc_video_amd import lib as L
    names = [n for n, _ in L.QformerModel._fields_]
    assert names[-3:] == ["prompts", "kv_keep", "kv_state"]
    assert dict(L.QformerModel._fields_)["kv_keep"] is C.c_void_p and dict(L.QformerModel._fields_)["kv_state"] is C.c_int
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdc_hip.h")).read()
    body = hdr[:hdr.index("} tdc_qformer_model;")]
    assert re.search(r"void\*\s*kv_keep;\s*int\s+kv_state;\s*$", body)          # appended behind everything else
    assert "kv_keep" not in L.SIGNATURES and not any("kv" in k for k in L.SIGNATURES)


# ------------------------------------------------------------------------------------------------- the composite's launches
def _kv_traces(workdir):
    """builds tests/kv_trace/kv_trace.cpp with api.cpp by the host compiler (as test_api_trace does) -> {case: trace lines}"""
    import os
    import subprocess
    from test_api_trace import ROOT, _toolchain
    cxx, inc = _toolchain()
    assert cxx, "no host C++ compiler ($CXX, else g++)"
    assert inc, "no ROCm headers (hip/hip_runtime.h declares the one runtime call api.cpp makes)"
    exe = os.path.join(str(workdir), "kv_trace")
    src = [os.path.join(ROOT, "tdc-video_amd", "csrc", "api.cpp"), os.path.join(ROOT, "tests", "kv_trace", "kv_trace.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O0", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-o", exe] + src, capture_output=True,
                       text=True)
    assert r.returncode == 0, "the trace program did not build:\n" + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, timeout=60)
    assert r.returncode == 0, "the trace program failed (%d):\n%s" % (r.returncode, r.stderr.decode()[-2000:])
    cases, cur = {}, None
    for line in r.stdout.decode().splitlines():
        if line.startswith("== "):
            cur = cases.setdefault(line[3:], [])
        else:
            cur.append(line)
    return cases, r.stderr.decode()


def _fields(line):
    return dict(t.split("=", 1) for t in line.split()[1:] if "=" in t)


def _ws(v):
    assert v.startswith("ws+0x"), v
    return int(v[5:], 16)


def _keep(v):
    assert v == "kv_keep" or v.startswith("kv_keep+0x"), v
    return int(v[10:], 16) if "+" in v else 0


def test_composite_trace_fill_moves_three_pointers_and_ready_drops_one_gemm(tmp_path):
    from test_api_trace import _toolchain
    if _toolchain() == (None, None):
        pytest.skip("neither a host C++ compiler nor the ROCm headers")
    cases, err = _kv_traces(tmp_path)
    n = 0
    for mode in (0, 1):
        for Lt in (0, 3):
            for form in ("single", "prompts"):
                name = "kv mode%d Lt%d %s " % (mode, Lt, form)
                plain, fill, ready = cases[name + "plain"], cases[name + "fill"], cases[name + "ready"]
                assert plain[-1].startswith("-> rc=0") and plain[-1] == fill[-1] == ready[-1]       # the same workspace bytes
                assert len(fill) == len(plain)
                kv_gemm = [i for i, l in enumerate(plain) if l.startswith("tdc_gemm ") and _fields(l)["W"] == "cross_kv.w"]
                assert len(kv_gemm) == 1
                base = _ws(_fields(plain[kv_gemm[0]])["C"])                                         # the workspace's K/V region
                moved = 0
                for i, (a, b) in enumerate(zip(plain, fill)):
                    fa, fb = _fields(a), _fields(b)
                    if i == kv_gemm[0]:
                        assert fb.pop("C") == "kv_keep" and fa.pop("C")                             # only the GEMM's C ...
                        moved += 1
                    elif a.startswith("tdc_attention ") and fa.get("sk") == "12" and fa.get("sq") == "16":
                        for f in ("k", "v"):                                                        # ... and the cross K / V move,
                            assert _keep(fb.pop(f)) == (_ws(fa.pop(f)) - base)                      # by the same offsets
                        moved += 1
                    assert a.split()[0] == b.split()[0] and fa == fb, (name, i, a, b)
                assert moved == 2, name                     # one stacked GEMM, one cross layer in the tiny model
                # ready: that GEMM is missing and nothing else differs; enc (NULL there) is named by no launch
                assert ready == fill[:kv_gemm[0]] + fill[kv_gemm[0] + 1:], name
                assert sum("=enc" in l for l in fill) == 1 and not any("=enc" in l for l in ready)
                n += 1
    assert n == 8
    for name, lines in cases.items():
        if name.startswith("refused"):
            assert lines[-1].startswith("-> rc=-2 "), name                                          # TDC_E_BADARG
            assert not any(l.startswith(("tdc_gemm", "tdc_attention", "tdc_layernorm")) for l in lines), name
    assert sum(n.startswith("refused") for n in cases) == 7
    assert err.count("kept K/V (kv_keep) runs xattn_mode 0 / 1 only") == 2
