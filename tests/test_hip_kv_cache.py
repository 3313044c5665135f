"""GPU (-m gpu): kept cross-attention K/V.  Every comparison is torch.equal: rows of tdc_gemm are
independent and a fill is the plain pass's launch on the same operands with another C pointer, so plain, fill and every later
ready pass give the same bits - at the C ABI (the composite tdc_qformer_fwd, full Q-Former width), in the per-kernel sequence,
through encode_video / encode_video_prompts with a FrameCache that has a K/V budget (the reduced fixtures), and through the
mixin's config key."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

PROMPTS = [[101, 2054, 102], [101] + list(range(2000, 2010)) + [102], [101] + list(range(4000, 4029)) + [102]]   # Lt 3, 12, 31
NF = 84                          # rows per frame of the synthetic group: a shape the whole-block kernel supports


# ------------------------------------------------------------------------------------- the composite and the per-kernel sequence
@pytest.fixture(scope="module")
def eng16():
    from test_hip_multi_prompt import _engine
    return _engine(16)


def _group(enc):
    """9 frames of NF rows; single form: 5 compressed frames; multi form: P = 3 prompts over U = 6 distinct frames"""
    from tdc_video_amd import pipeline
    g = torch.Generator(device="cuda").manual_seed(17)
    Hp = (enc.c.H + 63) // 64 * 64
    Xf = (torch.randn(9 * NF, Hp, device="cuda", generator=g) * 0.5).to(enc.dtype)
    Xf[:, enc.c.H:] = 0
    frames = [[1, 2, 3, 5, 7], [2, 3, 4], [1, 5, 8]]
    plans = [dict(comp_frames=fr, comp_chunk=[0 if f < 4 else 1 for f in fr], key_frames=[0, 4]) for fr in frames]
    return Xf, plans, pipeline.prompt_maps(plans)


def _forms(enc):
    """-> Xf, {form: (frame_rows, qtable, qsrc, prompt_ids, multi)}"""
    Xf, plans, m = _group(enc)
    qt = enc.make_queries(Xf, NF, NF, [0, 4])
    return Xf, dict(single=(plans[0]["comp_frames"], qt, plans[0]["comp_chunk"], PROMPTS[1], None),
                    multi=(m["enc_frames"], qt, m["qsrc"], PROMPTS, dict(kv_src=m["kv_src"], frame_prompt=m["frame_prompt"])))


def _rows(Xf, frames):
    return torch.cat([Xf[f * NF:(f + 1) * NF] for f in frames]).contiguous()


def _pass(enc, native, rows, F, qt, qsrc, prompt_ids, multi, kv):
    """one pass behind compress_frames' row gather: `rows` is the enc operand itself (None: a NULL pointer)"""
    qs = torch.tensor(qsrc, dtype=torch.int32, device="cuda")
    if native:
        return enc._compress_native(rows, F, NF, qt, qs, prompt_ids, multi, kv)
    return enc.qformer(rows, F, NF, qt, qs, prompt_ids, multi, kv)[0]


@pytest.mark.parametrize("form", ["single", "multi"])
@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("mode", [1, 0])
def test_plain_fill_ready_same_bits_and_memory_contract(eng16, native, form, mode):
    import memcheck
    from tdc_video_amd.cache import KeptKV
    enc = eng16
    Xf, forms = _forms(enc)
    frames, qt, qsrc, pids, multi = forms[form]
    U, F = len(frames), len(qsrc)
    n = enc.c.qformer.cross_kv.w.shape[0]
    assert enc.kv_entry_bytes(U, NF) == U * NF * n * 2 and tuple(enc.kv_alloc(U, NF).shape) == (U * NF, n)
    old = enc.native_qformer, enc.xattn_mode
    enc.native_qformer, enc.xattn_mode = native, mode
    try:
        assert enc.kv_cache_ok(NF)
        plain = enc.compress_frames(Xf, NF, frames, qt, qsrc, pids, None, multi).clone()
        # engine level: fill, then ready over an Xf that holds NaN everywhere - compress_frames reads no row of it
        kv = KeptKV(enc.kv_alloc(U, NF), False)
        assert torch.equal(enc.compress_frames(Xf, NF, frames, qt, qsrc, pids, None, multi, kv=kv), plain)
        kv.ready = True
        bad = torch.full_like(Xf, float("nan"))
        assert torch.equal(enc.compress_frames(bad, NF, frames, qt, qsrc, pids, None, multi, kv=kv), plain)
        # behind the gather: the kept buffer inside a guarded arena
        mm = None if multi is None else dict(multi, enc_frames=U)
        rows = _rows(Xf, frames)
        want = _pass(enc, native, rows, F, qt, qsrc, pids, mm, None).clone()
        view, arena = memcheck.guarded((U * NF, n), enc.dtype, "cuda", 4, 4)
        got = _pass(enc, native, rows, F, qt, qsrc, pids, mm, KeptKV(view, False))
        torch.cuda.synchronize()
        memcheck.assert_untouched(arena, None, "kv_keep on a fill")       # rows 0 .. U*Nenc, columns 0 .. cross_kv.n, no more
        assert memcheck.same_bits(got, want)
        assert torch.equal(view, kv.buf)                                  # the rows the engine-level fill projected
        before = arena.buf.clone()
        # ready: enc as a poisoned arena (no declared read set: every byte 0x00, then 0xFF) and as NULL
        for byte in memcheck.PATTERNS:
            poison, _ = memcheck.poisoned(rows[:0], 4, 4, total_rows=U * NF, fill=byte)
            got = _pass(enc, native, poison, F, qt, qsrc, pids, mm, KeptKV(view, True))
            assert memcheck.same_bits(got, want), hex(byte)
        got = _pass(enc, native, None, F, qt, qsrc, pids, mm, KeptKV(view, True))
        torch.cuda.synchronize()
        assert memcheck.same_bits(got, want)
        assert torch.equal(arena.buf, before), "a ready pass changed a byte of kv_keep"
    finally:
        enc.native_qformer, enc.xattn_mode = old


def test_whole_block_kernel_refuses_kept_kv(eng16):
    from tdc_video_amd import lib as L
    from tdc_video_amd.cache import KeptKV
    enc = eng16
    Xf, forms = _forms(enc)
    frames, qt, qsrc, pids, _ = forms["single"]
    U = len(frames)
    old = enc.xattn_mode
    try:
        enc.xattn_mode = 2
        assert not enc.kv_cache_ok(NF) and enc.kv_cache_ok(NF + 1)        # where the kernel's shape support holds
        buf = enc.kv_alloc(U, NF)
        for ready in (False, True):
            with pytest.raises(ValueError):                               # the engine refuses on the host, before any launch
                enc.compress_frames(Xf, NF, frames, qt, qsrc, pids, None, None, kv=KeptKV(buf, ready))
            with pytest.raises(L.TdcHipError, match="-2"):                # and the C ABI with TDC_E_BADARG
                _pass(enc, True, _rows(Xf, frames), U, qt, qsrc, pids, None, KeptKV(buf, ready))
        enc.xattn_mode = 1
        for state in (2, -1):                                             # any other kv_state
            m = enc._qformer_struct()[0]                                  # the engine only passes 0 / 1: go below it
            import ctypes as C
            mk = L.QformerModel()
            C.pointer(mk)[0] = m
            mk.kv_keep, mk.kv_state = buf.data_ptr(), state
            assert L.load().tdc_qformer_workspace_bytes(C.byref(mk), U, enc.K, 0, NF) == \
                L.load().tdc_qformer_workspace_bytes(C.byref(m), U, enc.K, 0, NF)                   # the layout does not change
            ws = torch.empty(L.load().tdc_qformer_workspace_bytes(C.byref(mk), U, enc.K, 0, NF), dtype=torch.uint8, device="cuda")
            out = torch.empty(U * enc.K, (enc.c.H + 63) // 64 * 64, device="cuda", dtype=enc.dtype)
            qs = torch.tensor(qsrc, dtype=torch.int32, device="cuda")
            rows = _rows(Xf, frames)
            from tdc_video_amd import ops
            rc = L.load().tdc_qformer_fwd(C.byref(mk), ops._ptr(rows), rows.stride(0), U, NF, ops._ptr(qt), qt.stride(0),
                                          ops._ptr(qs), C.c_void_p(0), 0, enc.K, ops._ptr(out), out.stride(0), ops._ptr(ws),
                                          ws.numel(), ops._stream())
            assert rc == -2, state
    finally:
        enc.xattn_mode = old


def test_engine_reports_unsupported_under_the_whole_block_kernel(eng16):
    from test_hip_multi_prompt import _video
    enc = eng16
    vs, vd = _video()
    old = enc.xattn_mode
    try:
        enc.xattn_mode = 2
        ref, info = {}, {}
        want = enc.encode_video(vs, vd, (384, 384), 64, 64, PROMPTS[1], info=ref)
        c = enc.new_cache(2 << 30, kv_bytes=1 << 30)
        got = enc.encode_video(vs, vd, (384, 384), 64, 64, PROMPTS[1], info=info, cache=c)
        assert torch.equal(got, want)
        assert not enc.kv_cache_ok(c.rows_per_frame), "the fixture's frames must be a shape the whole-block kernel supports"
        assert info["cache"]["kv"]["state"] == "unsupported" and c.kv_stats()["entries"] == 0
        assert {k: v for k, v in info.items() if k != "cache"} == ref
    finally:
        enc.xattn_mode = old


# ------------------------------------------------------------------------------------------- the engine, on the reduced fixtures
def _fixture(name):
    import synth
    from tdc_video_amd.pipeline import VideoEncoder
    from util import load_fixture, pipeline_cfg
    W, o = load_fixture(name)
    enc = VideoEncoder(W, pipeline_cfg(o), dtype=torch.float16, device="cuda", siglip_heads=4, dino_heads=4, qformer_heads=4)
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"])).cuda()
    ids = torch.from_numpy(o["input_ids"])[0]
    return enc, vid, (vid + 0.01), tuple(int(v) for v in o["image_size"]), len(ids), [int(i) for i in o["prompt_ids"]], o


@pytest.fixture(scope="module")
def t40():
    return _fixture("pipeline_T40.npz")


def _run(fx, prompt=None, cache=None, info=None, cap=224, audio=None, vid=None):
    enc, vs, vd, size, n_ids, pid, _ = fx
    prompt = pid if prompt is None else prompt
    if vid is not None:
        vs, vd = vid
    return enc.encode_video(vs, vd, size, budget_text_len=n_ids, n_text_tokens=n_ids - 1 + len(prompt) - len(pid),
                            prompt_ids=prompt, audio=audio, frame_cap=cap, info=info, cache=cache)


def _strip(info):
    return {k: v for k, v in info.items() if k != "cache"}


def test_filled_then_hit_equal_fresh_and_kv_off(t40):
    enc, pid = t40[0], t40[5]
    short = pid[:4] + pid[-1:]                                            # a second prompt of another length
    ref_a, ref_b = {}, {}
    want_a, want_b = _run(t40, info=ref_a), _run(t40, short, info=ref_b)
    off, on = enc.new_cache(1 << 30), enc.new_cache(1 << 30, kv_bytes=1 << 28)
    for cache in (off, on):
        ia, ib = {}, {}
        assert torch.equal(_run(t40, cache=cache, info=ia), want_a)
        assert torch.equal(_run(t40, short, cache=cache, info=ib), want_b)
        assert _strip(ia) == ref_a and _strip(ib) == ref_b
        if cache is off:
            assert "kv" not in ia["cache"] and "kv" not in ib["cache"]
            off_info = ia, ib
    assert ia["cache"]["kv"]["state"] == "filled" and ib["cache"]["kv"]["state"] == "hit"
    U = ia["cache"]["kv"]["frames"]
    assert U == 15 and ia["cache"]["kv"]["bytes"] == enc.kv_entry_bytes(U, on.rows_per_frame) == ib["cache"]["kv"]["bytes"]
    for a, b in zip(off_info, (ia, ib)):                                  # every info["cache"] key of today, unchanged
        assert {k: v for k, v in b["cache"].items() if k != "kv"} == a["cache"]
    assert off.stats() == on.stats() and off.bytes == on.bytes
    assert on.kv_stats()["fills"] == 1 and on.kv_stats()["hits"] == 1 and on.kv_stats()["bytes"] == ia["cache"]["kv"]["bytes"]
    assert off.kv_stats()["entries"] == 0 and off.kv_stats()["misses"] == 0
    on.clear()
    assert on.kv_stats()["entries"] == 0 and on.kv_stats()["bytes"] == 0


@pytest.mark.parametrize("native", [True, False])
def test_hit_runs_one_gemm_and_one_gather_fewer(t40, native, monkeypatch):
    enc, pid = t40[0], t40[5]
    ops = sys.modules[type(enc).__module__].ops
    short = pid[:4] + pid[-1:]
    off, on = enc.new_cache(1 << 30), enc.new_cache(1 << 30, kv_bytes=1 << 28)
    old = enc.native_qformer
    enc.native_qformer = native
    try:
        want = _run(t40, short)
        for cache in (off, on):
            _run(t40, cache=cache)                                        # warm: the frames, and the K/V entry
        real, counts = ops.gather_rows, {}

        def gather_rows(*a, **kw):
            counts["gather"] = counts.get("gather", 0) + 1
            return real(*a, **kw)
        monkeypatch.setattr(ops, "gather_rows", gather_rows)
        n = {}
        for name, cache in (("off", off), ("hit", on)):
            counts.clear()
            info = {}
            ops.profile_start()
            try:
                got = _run(t40, short, cache=cache, info=info)
                torch.cuda.synchronize()
            finally:
                recs = ops.profile_stop()
            assert torch.equal(got, want)
            n[name] = (sum(r["kind"] == "gemm" for r in recs), counts["gather"], len(recs))
        assert info["cache"]["kv"]["state"] == "hit"
        assert n["hit"][0] == n["off"][0] - 1 and n["hit"][1] == n["off"][1] - 1, n
        assert n["hit"][2] == n["off"][2] - 1, n                          # no other profiled launch appears or leaves
    finally:
        enc.native_qformer = old


def test_another_frame_cap_is_an_entry_of_its_own(t40):
    enc = t40[0]
    c = enc.new_cache(1 << 30, kv_bytes=1 << 28)
    i1, i2, i3 = {}, {}, {}
    _run(t40, cache=c, info=i1)
    assert torch.equal(_run(t40, cache=c, info=i2, cap=30), _run(t40, cap=30))
    assert len(i2["frame_indices"]) == 30 and i2["cache"]["kv"]["state"] == "filled" and c.kv_stats()["entries"] == 2
    assert torch.equal(_run(t40, cache=c, info=i3, cap=30), _run(t40, cap=30))
    assert i3["cache"]["kv"]["state"] == "hit" and c.kv_stats()["entries"] == 2


def test_budget_of_one_entry_and_below_one(t40):
    enc, vs, vd = t40[0], t40[1], t40[2]
    probe, info = enc.new_cache(1 << 30, kv_bytes=1 << 28), {}
    _run(t40, cache=probe, info=info)
    nb = info["cache"]["kv"]["bytes"]
    other = (vs.flip(0).contiguous() * 0.5, vd.flip(0).contiguous() * 0.5)
    c = enc.new_cache(1 << 30, kv_bytes=nb + nb // 2)                     # one entry fits, two do not
    states = []
    for vid in (None, other, None, None):
        info = {}
        assert torch.equal(_run(t40, cache=c, info=info, vid=vid), _run(t40, vid=vid))
        states.append(info["cache"]["kv"]["state"])
        assert c.kv_stats()["bytes"] <= c.kv_max_bytes and c.kv_stats()["entries"] == 1
    assert states == ["filled", "filled", "filled", "hit"] and c.kv_stats()["evictions"] == 2
    c = enc.new_cache(1 << 30, kv_bytes=nb - 1)                           # below one entry: the call runs as today
    for _ in range(2):
        info = {}
        assert torch.equal(_run(t40, cache=c, info=info), _run(t40))
        assert info["cache"]["kv"] == dict(state="bypassed", frames=15, bytes=nb)
    assert c.kv_stats()["entries"] == 0 and c.kv_stats()["bytes"] == 0


def test_audio_same_hits_changed_misses():
    import synth
    fx = _fixture("pipeline_T40_audio.npz")
    enc, o = fx[0], fx[6]
    wins = synth.beats_windows(torch.from_numpy(o["audio_wav"].astype(np.float32)))
    scale = (lambda w, s: [x * s for x in w] if isinstance(w, (list, tuple)) else w * s)
    same, changed = {"beats_windows": scale(wins, 1.0)}, {"beats_windows": scale(wins, 0.5)}
    want, want_changed = _run(fx, audio={"beats_windows": wins}), _run(fx, audio=changed)
    assert not torch.equal(want, want_changed)
    c = enc.new_cache(1 << 30, kv_bytes=1 << 28)
    states = []
    for audio, w in (({"beats_windows": wins}, want), (same, want), (changed, want_changed), (None, _run(fx))):
        info = {}
        assert torch.equal(_run(fx, audio=audio, cache=c, info=info), w)
        states.append(info["cache"]["kv"]["state"])
    assert states == ["filled", "hit", "filled", "filled"] and c.kv_stats()["entries"] == 3


def test_encode_video_prompts_fills_once_and_later_calls_hit(t40):
    enc, vs, vd, size, n_ids, pid, _ = t40
    mk = lambda p: dict(budget_text_len=n_ids, n_text_tokens=n_ids - 1 + len(p) - len(pid), prompt_ids=p)
    first = [mk(pid), mk(pid[:4] + pid[-1:]), mk(pid[:2] + pid[-1:]), mk(pid)]
    later = [mk(pid[:3] + pid[-1:]), mk(pid[:5] + pid[-1:])]
    c = enc.new_cache(1 << 30, kv_bytes=1 << 28)
    for qs, states in ((first, {"filled", "hit"}), (later, {"hit"})):
        want, winfo = [], []
        for q in qs:
            info = {}
            want.append(enc.encode_video(vs, vd, size, q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"], info=info))
            winfo.append(info)
        infos = [{} for _ in qs]
        got = enc.encode_video_prompts(vs, vd, size, qs, infos=infos, cache=c, max_prompts=2, pad_fraction=1.0)
        for p in range(len(qs)):
            assert torch.equal(got[p], want[p]), p
            assert {k: v for k, v in infos[p].items() if k not in ("cache", "prompts")} == winfo[p]
        assert {i["cache"]["kv"]["state"] for i in infos} == states
        assert infos[0]["cache"]["kv"]["state"] == ("filled" if qs is first else "hit")
    assert c.kv_stats()["fills"] == 1 and c.kv_stats()["entries"] == 1   # the groups of both calls share the one entry


# ---------------------------------------------------------------------------------------------------------- boundary (model.py)
def test_boundary_kv_config_key():
    import synth
    from test_hip_boundary import loaded_lm
    from test_hip_video_cache import _boundary_call, _same
    from util import load_fixture
    W, o = load_fixture("pipeline_T40.npz")
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    ids = torch.from_numpy(o["input_ids"])
    text = [j for j in range(ids.shape[1]) if int(ids[0, j]) != -200]
    ids2 = ids[:, [j for j in range(ids.shape[1]) if j not in text[-3:-1]]]          # a shorter question
    pid = [int(i) for i in o["prompt_ids"]]
    calls = ((ids, pid), (ids2, pid[:4] + pid[-1:]), (ids, pid))
    off = loaded_lm(W, o, tdc_video_cache_bytes=1 << 30)
    want = [_boundary_call(off, i, vid, o, p) for i, p in calls]
    on = loaded_lm(W, o, tdc_video_cache_bytes=1 << 30, tdc_kv_cache_bytes=1 << 28)
    for (i, p), w in zip(calls, want):
        _same(_boundary_call(on, i, vid, o, p), w)
    st = on.get_model().tdc_video_cache().kv_stats()
    assert st["fills"] >= 1 and st["hits"] >= 1 and st["max_bytes"] == 1 << 28
    assert on.get_model().tdc_video_cache().stats() == off.get_model().tdc_video_cache().stats()
    assert off.get_model().tdc_video_cache().kv_stats()["max_bytes"] == 0
    on.get_model().tdc_video_cache_clear()
    assert on.get_model().tdc_video_cache().kv_stats()["entries"] == 0
    with pytest.raises(ValueError, match="tdc_kv_cache_bytes"):
        _boundary_call(loaded_lm(W, o, tdc_video_cache_bytes=1 << 30, tdc_kv_cache_bytes=-5), ids, vid, o, pid)
    with pytest.raises(ValueError, match="tdc_video_cache_bytes"):
        _boundary_call(loaded_lm(W, o, tdc_kv_cache_bytes=1 << 28), ids, vid, o, pid)
