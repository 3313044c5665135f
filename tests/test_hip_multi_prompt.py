"""GPU (-m gpu): several prompts about one video in one compressor pass.  Every comparison is
torch.equal against what the single-prompt calls give: per-item key counts / K, V sources in tdc_attention against one uniform
launch per distinct (sk, source) on the same buffers, the prompt table of tdc_qformer_embed against per-prompt calls, the multi
form of tdc_qformer_fwd (and of the per-kernel sequence) at full width against P single-prompt passes, and
encode_video_prompts against [encode_video(p) for p]."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DTYPES = [torch.float16, torch.bfloat16]


# ------------------------------------------------------------------------------------------------------------- tdc_attention
def _attn_buffers(dtype, batch, slots, heads, sq, sk, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ld = 3 * heads * 64
    q = torch.randn(batch * sq, ld, device="cuda", generator=g).to(dtype)
    kv = torch.randn(slots * sk, ld, device="cuda", generator=g).to(dtype)
    return q, kv, ld


def _attn(q, kv, out, batch, heads, sq, sk, form, q_off=0, kv_off=0, **kw):
    from tdc_video_amd import ops
    D = heads * 64
    ld = q.stride(0)
    return ops.attention(q[q_off * sq:, 0:D], kv[kv_off * sk:, D:2 * D], kv[kv_off * sk:, 2 * D:3 * D], out, batch, heads, 64,
                         sq, sk, 0.125, sq * ld, sk * ld, sk * ld, sq * out.stride(0), form=form, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("sq", [28, 46, 156, 184])
def test_attention_k_len_kv_index_equal_uniform_launches(dtype, form, sq):
    import memcheck
    heads, batch, K = 3, 6, 16
    sk = sq                                                       # the self-attention shape: S = K + Lmax rows
    q, kv, ld = _attn_buffers(dtype, batch, batch, heads, sq, sk, sq)
    D = heads * 64
    k_len = [sk, K + 1, sk - 1, min(sk, 65), K + 1, sk]            # k_len == sk, the smallest case K + 1, a tile boundary + 1
    kv_index = [2, 2, 0, 5, 1, 2]                                 # repeats; slots 3 and 4 are never named
    perm = [3, 1, 4, 0, 5, 2]

    def uniform(b, n, src):
        """item b as a uniform launch of ONE item with sk = n on K / V slot src of the same buffers"""
        o = torch.zeros(sq, D, device="cuda", dtype=dtype)
        from tdc_video_amd import ops
        ops.attention(q[b * sq:(b + 1) * sq, 0:D], kv[src * sk:src * sk + n, D:2 * D], kv[src * sk:src * sk + n, 2 * D:3 * D], o,
                      1, heads, 64, sq, n, 0.125, sq * ld, n * ld, n * ld, sq * D, form=form)
        return o

    for kl, ki in ((k_len, None), (None, kv_index), (k_len, kv_index), (k_len, perm)):
        out, arena = memcheck.guarded((batch * sq, D), dtype, "cuda", 4, 4)
        _attn(q, kv, out, batch, heads, sq, sk, form, k_len=kl, kv_index=ki)
        memcheck.assert_untouched(arena, None, "attention output")
        for b in range(batch):
            want = uniform(b, sk if kl is None else kl[b], b if ki is None else ki[b])
            assert torch.equal(out[b * sq:(b + 1) * sq], want), (kl is not None, ki is not None, b)

    # memory contract: the keys at and beyond k_len[b] and the K / V slots no kv_index names hold 0x00, then 0xFF (NaN)
    ref = torch.zeros(batch * sq, D, device="cuda", dtype=dtype)
    _attn(q, kv, ref, batch, heads, sq, sk, form, k_len=k_len, kv_index=kv_index)
    named_len = {}
    for n, s in zip(k_len, kv_index):
        named_len[s] = max(named_len.get(s, 0), n)
    for byte in memcheck.PATTERNS:
        kvp = kv.clone()
        raw = kvp.view(torch.uint8).view(batch, sk, -1)
        for s in range(batch):
            raw[s, named_len.get(s, 0):] = byte
        out = torch.zeros(batch * sq, D, device="cuda", dtype=dtype)
        _attn(q, kvp, out, batch, heads, sq, sk, form, k_len=k_len, kv_index=kv_index)
        assert torch.isfinite(out.float()).all() and torch.equal(out, ref), hex(byte)


def test_attention_refuses_bias_and_unchecked_indices():
    from tdc_video_amd import ops
    dtype, heads, batch, sq, sk = torch.float16, 2, 2, 32, 32
    q, kv, ld = _attn_buffers(dtype, batch, batch, heads, sq, sk, 1)
    D = heads * 64
    out = torch.zeros(batch * sq, D, device="cuda", dtype=dtype)
    bias = torch.zeros(heads, sq, sk, device="cuda")
    gate = torch.ones(batch * sq, heads, device="cuda")
    for kw in (dict(k_len=[32, 20]), dict(kv_index=[1, 0])):
        with pytest.raises(ValueError):
            _attn(q, kv, out, batch, heads, sq, sk, 0, bias=bias, gate=gate, **kw)
    # the C ABI refuses the combination too (TDC_E_BADARG), whatever the wrapper does
    import ctypes as C
    from tdc_video_amd import lib as L
    d = L.AttnDesc()
    one = torch.ones(batch, device="cuda", dtype=torch.int32)
    d.q, d.k, d.v, d.o = q.data_ptr(), kv.data_ptr(), kv.data_ptr(), out.data_ptr()
    d.q_bs = d.k_bs = d.v_bs = sq * ld
    d.o_bs = sq * D
    d.q_rs, d.k_rs, d.v_rs, d.o_rs = ld, ld, ld, D
    d.batch, d.heads, d.head_dim, d.sq, d.sk, d.scale, d.dtype = batch, heads, 64, sq, sk, 0.125, L.F16
    d.bias, d.bias_hs, d.bias_rs, d.gate, d.gate_rs = bias.data_ptr(), sq * sk, sk, gate.data_ptr(), heads
    d.k_len = one.data_ptr()
    assert L.load().tdc_attention(C.byref(d), ops._stream()) == -2
    d.k_len, d.kv_index = None, one.data_ptr()
    assert L.load().tdc_attention(C.byref(d), ops._stream()) == -2
    # out-of-range entries never reach a launch
    for kw in (dict(k_len=[33, 20]), dict(k_len=[0, 20]), dict(kv_index=[2, 0]), dict(kv_index=[-1, 0])):
        with pytest.raises(ValueError):
            _attn(q, kv, out, batch, heads, sq, sk, 0, **kw)


# --------------------------------------------------------------------------------------------------------- tdc_qformer_embed
@pytest.mark.parametrize("dtype", DTYPES)
def test_qformer_embed_prompt_table_equals_per_prompt_calls(dtype):
    from tdc_video_amd import ops
    g = torch.Generator(device="cuda").manual_seed(2)
    K, D, vocab = 16, 768, 500
    query = torch.randn(5 * K, D, device="cuda", generator=g).to(dtype)
    word = torch.randn(vocab, D, device="cuda", generator=g)
    pos = torch.randn(64, D, device="cuda", generator=g)
    gamma, beta = torch.rand(D, device="cuda", generator=g) + 0.5, torch.randn(D, device="cuda", generator=g)
    prompts = [[101, 7, 102], list(range(20, 32)), [], list(range(100, 131))]
    frame_prompt = [0, 1, 1, 3, 2, 0, 3]
    qsrc = [0, 1, 4, 2, 3, 3, 0]
    F, Lmax = len(frame_prompt), 31
    S = K + Lmax
    qs = torch.tensor(qsrc, dtype=torch.int32, device="cuda")
    outs = []
    for pad_id in (0, -1):                                       # -1: the 0xFF poison of an over-read id
        h32, h16 = ops.qformer_embed(query, qs, word, pos, prompts, gamma, beta, 1e-12, F, K, D, dtype, frame_prompt=frame_prompt,
                                     pad_id=pad_id)
        outs.append((h32, h16))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    h32, h16 = outs[0]
    assert tuple(h32.shape) == (F * S, D)
    for f, p in enumerate(frame_prompt):
        ids = torch.tensor(prompts[p], dtype=torch.int32, device="cuda") if prompts[p] else None
        w32, w16 = ops.qformer_embed(query, qs[f:f + 1], word, pos, ids, gamma, beta, 1e-12, 1, K, D, dtype)
        n = K + len(prompts[p])
        assert torch.equal(h32[f * S:f * S + n], w32) and torch.equal(h16[f * S:f * S + n], w16), f
        assert not h32[f * S + n:(f + 1) * S].any() and not h16[f * S + n:(f + 1) * S].view(torch.int16).any(), f
    # a prompt no frame names: its whole row of the device table is padding, 0x00 then 0xFF (prompt 2 is empty) - no bit changes
    unnamed = [0, 1, 1, 3, 3, 0, 3]
    u = [ops.qformer_embed(query, qs, word, pos, prompts, gamma, beta, 1e-12, F, K, D, dtype, frame_prompt=unnamed, pad_id=pad_id)
         for pad_id in (0, -1)]
    assert torch.equal(u[0][0], u[1][0]) and torch.equal(u[0][1], u[1][1])
    for f, p in enumerate(unnamed):
        if p == frame_prompt[f]:
            assert torch.equal(u[0][0][f * S:(f + 1) * S], h32[f * S:(f + 1) * S]), f
            assert torch.equal(u[0][1][f * S:(f + 1) * S], h16[f * S:(f + 1) * S]), f
    assert torch.equal(u[0][1][4 * S:5 * S], h16[3 * S:4 * S].clone().index_copy_(
        0, torch.arange(K, device="cuda"), u[0][1][4 * S:4 * S + K]))      # frame 4: prompt 3's text rows behind its own query rows
    with pytest.raises(ValueError):
        ops.qformer_embed(query, qs, word, pos, prompts, gamma, beta, 1e-12, F, K, D, dtype, frame_prompt=[0, 1, 1, 4, 2, 0, 3])
    with pytest.raises(ValueError):
        ops.qformer_embed(query, qs, word, pos, [[vocab]] + prompts[1:], gamma, beta, 1e-12, F, K, D, dtype,
                          frame_prompt=frame_prompt)


# ------------------------------------------------------------------------------------------------- the composite, full width
T = 40
PROMPTS = [[101, 2054, 102], [101] + list(range(2000, 2010)) + [102], [101] + list(range(3000, 3010)) + [102],
           [101] + list(range(4000, 4029)) + [102]]               # Lt = 3, 12, 12, 31


def _engine(K):
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd.pipeline import VideoEncoder
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    H = 3584
    sd = bench.random_state_dict(H, K, dev, gen)
    enc = VideoEncoder(sd, bench.model_cfg(H, K, T), dtype=torch.float16, device=dev, tower_dtype=torch.bfloat16,
                       tower_res_dtype=torch.float16)
    del sd
    torch.cuda.empty_cache()
    return enc


@pytest.fixture(scope="module")
def eng144():
    return _engine(144)


@pytest.fixture(scope="module")
def eng16():
    return _engine(16)


def _group(enc, Nf, n_frames=9, seed=0):
    """a synthetic group: P = 4 prompts with overlapping but unequal compressed-frame lists over n_frames frames of Nf rows"""
    from tdc_video_amd import pipeline
    g = torch.Generator(device="cuda").manual_seed(seed + Nf)
    Hp = (enc.c.H + 63) // 64 * 64
    Xf = (torch.randn(n_frames * Nf, Hp, device="cuda", generator=g) * 0.5).to(enc.dtype)
    Xf[:, enc.c.H:] = 0
    frames = [[1, 2, 3, 5], [2, 3, 4], [1, 5, 6, 7, 8], [3]]
    plans = [dict(comp_frames=fr, comp_chunk=[0 if f < 4 else 1 for f in fr], key_frames=[0, 4]) for fr in frames]
    return Xf, plans, pipeline.prompt_maps(plans)


def _check_multi(enc, Nf, prompts, native):
    Xf, plans, m = _group(enc, Nf)
    K = enc.K
    enc.native_qformer = native
    try:
        qt = enc.make_queries(Xf, Nf, Nf, m["key_frames"])
        multi = dict(kv_src=m["kv_src"], frame_prompt=m["frame_prompt"])
        got = enc.compress_frames(Xf, Nf, m["enc_frames"], qt, m["qsrc"], prompts, None, multi)
        assert got.shape[0] == m["offsets"][-1] * K
        for p, pl in enumerate(plans):
            qt1 = enc.make_queries(Xf, Nf, Nf, pl["key_frames"])
            want = enc.compress_frames(Xf, Nf, pl["comp_frames"], qt1, pl["comp_chunk"], prompts[p] or None)
            lo, hi = m["offsets"][p], m["offsets"][p + 1]
            assert torch.equal(got[lo * K:hi * K], want), (Nf, p, native)
        # virtual-frame order permuted -> row blocks permuted, bits unchanged
        F = m["offsets"][-1]
        perm = [(5 * i + 3) % F for i in range(F)]
        assert sorted(perm) == list(range(F))
        multi2 = dict(kv_src=[m["kv_src"][i] for i in perm], frame_prompt=[m["frame_prompt"][i] for i in perm])
        got2 = enc.compress_frames(Xf, Nf, m["enc_frames"], qt, [m["qsrc"][i] for i in perm], prompts, None, multi2)
        for j, i in enumerate(perm):
            assert torch.equal(got2[j * K:(j + 1) * K], got[i * K:(i + 1) * K]), (Nf, j)
        return got
    finally:
        enc.native_qformer = True


@pytest.mark.parametrize("Nf", [156, 84, 206])
def test_qformer_multi_equals_single_prompt_passes_k144(eng144, Nf):
    a = _check_multi(eng144, Nf, PROMPTS, True)
    b = _check_multi(eng144, Nf, PROMPTS, False)                 # composite == per-kernel sequence
    assert torch.equal(a, b)


@pytest.mark.parametrize("Nf", [156, 84, 206])
def test_qformer_multi_equals_single_prompt_passes_k16(eng16, Nf):
    a = _check_multi(eng16, Nf, PROMPTS, True)
    b = _check_multi(eng16, Nf, PROMPTS, False)
    assert torch.equal(a, b)


def test_qformer_multi_without_text_and_xattn_modes(eng16):
    a = _check_multi(eng16, 84, [[], [], [], []], True)           # Lmax = 0
    assert torch.equal(a, _check_multi(eng16, 84, [[], [], [], []], False))
    old = getattr(eng16, "xattn_mode", 1)
    try:
        eng16.xattn_mode = 0
        _check_multi(eng16, 84, PROMPTS, True)
        _check_multi(eng16, 84, PROMPTS, False)
        eng16.xattn_mode = 2                                      # the whole-block kernel: the form is refused, callers fall back
        assert not eng16.multi_prompt_ok(84)
        Xf, plans, m = _group(eng16, 84)
        qt = eng16.make_queries(Xf, 84, 84, m["key_frames"])
        with pytest.raises(ValueError):                           # refused on the host, before any launch
            eng16.compress_frames(Xf, 84, m["enc_frames"], qt, m["qsrc"], PROMPTS, None,
                                  dict(kv_src=m["kv_src"], frame_prompt=m["frame_prompt"]))
    finally:
        eng16.xattn_mode = old


def test_qformer_multi_workspace_contents_do_not_matter(eng16):
    """the composite's workspace 0x00-filled, 0xFF-filled and re-used: the same bits"""
    Xf, plans, m = _group(eng16, 84)
    qt = eng16.make_queries(Xf, 84, 84, m["key_frames"])
    multi = dict(kv_src=m["kv_src"], frame_prompt=m["frame_prompt"])
    ref = eng16.compress_frames(Xf, 84, m["enc_frames"], qt, m["qsrc"], PROMPTS, None, multi).clone()
    ws = eng16._qf_ws
    assert torch.is_tensor(ws) and ws.numel() > 0
    for byte in (0x00, 0xFF, None):
        if byte is not None:
            ws.view(torch.uint8).fill_(byte)
        got = eng16.compress_frames(Xf, 84, m["enc_frames"], qt, m["qsrc"], PROMPTS, None, multi)
        assert eng16._qf_ws is ws                                 # re-used, not re-allocated
        assert torch.isfinite(got.float()).all() and torch.equal(got, ref), byte


@pytest.mark.parametrize("which,lens", [("k16", (3, 60, 30, 3)), ("k144", (10, 50, 10, 50))])
def test_qformer_multi_across_query_tile_classes(which, lens, eng16, eng144):
    """a group's frame stride S = K + Lmax in another 64-row query-tile class of the attention kernel than its members' own
    K + Lt: K = 16 with Lt 3 / 60 (19 rows against 76), K = 144 with Lt 10 / 50 (154 rows against 194, across 192)"""
    enc = eng16 if which == "k16" else eng144
    K = enc.K
    prompts = [[101] + list(range(2000 + 100 * i, 2000 + 100 * i + n - 2)) + [102] for i, n in enumerate(lens)]
    assert len({(K + n - 1) // 64 for n in lens}) > 1
    a = _check_multi(enc, 84, prompts, True)
    assert torch.equal(a, _check_multi(enc, 84, prompts, False))


@pytest.mark.parametrize("native", [True, False])
def test_qformer_multi_outputs_in_sentinel_arenas_inputs_poisoned(eng16, native, monkeypatch):
    """every buffer the multi form allocates (the gathered encoder rows, the embedding's h32 / h16, the K/V and context buffers
    of the per-kernel sequence, the composite's `out`) starts as 0x00 / 0xFF inside a guarded arena: the same bits come out, no
    guard band changes - and, in the per-kernel sequence, the padding text rows of every frame are overwritten with the
    poison before each self-attention launch, so no valid row may read them"""
    import memcheck
    ops = sys.modules[type(eng16).__module__].ops                 # the module object the engine's launches go through
    Xf, plans, m = _group(eng16, 84)
    K = eng16.K
    qt = eng16.make_queries(Xf, 84, 84, m["key_frames"])
    multi = dict(kv_src=m["kv_src"], frame_prompt=m["frame_prompt"])
    eng16.native_qformer = native
    try:
        ref = eng16.compress_frames(Xf, 84, m["enc_frames"], qt, m["qsrc"], PROMPTS, None, multi).clone()
        real = ops.attention
        for byte in memcheck.PATTERNS:
            poisoned, calls = [], []

            def attention(q, k, v, out, batch, heads, hd, sq, sk, *a, **kw):
                kl = kw.get("k_len")
                calls.append(kl is not None)
                if kl is not None:                                # self-attention of the multi form: q, k, v view one buffer
                    for t in (q, k, v):
                        for b, n in enumerate(kl):
                            if n < sk:
                                t[b * sq + n:(b + 1) * sq].fill_(float("nan") if byte else 0.0)
                                poisoned.append(b)
                return real(q, k, v, out, batch, heads, hd, sq, sk, *a, **kw)
            with monkeypatch.context() as mp:
                mp.setattr(ops, "attention", attention)
                arenas = memcheck.poison_empty(mp, byte, guard_bytes=4096)
                got = eng16.compress_frames(Xf, 84, m["enc_frames"], qt, m["qsrc"], PROMPTS, None, multi)
                torch.cuda.synchronize()
            assert arenas
            assert native or (calls and any(calls)), calls        # the per-kernel sequence went through the wrapper
            assert native or poisoned                             # ... and its padding rows were poisoned
            for a in arenas:
                memcheck.assert_untouched(a, None, "multi-prompt Q-Former buffer")
            assert torch.isfinite(got[:, :eng16.c.H].float()).all() and torch.equal(got, ref), (hex(byte), native)
    finally:
        eng16.native_qformer = True


def test_index_arrays_are_checked_on_the_host(eng16):
    Xf, plans, m = _group(eng16, 84)
    qt = eng16.make_queries(Xf, 84, 84, m["key_frames"])
    U, F = len(m["enc_frames"]), m["offsets"][-1]
    for native in (True, False):
        eng16.native_qformer = native
        try:
            for bad in (dict(kv_src=[U] + m["kv_src"][1:], frame_prompt=m["frame_prompt"]),
                        dict(kv_src=m["kv_src"], frame_prompt=[4] + m["frame_prompt"][1:]),
                        dict(kv_src=[-1] + m["kv_src"][1:], frame_prompt=m["frame_prompt"])):
                with pytest.raises(ValueError):
                    eng16.compress_frames(Xf, 84, m["enc_frames"], qt, m["qsrc"], PROMPTS, None, bad)
        finally:
            eng16.native_qformer = True


# ------------------------------------------------------------------------------------------------------- encode_video_prompts
def _video():
    import bench
    dev = torch.device("cuda", 0)
    vs = bench.synth_video(0, T, 384, dev, torch.float16, scene_len=5)
    vd = bench.synth_video(0, T, 378, dev, torch.float16, seed=4321, scene_len=5)
    return vs, vd


def _qs(btl_long=None):
    qs = [dict(budget_text_len=64, n_text_tokens=64 + 3 * i, prompt_ids=p) for i, p in enumerate(PROMPTS)]
    qs.append(dict(budget_text_len=64, n_text_tokens=90, prompt_ids=PROMPTS[1]))
    if btl_long is not None:
        qs.insert(2, dict(budget_text_len=btl_long, n_text_tokens=btl_long, prompt_ids=PROMPTS[2]))
    return qs


def _strip(info):
    return {k: v for k, v in info.items() if k not in ("prompts", "cache")}


@pytest.mark.parametrize("which", ["k16", "k144"])
def test_encode_video_prompts_equals_per_prompt_encode_video(which, eng16, eng144):
    enc = eng16 if which == "k16" else eng144
    vs, vd = _video()
    from tdc_video_amd import pipeline
    # a budget_text_len long enough to change the a1 selection, if the config has one below T frames
    btl_long = None
    for cand in (2000, 8000, 20000):
        if len(pipeline.frame_indices(enc.cfg, T, cand, 224)) < T:
            btl_long = cand
            break
    qs = _qs(btl_long)
    want, winfo = [], []
    for q in qs:
        info = {}
        want.append(enc.encode_video(vs, vd, (384, 384), q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"], info=info))
        winfo.append(info)
    for max_prompts, pad in ((8, 1.0), (2, 1.0), (8, 0.25), (8, 0.0)):           # P above max_prompts; the padding limits
        infos = [{} for _ in qs]
        got = enc.encode_video_prompts(vs, vd, (384, 384), qs, infos=infos, max_prompts=max_prompts, pad_fraction=pad)
        for p in range(len(qs)):
            assert torch.equal(got[p], want[p]), (max_prompts, pad, p)
            assert _strip(infos[p]) == _strip(winfo[p]), (max_prompts, pad, p)
        sizes = [i["prompts"]["group_size"] for i in infos]
        assert max(sizes) <= max_prompts
        if pad == 1.0 and max_prompts == 8:
            assert max(sizes) >= 4
        if btl_long is not None:
            assert infos[2]["prompts"]["group"] not in {infos[p]["prompts"]["group"] for p in range(len(qs)) if p != 2}
    # a cold, then a warm frame cache
    cache = enc.new_cache(2 << 30)
    for warm in (False, True):
        infos = [{} for _ in qs]
        got = enc.encode_video_prompts(vs, vd, (384, 384), qs, infos=infos, cache=cache)
        for p in range(len(qs)):
            assert torch.equal(got[p], want[p]), (warm, p)
        if warm:
            assert all(i["cache"]["frames_encoded"] == 0 for i in infos)
    # the whole-block cross-attention kernel: one pass per prompt, the same results
    old = getattr(enc, "xattn_mode", 1)
    try:
        for mode in (0, 2):
            enc.xattn_mode = mode
            w = [enc.encode_video(vs, vd, (384, 384), q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"]) for q in qs[:3]]
            g = enc.encode_video_prompts(vs, vd, (384, 384), qs[:3], max_prompts=8, pad_fraction=1.0)
            for a, b in zip(g, w):
                assert torch.equal(a, b), mode
    finally:
        enc.xattn_mode = old
