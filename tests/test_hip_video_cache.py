"""GPU (-m gpu): the content-keyed frame cache end to end.  Every comparison is torch.equal against a fresh, uncached encode of
the same inputs: the cache reuses rows that frames produce independently of each other (a3-a10), so a cached encode must be
bit for bit the uncached one.  Full architecture (SigLIP-so400m + DINOv2-giant, H = 3584, K = 144) at T = 48, in the bench's
types (fp16 connector / Q-Former, bf16 towers, fp16 residual stream: the selection refinement is on)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 48
PROMPT_A = [101] + list(range(2000, 2010)) + [102]
PROMPT_B = [101, 3000, 3001, 3002, 102]


@pytest.fixture(scope="module")
def full():
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd.pipeline import VideoEncoder
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    H, K = 3584, 144
    sd = bench.random_state_dict(H, K, dev, gen)
    enc = VideoEncoder(sd, bench.model_cfg(H, K, T), dtype=torch.float16, device=dev, tower_dtype=torch.bfloat16,
                       tower_res_dtype=torch.float16)
    del sd
    torch.cuda.empty_cache()
    vs = bench.synth_video(0, T, 384, dev, torch.float16, scene_len=5)
    vd = bench.synth_video(0, T, 378, dev, torch.float16, seed=4321, scene_len=5)
    return enc, vs, vd


def run(enc, vs, vd, prompt=PROMPT_A, n_text=64, btl=64, **kw):
    return enc.encode_video(vs, vd, (384, 384), budget_text_len=btl, n_text_tokens=n_text, prompt_ids=prompt, **kw)


def _fp_host(x, rows, row_bytes=None, row_stride=None):
    from tdc_video_amd.cache import fingerprint_rows_host
    b = x.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy()
    row_stride = x[0].numel() * x.element_size() if row_stride is None else row_stride
    row_bytes = row_stride if row_bytes is None else row_bytes
    return fingerprint_rows_host(np.stack([b[r * row_stride:r * row_stride + row_bytes] for r in rows]))


def _fp_dev(x, rows, row_bytes=None, row_stride=None):
    from tdc_video_amd import ops
    return ops.fingerprint_rows(x, rows, row_bytes, row_stride).cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("px", [384, 378])
def test_fingerprint_kernel_equals_host_frames(dtype, px):
    import tdc_video_amd  # noqa: F401
    g = torch.Generator(device="cuda").manual_seed(px)
    x = torch.randn(6, 3, px, px, device="cuda", generator=g).to(dtype)
    rows = [0, 2, 3, 5]                                        # an index list with gaps
    assert np.array_equal(_fp_dev(x, rows), _fp_host(x, rows))


def test_fingerprint_kernel_waveform_slices_and_odd_lengths():
    import tdc_video_amd  # noqa: F401
    g = torch.Generator(device="cuda").manual_seed(3)
    wav = torch.randn(1, 16000 * 35 + 123, device="cuda", generator=g)
    n = 16000 * 10 * 4
    assert np.array_equal(_fp_dev(wav, [0, 1, 2], n, n), _fp_host(wav, [0, 1, 2], n, n))
    tail = (wav.shape[1] - 16000 * 30) * 4                    # the short last window, at a 16-byte-aligned offset
    assert np.array_equal(_fp_dev(wav, [1], tail, 3 * n), _fp_host(wav, [1], tail, 3 * n))
    b = torch.randint(0, 256, (40000,), device="cuda", generator=g, dtype=torch.uint8)
    for row_bytes, stride in ((1001, 1003), (17, 17), (2048, 2052), (9, 4), (4099, 4104)):   # unaligned starts, tails
        rows = [0, 1, 5, 7]
        assert np.array_equal(_fp_dev(b, rows, row_bytes, stride), _fp_host(b, rows, row_bytes, stride)), (row_bytes, stride)


def test_fingerprint_kernel_single_bit_variants():
    import tdc_video_amd  # noqa: F401
    r = np.random.default_rng(0).integers(0, 256, 2048, dtype=np.uint8)
    flips = np.repeat(r[None], 16384, 0)
    bit = np.arange(16384)
    flips[bit, bit // 8] ^= (1 << (bit % 8)).astype(np.uint8)
    x = torch.from_numpy(np.concatenate([r[None], flips], 0)).cuda()
    rows = list(range(x.shape[0]))
    got = _fp_dev(x, rows)
    assert len({(int(a), int(b)) for a, b in got}) == 16385
    assert np.array_equal(got, _fp_host(x, rows))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_pair_cossim_equals_frame_cossim(dtype):
    from tdc_video_amd import ops
    g = torch.Generator(device="cuda").manual_seed(9)
    slab = torch.randn(6, 576, 1536, device="cuda", generator=g).to(dtype)
    slab[4] = slab[1] + 0.01 * slab[4]                         # a near-duplicate pair too
    pairs = [(0, 3), (3, 5), (5, 1), (1, 4), (2, 2)]
    got = ops.pair_cossim(slab, pairs, 576 * 1536)
    for j, (a, b) in enumerate(pairs):
        want = ops.frame_cossim(torch.cat([slab[a], slab[b]], 0).contiguous(), 2, 576 * 1536)
        assert torch.equal(got[j:j + 1], want), (a, b)
    # in a longer contiguous run, every adjacent pair
    seq = [0, 3, 5, 1, 4]
    want = ops.frame_cossim(torch.cat([slab[s] for s in seq], 0).contiguous(), len(seq), 576 * 1536)
    assert torch.equal(ops.pair_cossim(slab, list(zip(seq[:-1], seq[1:])), 576 * 1536), want)


def test_connector_rows_of_a_subset_equal_the_whole_video(full):
    enc, vs, vd = full
    sig, dino = enc.tower("siglip", vs), enc.tower("dino", vd)
    X, _ = enc.connector(sig, dino, T, [(384, 384)] * T)
    N = X.shape[0] // T
    sub = [1, 2, 7, 30, 47]
    P = sig.shape[0] // T
    rows = torch.cat([torch.arange(f * P, (f + 1) * P, device=sig.device) for f in sub])
    Xs, _ = enc.connector(sig[rows].contiguous(), dino[rows].contiguous(), len(sub), [(384, 384)] * len(sub))
    for j, f in enumerate(sub):
        assert torch.equal(Xs[j * N:(j + 1) * N], X[f * N:(f + 1) * N]), f


# ------------------------------------------------------------------------------------------------ cached encode
def test_two_prompts_one_video(full):
    from tdc_video_amd import ops
    enc, vs, vd = full
    want_a, want_b = run(enc, vs, vd), run(enc, vs, vd, prompt=PROMPT_B, n_text=40)
    c = enc.new_cache(4 << 30)
    i1, i2 = {}, {}
    assert torch.equal(run(enc, vs, vd, cache=c, info=i1), want_a)
    assert i1["cache"]["frames_encoded"] == T
    ops.profile_start()
    try:
        got_b = run(enc, vs, vd, prompt=PROMPT_B, n_text=40, cache=c, info=i2)
        torch.cuda.synchronize()
    finally:
        recs = ops.profile_stop()
    assert torch.equal(got_b, want_b)
    assert i2["cache"]["frames_encoded"] == 0 and i2["cache"]["frames_hit"] == T and i2["cache"]["pairs_computed"] == 0
    assert not [r for r in recs if r["kind"] == "gemm" and r["K"] in (1152, 1536)], "a tower or the connector ran"
    assert c.bytes <= c.max_bytes


def test_partial_hits_and_lvcot(full):
    enc, vs, vd = full
    cfg = enc.cfg
    tpf = (144 + cfg["context_token_num"] * 7) // 8
    old = cfg["tokenizer_model_max_length"]
    cfg["tokenizer_model_max_length"] = 16 + 20 + tpf * 40          # budget_text_len 20 -> 40 frames, 116 -> 37
    try:
        c = enc.new_cache(4 << 30)
        for btl, prompt in ((20, PROMPT_A), (20 + 3 * tpf, PROMPT_B)):
            info, ref = {}, {}
            want = run(enc, vs, vd, prompt=prompt, btl=btl, n_text=btl, info=ref)
            assert torch.equal(run(enc, vs, vd, prompt=prompt, btl=btl, n_text=btl, cache=c, info=info), want)
            assert info["seg_indices"] == ref["seg_indices"]
        assert len(ref["frame_indices"]) == 37 and 0 < info["cache"]["frames_encoded"] < 37
    finally:
        cfg["tokenizer_model_max_length"] = old
    # LVCoT: each half, then the whole video
    c = enc.new_cache(4 << 30)
    h = T // 2
    for lo, hi in ((0, h), (h, T), (0, T)):
        info = {}
        got = run(enc, vs[lo:hi], vd[lo:hi], cache=c, info=info)
        assert torch.equal(got, run(enc, vs[lo:hi], vd[lo:hi]))
    assert info["cache"]["frames_encoded"] == 0


def test_redecoded_copy_hits_and_one_pixel_reencodes_one_frame(full):
    enc, vs, vd = full
    c = enc.new_cache(4 << 30)
    run(enc, vs, vd, cache=c)
    info = {}
    vs2, vd2 = vs.clone(), vd.clone()
    assert torch.equal(run(enc, vs2, vd2, cache=c, info=info), run(enc, vs, vd))
    assert info["cache"]["frames_encoded"] == 0
    vd2[17, 1, 200, 100] += 0.25
    info = {}
    assert torch.equal(run(enc, vs2, vd2, cache=c, info=info), run(enc, vs2, vd2))
    assert info["cache"]["frames_encoded"] == 1 and info["cache"]["pairs_computed"] >= 2


def test_eviction_a_b_a(full):
    enc, vs, vd = full
    c = enc.new_cache(4 << 30)
    run(enc, vs, vd, cache=c)
    budget = int(1.5 * T * c.frame_bytes * c.AUDIO_SHARE / (c.AUDIO_SHARE - 1))     # 1.5 videos of frames
    c = enc.new_cache(budget)
    vs_b, vd_b = vs.flip(0).contiguous() * 0.5, vd.flip(0).contiguous() * 0.5
    for a, b in ((vs, vd), (vs_b, vd_b), (vs, vd)):
        info = {}
        assert torch.equal(run(enc, a, b, cache=c, info=info), run(enc, a, b))
        assert c.bytes <= c.max_bytes and c.reserved_bytes <= c.max_bytes and not info["cache"]["bypassed"]
    assert c.stats()["evictions"] > 0


def test_near_tied_video_refinement(full):
    from test_hip_selection_risk import _video
    enc, vs, _ = full
    dev = vs.device
    g = torch.Generator(device=dev).manual_seed(77)
    A = torch.rand(3, 378, 378, device=dev, generator=g) * 2 - 1
    B = torch.rand(3, 378, 378, device=dev, generator=g) * 2 - 1
    # calibration (as test_hip_selection_risk): 1 - similarity of the engine's DINOv2 tower against the angle step, then
    # steps whose dissimilarities are 4.9e-3 apart (> 4 selection_eps) except three equal ones at the decisive rank (24 of 47)
    ladder = torch.tensor(np.geomspace(2e-3, 0.6, T - 1), device=dev, dtype=torch.float32)
    cal = _video(A, B, ladder)
    q = np.maximum.accumulate(1.0 - np.asarray(enc.sims_tensor(enc.tower("dino", cal), T).cpu().tolist()))
    lo, hi = 0.02, 0.25
    assert q[0] < lo and q[-1] > hi, (q[0], q[-1])
    targets = lo + (hi - lo) * (np.arange(T - 1) + 0.5) / (T - 1)
    targets[22:25] = targets[23]
    steps = np.interp(targets, q, ladder.cpu().numpy())
    steps = torch.tensor(steps[np.random.RandomState(5).permutation(T - 1)], device=dev, dtype=torch.float32)
    vd = _video(A, B, steps)
    ref = {}
    want = run(enc, vs, vd, info=ref)
    assert ref.get("refined_pairs"), "the video must trigger the selection refinement"
    c = enc.new_cache(4 << 30)
    for _ in range(2):
        info = {}
        assert torch.equal(run(enc, vs, vd, cache=c, info=info), want)
        assert info["seg_indices"] == ref["seg_indices"] and info["refined_pairs"] == ref["refined_pairs"]
    assert info["cache"]["pairs_computed"] == 0


def test_raw_waveform_audio_through_beats(full):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_beats import random_beats_state
    from tdc_video_amd import weights as Wt
    from tdc_video_amd.beats import BEATS_ITER3_CFG, BeatsEncoder
    enc, vs, vd = full
    dev = vs.device
    gen = torch.Generator(device=dev).manual_seed(5)
    H = enc.c.H
    saved = enc.cfg.get("audio_input"), enc.c.audio_proj, enc.beats
    enc.cfg["audio_input"] = True
    enc.c.audio_proj = Wt.make_lin(torch.randn(H, 768, device=dev, generator=gen) * 0.02, torch.zeros(H, device=dev),
                                   enc.dtype, dev)
    enc.beats = BeatsEncoder(random_beats_state(BEATS_ITER3_CFG), BEATS_ITER3_CFG, dtype=enc.dtype, device=dev)
    try:
        wav = (0.1 * torch.randn(1, 16000 * T + 4321, device=dev, generator=gen)).half()
        audio = {"audio_wav": wav}
        want = run(enc, vs, vd, audio=audio)
        c = enc.new_cache(4 << 30)
        i1, i2 = {}, {}
        assert torch.equal(run(enc, vs, vd, audio=audio, cache=c, info=i1), want)
        assert i1["cache"]["windows_encoded"] > 0
        assert torch.equal(run(enc, vs, vd, audio={"audio_wav": wav.clone()}, cache=c, info=i2), want)
        assert i2["cache"]["windows_encoded"] == 0 and i2["cache"]["frames_encoded"] == 0
    finally:
        enc.cfg["audio_input"], enc.c.audio_proj, enc.beats = saved
        if saved[0] is None:
            enc.cfg.pop("audio_input")


# ------------------------------------------------------------------------------------------------ boundary (model.py)
def _boundary_call(lm, ids, vid, o, prompt):
    return lm.prepare_inputs_labels_for_multimodal(ids, None, torch.ones_like(ids), None, ids.clone(),
                                                   [vid.unsqueeze(0), (vid + 0.01).unsqueeze(0)],
                                                   image_sizes=[tuple(int(v) for v in o["image_size"])],
                                                   video_indices=[None], prompts=[prompt], audios=[None])


def _same(a, b):
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert torch.equal(x, y)
        else:
            assert x == y


def test_boundary_cache_config():
    import synth
    import torch.distributed as dist
    from test_hip_boundary import loaded_lm
    from util import load_fixture
    W, o = load_fixture("pipeline_T40.npz")
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    ids = torch.from_numpy(o["input_ids"])
    text = [j for j in range(ids.shape[1]) if int(ids[0, j]) != -200]
    ids2 = ids[:, [j for j in range(ids.shape[1]) if j not in text[-3:-1]]]          # a shorter question
    pid = [int(i) for i in o["prompt_ids"]]
    calls = ((ids, pid), (ids2, pid[:4] + pid[-1:]))
    off = loaded_lm(W, o)
    want = [_boundary_call(off, i, vid, o, p) for i, p in calls]
    on = loaded_lm(W, o, tdc_video_cache_bytes=1 << 30)
    for (i, p), w in zip(calls, want):
        _same(_boundary_call(on, i, vid, o, p), w)
    st = on.get_model().tdc_video_cache().stats()
    assert 0 < st["frames_encoded"] <= 40 and st["hits"] > 0
    # single images share the store
    img = [vid[5:6] * 0.5, vid[5:6] * 0.5 + 0.01]
    size = [tuple(int(v) for v in o["image_size"])]
    want_img = off.prepare_inputs_labels_for_multimodal(ids, None, torch.ones_like(ids), None, ids.clone(), img, image_sizes=size)
    for _ in range(2):
        _same(on.prepare_inputs_labels_for_multimodal(ids, None, torch.ones_like(ids), None, ids.clone(), img,
                                                      image_sizes=size), want_img)
    assert on.get_model().tdc_video_cache().stats()["frames_encoded"] == st["frames_encoded"] + 1
    on.get_model().tdc_video_cache_clear()
    assert on.get_model().tdc_video_cache().stats()["frames"] == 0
    with pytest.raises(ValueError):
        _boundary_call(loaded_lm(W, o, tdc_video_cache_bytes=-5), ids, vid, o, pid)
    # frame sharding (here a world-1 group): the cache is ignored, the results are the serial ones
    sh = loaded_lm(W, o, tdc_video_cache_bytes=1 << 30, tdc_shard_frames=True)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for (i, p), w in zip(calls, want):
            _same(_boundary_call(sh, i, vid, o, p), w)
        assert sh.get_model().tdc_video_cache() is None
    finally:
        dist.destroy_process_group()
