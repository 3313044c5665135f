"""GPU (-m gpu): the reference's three aux outputs of the 10-tuple on the reduced reference fixtures
(C = 64, side 4, r 2, 126-px frames) - tdc_connector_fwd with aux_keep / ctx_keep against the composite without them and the
per-kernel sequence, inside guarded arenas; encode_video(aux=) against the engine's own aux rows through the index maps the
reference's outputs were recorded as (tests/golden/aux_outputs.npz) and against the reference's values; the gather maps at the
production grid against the oracle's geometry; and `config.tdc_return_aux` through the mixin for pixel, frame and feature
inputs.  Everything that compares the engine with itself is bit for bit."""
import types

import numpy as np
import pytest
import torch

import memcheck
import synth
from test_aux_outputs import CASES, oracle_composition
from test_hip_boundary import loaded_lm
from test_hip_frame_inputs import frames_of, reference_pixels, towers
from test_hip_pipeline import MIXED_R16, make_encoder, rel, stage_tol
from util import GOLDEN, load_fixture, pipeline_cfg

pytestmark = pytest.mark.gpu

PIPELINE = {"T40": "pipeline_T40.npz", "T10_land": "pipeline_T10_land.npz", "T10_480x640": "pipeline_T10_land.npz"}
C, SIDE, R, P = 64, 4, 2, 64
_CACHE = {}


def golden(case):
    if "aux" not in _CACHE:
        z = np.load(GOLDEN + "/aux_outputs.npz", allow_pickle=False)
        _CACHE["aux"] = {c: {k.split("::", 1)[1]: z[k] for k in z.files if k.startswith(c + "::")} for c in CASES}
    return _CACHE["aux"][case]


def setup(case, dtype):
    """(engine, fixture arrays, pixels on the device) of a case - one engine per (pipeline fixture, type), made once"""
    name = PIPELINE[case]
    if name not in _CACHE:
        W, o = load_fixture(name)
        vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"])).cuda()
        _CACHE[name] = (W, o, vid)
    W, o, vid = _CACHE[name]
    if (name, dtype) not in _CACHE:
        _CACHE[(name, dtype)] = make_encoder(W, pipeline_cfg(o), dtype)
    return _CACHE[(name, dtype)], o, vid


# ------------------------------------------------------------------------------------------------- the composite
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_composite_keeps_its_aux_rows_in_the_callers_buffers(dtype):
    from tdc_video_amd import ops
    enc, o, vid = setup("T10_land", dtype)
    T = 10
    sig, dino = enc.tower("siglip", vid), enc.tower("dino", vid + 0.01)
    sizes = [(360, 640)] * T
    plain = enc._connector_native(sig, dino, T, sizes)
    arenas = [memcheck.guarded((n, C), enc.dtype, "cuda", 4, 4) for n in (T * P, T * P, T)]
    kept = tuple(v for v, _ in arenas)
    assert all(v.data_ptr() % 256 == 0 for v in kept)
    out = enc._connector_native(sig, dino, T, sizes, kept)
    assert torch.equal(out, plain)
    keep = {}
    enc.connector(sig, dino, T, sizes, keep=keep)                   # the per-kernel sequence
    assert torch.equal(kept[0], keep["aux0"]) and torch.equal(kept[1], keep["aux1"])
    assert torch.equal(kept[2], ops.token_mean(keep["aux0"], T, P))
    for (_, a), what in zip(arenas, ("aux_keep[0]", "aux_keep[1]", "ctx_keep")):
        memcheck.assert_untouched(a, what=what)                     # write set: the whole [rows, pad64(C)] view, nothing around it
    # the cached model struct was not touched: the next plain call is the plain call
    assert torch.equal(enc._connector_native(sig, dino, T, sizes), plain)


# ------------------------------------------------------------------------------------------------- the engine
@pytest.mark.parametrize("dtype", [torch.float16, MIXED_R16])
@pytest.mark.parametrize("case", CASES)
def test_encode_video_aux_outputs(case, dtype):
    from tdc_video_amd import ops
    enc, o, vid = setup(case, dtype)
    g = golden(case)
    size = tuple(int(v) for v in g["image_size"])
    ids = o["input_ids"][0]
    args = (vid, vid + 0.01, size, len(ids), len(ids) - 1, [int(i) for i in o["prompt_ids"]])
    T = vid.shape[0]
    plain = enc.encode_video(*args)
    d, info = {}, {}
    vis = enc.encode_video(*args, aux=d, info=info)
    assert torch.equal(vis, plain)
    assert [list(s) for s in info["final_size"]] == g["final_size"].tolist()
    keep = {}
    enc.encode_video(*args, keep=keep)                              # the engine's own aux rows (per-kernel connector)
    assert len(keep["selected"]) == T
    n = g["ctx_src"].shape[0]
    mean = ops.token_mean(keep["aux0"], T, P)
    ctx_src = torch.from_numpy(g["ctx_src"]).long().cuda()
    for i in range(2):
        src = torch.from_numpy(g["feat_src%d" % i]).long().cuda()
        f = d["features"][i]
        assert tuple(f.shape) == (n, R * R, C) and f.dtype == enc.dtype and f.is_contiguous() and f.is_cuda
        assert torch.equal(f, keep["aux%d" % i][:, :C][src])
        m = d["masks"][i]
        assert m.dtype == torch.bool and m.is_cuda and torch.equal(m.cpu(), torch.from_numpy(g["mask%d" % i]))
    gc = d["global_context"]
    assert tuple(gc.shape) == (n, 1, C) and gc.dtype == enc.dtype and gc.is_contiguous()
    assert torch.equal(gc[:, 0], mean[:, :C][ctx_src])
    # both connector routes give the same bits
    enc.native_connector = False
    try:
        d2 = {}
        assert torch.equal(enc.encode_video(*args, aux=d2), plain)
    finally:
        enc.native_connector = True
    for i in range(2):
        assert torch.equal(d2["features"][i], d["features"][i]) and torch.equal(d2["masks"][i], d["masks"][i])
    assert torch.equal(d2["global_context"], gc)
    # against the reference's values: the bound the stage test holds aux0 to
    for i in range(2):
        want = o["out_aux%d" % i].reshape(T * P, C)[g["feat_src%d" % i]]
        err = rel(d["features"][i], want)
        print("%s %s: features[%d] error %.3e of max|ref|" % (case, dtype, i, err))
        assert err < stage_tol(dtype, "aux0"), (i, err)
    err = rel(gc[:, 0], g["ctx_rows"][g["ctx_src"]])
    print("%s %s: global_context error %.3e of max|ref|" % (case, dtype, err))
    assert err < stage_tol(dtype, "aux0"), err


def test_aux_with_cache_raises():
    enc, o, vid = setup("T10_land", torch.float16)
    ids = o["input_ids"][0]
    cache = enc.new_cache(1 << 24)
    with pytest.raises(ValueError, match="aux=.*cache="):
        enc.encode_video(vid, vid + 0.01, (360, 640), len(ids), len(ids) - 1, [1, 2], cache=cache, aux={})
    with pytest.raises(ValueError, match="aux=.*cache="):
        enc.encode_video(vid[:1], vid[:1] + 0.01, (360, 640), None, len(ids) - 1, None, cache=cache, aux={}, image=True)
    assert cache.stats()["frames_encoded"] == 0


# ------------------------------------------------------------------------------------------------- the production grid
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_gather_maps_at_the_production_grid(dtype):
    """side 12, r 2, P = 576: three frames of three sizes - one call with per-frame sizes and the image form (one frame a call) -
    give the oracle composition's rows bit for bit.  C = 72 under a row stride of 128: the pad columns are stripped."""
    from tdc_video_amd import ops
    from tdc_video_amd.pipeline import VideoEncoder, _LRU
    from util import oracle
    side, r, Pp, T, Cc, Cp = 12, 2, 576, 3, 72, 128
    sizes = [(384, 384), (360, 640), (480, 640)]
    enc = VideoEncoder.__new__(VideoEncoder)
    enc.dtype, enc.dev, enc.side, enc._tables = dtype, torch.device("cuda"), side, _LRU(32)
    enc.c = types.SimpleNamespace(C=Cc)
    gen = torch.Generator().manual_seed(18)
    rows = [torch.zeros(T * Pp, Cp, dtype=dtype) for _ in range(2)]
    for x in rows:
        x[:, :Cc] = torch.randn(T * Pp, Cc, generator=gen).to(dtype)
        x[:, Cc:] = float("nan")                                    # columns the gather is not given
    dev = [x.cuda() for x in rows]
    ctx = ops.token_mean(dev[0], T, Pp)
    d = {}
    enc.aux_outputs(dev[0], dev[1], ctx, T, sizes, d)
    want_f, want_m, want_c = [[], []], [], []
    for t, size in enumerate(sizes):
        src, mask, hw = oracle_composition(side, r, size)
        assert hw[0] * hw[1] > 0
        for i in range(2):
            win = oracle.rearrange_windows(rows[i][:, :Cc].reshape(T, Pp, Cc)[t:t + 1], side).view(side, side, r * r, Cc)
            r0, r1, c0, c1 = oracle.unpad_bounds(side, side, size)
            want_f[i].append(win[r0:r1, c0:c1].reshape(-1, r * r, Cc))
        want_m.append(torch.from_numpy(mask))
        want_c.append(ctx[t:t + 1, :Cc].cpu().expand(hw[0] * hw[1], -1))
    n = sum(m.shape[0] for m in want_m)
    assert n == 144 + 12 * 6 + 120
    for i in range(2):
        assert tuple(d["features"][i].shape) == (n, r * r, Cc) and d["features"][i].is_contiguous()
        assert memcheck.same_bits(d["features"][i].cpu(), torch.cat(want_f[i], 0))
        assert torch.equal(d["masks"][i].cpu(), torch.cat(want_m, 0))
    assert memcheck.same_bits(d["global_context"].cpu(), torch.cat(want_c, 0)[:, None, :].contiguous())
    assert int((~d["masks"][0].all(-1)).sum()) == 24                # the (480, 640) frame's windows with masked entries
    # the image form: every frame a call of its own
    parts = []
    for t, size in enumerate(sizes):
        e = {}
        enc.aux_outputs(dev[0][t * Pp:(t + 1) * Pp], dev[1][t * Pp:(t + 1) * Pp], ctx[t:t + 1], 1, [size], e)
        parts.append(e)
    for i in range(2):
        assert torch.equal(torch.cat([e["features"][i] for e in parts], 0), d["features"][i])
        assert torch.equal(torch.cat([e["masks"][i] for e in parts], 0), d["masks"][i])
    assert torch.equal(torch.cat([e["global_context"] for e in parts], 0), d["global_context"])


# ------------------------------------------------------------------------------------------------- the mixin
def _call(lm, ids, images, size, prompts, n=1):
    ids = ids.repeat(n, 1)
    return lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, images, image_sizes=[size] * n,
                                                   video_indices=[None] * n, prompts=prompts, audios=[None] * n)


def _same_aux(a, b):
    for i in range(2):
        assert torch.equal(a[6][i], b[6][i]) and torch.equal(a[7][i], b[7][i]), i
    assert torch.equal(a[9], b[9])


def test_mixin_returns_the_three_slots_for_pixel_frame_and_feature_inputs():
    H, W = 90, 160
    frames = frames_of(H, W)
    ps, pd = reference_pixels(frames)
    Wt, o = load_fixture("pipeline_T40.npz")
    pid = [[int(i) for i in o["prompt_ids"]]]
    lm = loaded_lm(Wt, o, tdc_frame_cap=30)
    cfg = lm.get_model().config
    ids = torch.from_numpy(o["input_ids"])
    eng = lm.get_model().tdc_engine()
    eng.frame_towers = towers()
    off = _call(lm, ids, [[ps], [pd]], (H, W), pid)
    off_im = _call(lm, ids, [ps[:2], pd[:2]], (H, W), pid * 2, 2)
    assert all(off[i] is None and off_im[i] is None for i in (6, 7, 9))
    cfg.tdc_return_aux = True
    on = _call(lm, ids, [[ps], [pd]], (H, W), pid)
    on_im = _call(lm, ids, [ps[:2], pd[:2]], (H, W), pid * 2, 2)
    for a, b in ((on, off), (on_im, off_im)):
        assert torch.equal(a[4], b[4]) and a[8] == b[8] and all(a[i] is None for i in (0, 1, 2, 3, 5))
    for out in (on, on_im):
        n = sum(h * w for h, w in out[8])
        assert n > 0 and isinstance(out[6], list) and isinstance(out[7], list) and len(out[6]) == len(out[7]) == 2
        for i in range(2):
            assert tuple(out[6][i].shape) == (n, 4, C) and out[6][i].dtype == torch.float16 and out[6][i].is_cuda
            assert tuple(out[7][i].shape) == (n, 4) and out[7][i].dtype == torch.bool and out[7][i].is_cuda
        assert tuple(out[9].shape) == (n, 1, C) and out[9].dtype == torch.float16
    assert len(on[8]) == 30 and len(on_im[8]) == 2
    # bsz = 2 images: sample order along dim 0
    one = _call(lm, ids, [ps[1:2], pd[1:2]], (H, W), pid)
    k = one[9].shape[0]
    assert torch.equal(on_im[6][0][k:], one[6][0]) and torch.equal(on_im[9][k:], one[9])
    # decoded frames in
    cfg.tdc_frame_inputs = True
    _same_aux(_call(lm, ids, [[frames], None], (H, W), pid), on)
    _same_aux(_call(lm, ids, [frames[:2], None], (H, W), pid * 2, 2), on_im)
    cfg.tdc_frame_inputs = False
    # stored tower features in
    fs = eng.export_features(ps.cuda(), pd.cuda(), (H, W))
    fs_im = [eng.export_features(ps[i:i + 1].cuda(), pd[i:i + 1].cuda(), (H, W)) for i in range(2)]
    cfg.tdc_feature_inputs = True
    got = _call(lm, ids, [[fs], [None]], (H, W), pid)
    _same_aux(got, on)
    assert torch.equal(got[4], off[4]) and got[8] == off[8]
    im = [torch.cat([f.siglip for f in fs_im], 0), torch.cat([f.dino for f in fs_im], 0)]         # images: [bsz, tokens, width]
    _same_aux(_call(lm, ids, im, (H, W), pid * 2, 2), on_im)
