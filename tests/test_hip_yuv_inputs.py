"""GPU (-m gpu): encode from YUV 4:2:0 frames.  tdc_yuv420_to_rgb against the numpy statement of the
conversion (yuv_cases) - all 2^24 triples, the shapes where indexing can go wrong, its memory contract and its refusals - and
the frames funnel on the tiny fixture engine of test_hip_frame_inputs: everything behind the conversion is the RGB frames
path, so every comparison is bit for bit against the same call on the definition's RGB frames."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import memcheck
import test_hip_memory_contract as contract
import yuv_cases as yc
from test_hip_boundary import loaded_lm
from test_hip_frame_inputs import IDX, R, _call, _same, fx, reference_pixels, towers  # noqa: F401  (fx: the engine fixture)

pytestmark = pytest.mark.gpu

LAYOUTS = ("nv12", "nv21", "i420")
BT601 = yc.TABLE["bt601", False]


def convert(s, flats, coef):
    """one tdc_yuv420_to_rgb call on the surface s, whose buffers are the flat device tensors `flats`"""
    from tdc_video_amd import ops
    y, u, v = s.views(flats)
    return ops.yuv420_to_rgb(y, u, v, s.c_step, coef, s.H, s.W)


def on_device(s):
    return [torch.from_numpy(b).cuda() for b in s.bufs]


# ---------------------------------------------------------------------------------------------------- values
@functools.lru_cache(maxsize=None)
def cube_on_device():
    y, u, v = yc.cube()
    return (y, u, v), {lay: (s, on_device(s)) for lay in ("nv12", "i420") for s in [yc.Surface(y, u, v, lay)]}


@pytest.mark.parametrize("matrix,full_range", yc.SETTINGS)
def test_every_triple_equals_the_definition(matrix, full_range):
    from tdc_video_amd import preprocess as pp
    (y, u, v), dev = cube_on_device()
    coef = pp.yuv_coefficients(matrix, full_range)
    assert coef == yc.TABLE[matrix, full_range]
    want = torch.from_numpy(yc.to_rgb(y, u, v, coef)).cuda()
    for lay, (s, flats) in dev.items():
        assert torch.equal(convert(s, flats, coef), want), lay


# ---------------------------------------------------------------------------------------------------- shapes
def up8(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("H,W", [(1, 1), (2, 8), (3, 5), (5, 24), (4, 20), (6, 16)])
def test_shapes_pitches_frame_strides_and_layouts(H, W):
    """T = 3 with frame strides larger than the planes.  Aligned pitches and gaps (the 8-pixel form where W % 8 == 0) and
    y_pitch = W + 3 with an odd c_pitch (the 2 x 2 form) both equal the definition, hence each other."""
    y, u, v = yc.random_planes(3, H, W)
    Wc = (W + 1) // 2
    for k, coef in enumerate((BT601, yc.TABLE["bt709", True])):
        want = torch.from_numpy(yc.to_rgb(y, u, v, coef)).cuda()
        for lay in LAYOUTS:
            cs = 1 if lay == "i420" else 2
            odd = cs * Wc + 1 + (cs * Wc) % 2
            for y_pitch, c_pitch, y_gap, c_gap in ((up8(W) + 8, up8(cs * Wc) + 8, 64, 32), (W + 3, odd, 5, 3), (None, None, 0, 0)):
                s = yc.Surface(y, u, v, lay, y_pitch, c_pitch, y_gap, c_gap, fill=0xA5)
                got = convert(s, on_device(s), coef)
                assert torch.equal(got, want), (lay, y_pitch, c_pitch)
            if k == 0:                                            # one frame of three, through the view's offset
                s = yc.Surface(y, u, v, lay, up8(W) + 8, up8(cs * Wc) + 8, 64, 32)
                yv, uv, vv = s.views(on_device(s))
                from tdc_video_amd import ops
                assert torch.equal(ops.yuv420_to_rgb(yv[1:2], uv[1:2], vv[1:2], cs, coef, H, W), want[1:2])


# ---------------------------------------------------------------------------------------------------- the memory contract
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  tdc_yuv420_to_rgb's is the function below: it is entered
# there under its own name (not a test_ name: that module collects nothing new).
@contract.covers("tdc_yuv420_to_rgb")
def yuv420_to_rgb_memory_contract(H, W):
    """tdc_yuv420_to_rgb: rgb in a guarded arena - nothing outside [T, H, W, 3] changes; the planes in poisoned arenas whose
    pitch padding, byte after an odd chroma row and gaps between frames hold 0x00, then 0xFF - identical output."""
    from tdc_video_amd import ops
    T = 2
    y, u, v = yc.random_planes(T, H, W, seed=1)
    want = torch.from_numpy(yc.to_rgb(y, u, v, BT601)).cuda()
    Wc = (W + 1) // 2
    for lay in LAYOUTS:
        cs = 1 if lay == "i420" else 2
        for y_pitch, c_pitch, y_gap, c_gap in ((up8(W) + 8, up8(cs * Wc) + 8, 16, 8), (W + 3, cs * Wc + 1, 7, 5)):
            results = []
            for pattern in memcheck.PATTERNS:
                s = yc.Surface(y, u, v, lay, y_pitch, c_pitch, y_gap, c_gap, fill=pattern)
                flats = [memcheck.poisoned(torch.from_numpy(b).cuda(), 256, 256, fill=pattern)[0] for b in s.bufs]
                out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
                yv, uv, vv = s.views(flats)
                ops.yuv420_to_rgb(yv, uv, vv, cs, BT601, H, W, out=out)
                torch.cuda.synchronize()
                memcheck.assert_untouched(arena)
                assert torch.equal(out, want), (lay, y_pitch, pattern)
                results.append(out.clone())
            assert torch.equal(*results)


contract.yuv420_to_rgb_memory_contract = yuv420_to_rgb_memory_contract


@pytest.mark.parametrize("H,W", [(3, 5), (6, 16), (5, 24)])
def test_memory_contract(H, W):
    yuv420_to_rgb_memory_contract(H, W)


# ---------------------------------------------------------------------------------------------------- refusals
def test_badarg_before_any_launch():
    from tdc_video_amd import lib as L
    lib = L.load()
    T, H, W = 2, 4, 6
    y, u, v = yc.random_planes(T, H, W)
    s = yc.Surface(y, u, v, "nv12", 8, 8, 8, 8)
    flats = on_device(s)
    out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
    yp, up = flats[0].data_ptr(), flats[1].data_ptr()
    good_p = dict(y=yp, u=up, v=up + 1, y_frame=s.y_frame, c_frame=s.c_frame, y_pitch=8, c_pitch=8, c_step=2)
    good_c = dict(zip(("y_off", "cy", "crv", "cgu", "cgv", "cbu"), BT601))

    def rc(p=None, c=None, dims=(T, H, W), rgb=out.data_ptr(), null=None):
        ps, cs = L.Yuv420Planes(**dict(good_p, **(p or {}))), L.YuvCoef(**dict(good_c, **(c or {})))
        return lib.tdc_yuv420_to_rgb(None if null == "p" else C.byref(ps), None if null == "c" else C.byref(cs), *dims,
                                     C.c_void_p(rgb), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [rc(null="p"), rc(null="c"), rc(rgb=0), rc(p=dict(y=0)), rc(p=dict(u=0)), rc(p=dict(v=0))]
    for i in range(3):
        for n in (0, -1, 65536):
            dims = [T, H, W]
            dims[i] = n
            bad.append(rc(dims=tuple(dims)))
    bad += [rc(p=dict(y_pitch=5)), rc(p=dict(c_pitch=5)), rc(p=dict(c_step=1, c_pitch=2)),
            rc(p=dict(y_frame=3 * 8 + 5)), rc(p=dict(c_frame=8 + 4)), rc(p=dict(y_frame=0)), rc(p=dict(c_frame=-8)),
            rc(p=dict(c_step=0)), rc(p=dict(c_step=3)), rc(c=dict(y_off=1)), rc(c=dict(y_off=-16))]
    for k in ("cy", "crv", "cgu", "cgv", "cbu"):
        bad += [rc(c={k: -1}), rc(c={k: (1 << 18) + 1})]
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad      # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(T, dtype=torch.bool))
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_yuv420_to_rgb")
    # the smallest strides that are enough, and the largest coefficients, are taken
    assert rc(p=dict(y_frame=3 * 8 + 6, c_frame=8 + 6), c=dict(cy=1 << 18, cbu=1 << 18, crv=0)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the funnel
def yuv_sources(y, u, v, lay):
    """the same video as YuvFrames over device surfaces with a pitch, pageable host surfaces with an odd pitch, and dense
    pinned planes"""
    from tdc_video_amd import preprocess as pp
    W = y.shape[2]
    Wc = (W + 1) // 2
    cs = 1 if lay == "i420" else 2
    make = (lambda planes: pp.YuvFrames.nv12(*planes, width=W)) if lay == "nv12" else (lambda planes: pp.YuvFrames.i420(*planes, width=W))
    a = yc.Surface(y, u, v, lay, up8(W) + 8, up8(cs * Wc) + 8, 64, 32, fill=0xFF)
    b = yc.Surface(y, u, v, lay, W + 3, cs * Wc + 1, 7, 5, fill=0xFF)
    c = yc.Surface(y, u, v, lay)
    return {"cuda": make(a.planes(on_device(a))), "pageable": make(b.planes([torch.from_numpy(x) for x in b.bufs])),
            "pinned": make(c.planes([torch.from_numpy(x).pin_memory() for x in c.bufs]))}


@pytest.mark.parametrize("H,W", [(90, 160), (160, 90), (126, 126), (45, 81)])
def test_preprocess_selected_on_yuv_equals_process_images_of_the_definitions_rgb(H, W):
    from tdc_video_amd import preprocess as pp
    y, u, v = yc.random_planes(16, H, W)
    rgb = torch.from_numpy(yc.to_rgb(y, u, v, BT601))
    want = reference_pixels(rgb[IDX])
    want_all = reference_pixels(rgb)
    nbytes = H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
    for lay in ("nv12", "i420"):
        for name, src in yuv_sources(y, u, v, lay).items():
            for slab in (1, 7, 64):
                stats = {}
                got = pp.preprocess_selected(src, IDX, towers(), torch.float16, slab, stats=stats)
                assert len(got) == 2
                for g, w in zip(got, want):
                    assert g.is_cuda and tuple(g.shape) == (10, 3, R, R) and memcheck.same_bits(g, w), (lay, name, slab)
                assert stats == dict(frames_in=16, frames_resized=10, bytes_uploaded=0 if name == "cuda" else 10 * nbytes)
            # idx=None: device surfaces are read in place through their strides, dense pinned planes uploaded as they lie
            stats = {}
            got = pp.preprocess_selected(src, None, towers(), torch.float16, 7, stats=stats)
            assert all(memcheck.same_bits(g, w) for g, w in zip(got, want_all)), (lay, name)
            assert stats["bytes_uploaded"] == (0 if name == "cuda" else 16 * nbytes)
    got = pp.preprocess_selected(yuv_sources(y, u, v, "nv12")["pinned"], IDX, towers(), torch.bfloat16, 7)
    assert all(memcheck.same_bits(g, w) for g, w in zip(got, reference_pixels(rgb[IDX], torch.bfloat16)))


def test_preprocess_selected_on_yuv_memory_contract(monkeypatch):
    """outputs in guarded arenas, both scratches allocated through torch.empty and guarded, dropped frames and padding holding
    0x00, then 0xFF: bit-identical outputs, nothing written outside out[0:len(idx)] or outside a scratch"""
    import importlib
    pp = importlib.import_module("tdc_video_amd.preprocess")      # under the name memcheck.poison_empty looks for
    H, W = 90, 160
    y, u, v = yc.random_planes(16, H, W)
    want = reference_pixels(torch.from_numpy(yc.to_rgb(y, u, v, BT601))[IDX])
    T = len(IDX)
    results = []
    for pattern in memcheck.PATTERNS:
        yy, uu, vv = (p.copy() for p in (y, u, v))
        for p in (yy, uu, vv):
            p[[t for t in range(16) if t not in IDX]] = pattern
        s = yc.Surface(yy, uu, vv, "nv12", up8(W) + 8, W + 8, 64, 32, fill=pattern)
        src = pp.YuvFrames.nv12(*s.planes(on_device(s)), width=W)
        outs = [memcheck.guarded((T + 2, 3, R, R), torch.float16, "cuda", 1, 1) for _ in range(2)]
        with monkeypatch.context() as mp:
            inner = memcheck.poison_empty(mp, pattern, guard_bytes=4096)
            got = pp.preprocess_selected(src, IDX, towers(), torch.float16, 3, out=[o for o, _ in outs])
        torch.cuda.synchronize()
        rows = torch.zeros(T + 2, dtype=torch.bool)
        rows[:T] = True
        for (_, arena), g, w in zip(outs, got, want):
            memcheck.assert_untouched(arena, rows)
            assert memcheck.same_bits(g, w)
        assert len(inner) >= 2, "the scratches were not allocated through torch.empty"
        for a in inner:
            memcheck.assert_untouched(a, what="scratch")
        results.append([g.clone() for g in got])
    assert all(memcheck.same_bits(a, b) for a, b in zip(*results))


# ---------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def video(H=90, W=160, T0=40):
    """(nv12 YuvFrames over host surfaces with a pitch, i420 YuvFrames over numpy planes, the definition's RGB frames)"""
    from tdc_video_amd import preprocess as pp
    y, u, v = yc.random_planes(T0, H, W, seed=4)
    for t in range(T0):                                           # scenes of five frames, so that the segmentation has cuts to find
        if t % 5:
            y[t] = np.clip(y[t - t % 5].astype(np.int32) + (y[t] % 7).astype(np.int32) - 3, 0, 255)
            u[t], v[t] = u[t - t % 5], v[t - t % 5]
    s = yc.Surface(y, u, v, "nv12", W + 16, None, 32, 0, fill=0xFF)
    nv12 = pp.YuvFrames.nv12(*s.planes([torch.from_numpy(b) for b in s.bufs]), width=W)
    return nv12, pp.YuvFrames.i420(y, u, v), torch.from_numpy(yc.to_rgb(y, u, v, BT601))


def test_encode_frames_and_prompts(fx):  # noqa: F811
    enc, pid = fx["enc"], fx["pid"]
    nv12, i420, rgb = video()
    wi, gi = {}, {}
    want = enc.encode_frames(rgb, 9, 8, pid, frame_cap=30, info=wi)
    assert torch.equal(enc.encode_frames(nv12, 9, 8, pid, frame_cap=30, info=gi), want) and gi == wi and gi["frames_resized"] == 30
    assert torch.equal(enc.encode_frames(i420, 9, 8, pid, frame_cap=30), want)
    assert torch.equal(enc.encode_frames(nv12, 9, 8, pid), enc.encode_frames(rgb, 9, 8, pid))        # every frame kept
    qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid),
          dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:])]
    for a, b in zip(enc.encode_frames_prompts(nv12, qs, frame_cap=30, pad_fraction=1.0),
                    enc.encode_frames_prompts(rgb, qs, frame_cap=30, pad_fraction=1.0)):
        assert torch.equal(a, b)
    i1, i2 = {}, {}
    assert torch.equal(enc.encode_frames(i420[3:4], None, 8, None, image=True, info=i1),
                       enc.encode_frames(rgb[3:4], None, 8, None, image=True, info=i2)) and i1 == i2


def test_export_features_from_yuv(fx):  # noqa: F811
    enc = fx["enc"]
    nv12, _, rgb = video()
    for store in ("f16", "e4m3"):
        want = enc.export_features_from_frames(rgb, store=store, slab=16)
        got = enc.export_features_from_frames(nv12, store=store, slab=16)
        assert got.signature == want.signature and got.image_size == want.image_size == (90, 160) and got.frames == 40
        assert memcheck.same_bits(got.siglip, want.siglip) and memcheck.same_bits(got.dino, want.dino)
        if store == "e4m3":
            assert torch.equal(got.siglip_scale, want.siglip_scale) and torch.equal(got.dino_scale, want.dino_scale)
            assert torch.equal(got.sims, want.sims)


def test_frame_cache_rgb_first_yuv_second_is_all_hits(fx):  # noqa: F811
    enc, pid = fx["enc"], fx["pid"]
    nv12, _, rgb = video()
    c = enc.new_cache(1 << 30)
    i1, i2 = {}, {}
    want = enc.encode_frames(rgb, 9, 8, pid, frame_cap=30, info=i1, cache=c)
    assert i1["cache"]["frames_encoded"] == 30
    assert torch.equal(enc.encode_frames(nv12, 9, 8, pid, frame_cap=30, info=i2, cache=c), want)
    assert i2["cache"]["frames_encoded"] == 0 and i2["cache"]["frames_hit"] == i2["cache"]["frames"] == 30


def test_mixin_yuv_inputs_equal_the_rgb_call(fx):  # noqa: F811
    nv12, i420, rgb = video()
    lm = loaded_lm(fx["W"], fx["o"], tdc_frame_cap=30)
    ids = torch.from_numpy(fx["o"]["input_ids"])
    lm.get_model().tdc_engine().frame_towers = towers()
    lm.get_model().config.tdc_frame_inputs = True
    want = _call(lm, ids, [[rgb], None], (90, 160), [fx["pid"]])
    _same(_call(lm, ids, [[nv12], None], (90, 160), [fx["pid"]]), want)
    _same(_call(lm, ids, [[i420], [None]], (90, 160), [fx["pid"]]), want)
    want_im = _call(lm, ids, [rgb[:2], None], (90, 160), [fx["pid"]] * 2, 2)
    _same(_call(lm, ids, [nv12[:2], None], (90, 160), [fx["pid"]] * 2, 2), want_im)
