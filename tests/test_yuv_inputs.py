"""CPU: encode from YUV 4:2:0 frames.  The conversion's definition against real arithmetic over all 2^24
(Y, U, V) triples, the YuvFrames container, the host-side gather that never reads a dropped frame or pitch padding, and the
frames funnel (encode.FrameSource, the mixin's config.tdc_frame_inputs) taking a YuvFrames where it takes RGB frames - on the
engine double of test_frame_inputs, whose pixels are the preprocess double's of the definition's RGB."""
import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
import yuv_cases as yc
from tdc_video_amd import encode, preprocess
from test_features import FeatureEngine, FeatureMixinEngine, Untouchable, feature_lm, same_tuple
from test_frame_inputs import SIZE, _Frames, call

YuvFrames = preprocess.YuvFrames
H, W = SIZE                                                       # (4, 6): the engine double's frames


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("matrix,full_range", yc.SETTINGS)
def test_definition_against_real_arithmetic_over_the_whole_cube(matrix, full_range):
    coef = yc.TABLE[matrix, full_range]
    assert preprocess.yuv_coefficients(matrix, full_range) == coef
    U, V = np.meshgrid(np.arange(256), np.arange(256))
    worst, acc = 0, 0
    for y0 in range(0, 256, 32):
        Y = np.arange(y0, y0 + 32)[:, None, None]
        Yb, Ub, Vb = np.broadcast_arrays(Y, U[None], V[None])
        got = yc.channels(Yb, Ub, Vb, coef)
        real = yc.real_channels(Yb, Ub, Vb, matrix, full_range)
        for g, r in zip(got, real):
            want = np.clip(np.floor(r + 0.5), 0, 255)
            worst = max(worst, int(np.abs(g.astype(np.int64) - want.astype(np.int64)).max()))
        y_off, cy, crv, cgu, cgv, cbu = coef                      # the accumulators in int64: int32 is safe
        yy, cb, cr = cy * (Yb.astype(np.int64) - y_off), Ub.astype(np.int64) - 128, Vb.astype(np.int64) - 128
        for a in (yy + crv * cr, yy - cgu * cb - cgv * cr, yy + cbu * cb):
            acc = max(acc, int(np.abs(a + 32768).max()))
    assert worst <= 1, worst
    assert acc < 3.6e7, acc
    # the grey axis
    Y = np.arange(256)
    r, g, b = yc.channels(Y, np.full(256, 128), np.full(256, 128), coef)
    assert np.array_equal(r, g) and np.array_equal(g, b)
    if full_range:
        assert np.array_equal(r, Y)
    else:
        assert r[16] == 0 and r[235] == 255 and r[0] == 0 and r[255] == 255


def test_to_rgb_replicates_chroma_and_handles_odd_sizes():
    y, u, v = yc.random_planes(2, 3, 5)
    rgb = yc.to_rgb(y, u, v, yc.TABLE["bt601", False])
    assert rgb.shape == (2, 3, 5, 3)
    for (t, yy, xx) in ((0, 0, 0), (1, 2, 4), (0, 1, 3), (1, 2, 1)):
        want = [int(c) for c in yc.channels(y[t, yy, xx], u[t, yy >> 1, xx >> 1], v[t, yy >> 1, xx >> 1], yc.TABLE["bt601", False])]
        assert rgb[t, yy, xx].tolist() == want


# ------------------------------------------------------------------------------------------------ the container
def test_yuvframes_describes_planes_without_copying():
    y, u, v = yc.random_planes(5, 4, 6)
    s = yc.Surface(y, u, v, "nv12", y_pitch=8, c_pitch=10, y_gap=16, c_gap=4)
    flats = [torch.from_numpy(b) for b in s.bufs]
    py, puv = s.planes(flats)
    f = YuvFrames.nv12(py, puv, width=6)
    assert f.shape == (5, 4, 6, 3) and not f.is_cuda
    assert encode.frames_size(f) == (5, (4, 6)) and encode.FrameSource(f).T0 == 5
    assert f.y.data_ptr() == flats[0].data_ptr()                  # over the same memory
    assert YuvFrames.nv12(py, puv).shape == (5, 4, 8, 3)          # width defaults to the luma row length
    g = f[1:3]
    assert isinstance(g, YuvFrames) and g.shape == (2, 4, 6, 3) and g.y.data_ptr() == py[1].data_ptr()
    assert g.matrix == f.matrix and g.full_range == f.full_range and g.c_step == 2
    assert [tuple(p.shape) for p in g.planes()] == [(2, 4, 6), (2, 2, 6)]
    with pytest.raises(TypeError):
        f[0]
    # i420, odd H and W, numpy planes, the other settings
    y, u, v = yc.random_planes(2, 3, 5)
    f = YuvFrames.i420(y, u, v, matrix="bt709", full_range=True)
    assert f.shape == (2, 3, 5, 3) and f.coef == yc.TABLE["bt709", True] and f.c_step == 1
    assert [tuple(p.shape) for p in f.planes()] == [(2, 3, 5), (2, 2, 3), (2, 2, 3)]
    assert YuvFrames.i420(y, u, v).coef == yc.TABLE["bt601", False]          # the defaults
    uv = np.stack([u, v], -1).reshape(2, 2, 6)
    assert YuvFrames.nv12(torch.from_numpy(y), uv).shape == (2, 3, 5, 3)      # torch and numpy planes mixed: both on the host


def test_yuvframes_refusals_name_the_plane():
    y, u, v = yc.random_planes(3, 4, 6)
    uv = np.stack([u, v], -1).reshape(3, 2, 6)
    bad = [("y", lambda: YuvFrames.nv12(y.astype(np.int32), uv)),                 # type
           ("y", lambda: YuvFrames.nv12(list(y), uv)),
           ("uv", lambda: YuvFrames.nv12(y, uv.astype(np.float32))),
           ("y", lambda: YuvFrames.nv12(y[0], uv)),                               # rank
           ("uv", lambda: YuvFrames.nv12(y, uv[..., None])),
           ("u", lambda: YuvFrames.i420(y, u[0], v)),
           ("uv", lambda: YuvFrames.nv12(y, uv[:2])),                             # chroma extents against T0, H and W
           ("uv", lambda: YuvFrames.nv12(y, uv[:, :1])),
           ("uv", lambda: YuvFrames.nv12(y, uv[:, :, :5])),
           ("v", lambda: YuvFrames.i420(y, u, v[:, :, :2])),
           ("u", lambda: YuvFrames.i420(y[:, :3], u[:, :1], v)),
           ("uv", lambda: YuvFrames.nv12(y, np.zeros((3, 2, 12), np.uint8)[:, :, ::2])),      # last dimension not dense
           ("strides", lambda: YuvFrames.i420(y, u, np.zeros((3, 2, 4), np.uint8)[:, :, :3])),
           ("width", lambda: YuvFrames.nv12(y, uv, width=7)),
           ("width", lambda: YuvFrames.nv12(y, uv, width=0)),
           ("matrix", lambda: YuvFrames.nv12(y, uv, matrix="bt2020")),
           ("full_range", lambda: YuvFrames.nv12(y, uv, full_range=1))]
    for name, make in bad:
        with pytest.raises(ValueError, match=name):
            make()
    meta = torch.empty(3, 2, 6, dtype=torch.uint8, device="meta")                  # mixed devices, without needing a GPU
    with pytest.raises(ValueError, match="uv is on meta"):
        YuvFrames.nv12(y, meta)
    # odd H and W need the rounded-up chroma extents
    y5 = np.zeros((1, 3, 5), np.uint8)
    with pytest.raises(ValueError, match="u must be"):
        YuvFrames.i420(y5, np.zeros((1, 1, 3), np.uint8), np.zeros((1, 1, 3), np.uint8))
    with pytest.raises(ValueError, match="uv must be"):
        YuvFrames.nv12(y5, np.zeros((1, 2, 5), np.uint8))
    # width < pitch relaxes the chroma rows with it
    assert YuvFrames.nv12(np.zeros((1, 4, 8), np.uint8), np.zeros((1, 2, 6), np.uint8), width=6).shape == (1, 4, 6, 3)


# ------------------------------------------------------------------------------------------------ dropped frames are never read
IDX = [0, 2, 3, 7]


@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("h,w", [(4, 6), (3, 5)])
def test_gather_reads_neither_dropped_frames_nor_padding(layout, h, w):
    y, u, v = yc.random_planes(9, h, w)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    staged = []
    for fill in (0xFF, 0x00):
        yy, uu, vv = (p.copy() for p in (y, u, v))
        for p in (yy, uu, vv):                                    # the dropped frames hold the fill too
            p[[t for t in range(9) if t not in IDX]] = fill
        s = yc.Surface(yy, uu, vv, layout, y_pitch=w + 3, c_pitch=s_c_pitch(layout, wc), y_gap=7, c_gap=5, fill=fill)
        planes = s.planes([torch.from_numpy(b) for b in s.bufs])
        f = YuvFrames.nv12(*planes, width=w) if layout == "nv12" else YuvFrames.i420(*planes, width=w)
        out, stage = preprocess.gather_planes(f, IDX, pin=False)
        assert stage.numel() == len(IDX) * (h * w + 2 * hc * wc) and stage.is_contiguous()
        assert all(o.data_ptr() >= stage.data_ptr() for o in out)
        assert np.array_equal(out[0].numpy(), y[IDX])
        if layout == "i420":
            assert np.array_equal(out[1].numpy(), u[IDX]) and np.array_equal(out[2].numpy(), v[IDX])
        else:
            assert np.array_equal(out[1].numpy().reshape(len(IDX), hc, wc, 2), np.stack([u[IDX], v[IDX]], -1))
        staged.append(stage.clone())
    assert torch.equal(*staged)


def s_c_pitch(layout, wc):
    return (2 * wc if layout == "nv12" else wc) + 3


# ------------------------------------------------------------------------------------------------ the frames funnel
class _YuvFrames(_Frames):
    """the engine double's pixels_from_frames for both kinds of frames: a YuvFrames goes through the product's host gather,
    then the numpy definition; bytes_uploaded as the product counts them"""

    def pixels_from_frames(self, frames, idx=None):
        if preprocess.is_yuv_frames(frames):
            self.kinds = getattr(self, "kinds", []) + ["yuv"]
            keep = list(range(frames.shape[0])) if idx is None else list(idx)
            planes, stage = preprocess.gather_planes(frames, keep, pin=False)
            self.bytes_uploaded = stage.numel()
            y = planes[0].numpy()
            if frames.c_step == 2:
                u, v = planes[1].numpy()[..., 0::2], planes[1].numpy()[..., 1::2]
            else:
                u, v = planes[1].numpy(), planes[2].numpy()
            rgb = yc.to_rgb(y, u, v, frames.coef)
            px = _Frames.pixels_from_frames(self, rgb, None)
            self.asked[-1] = None if idx is None else list(idx)
            return px
        return _Frames.pixels_from_frames(self, frames, idx)


class YuvEngine(_YuvFrames, FeatureEngine):
    pass


def video(T0, layout="nv12", seed=3, pad=True):
    y, u, v = yc.random_planes(T0, H, W, seed)
    s = yc.Surface(y, u, v, layout, y_pitch=W + 2 if pad else None, c_pitch=None, y_gap=3 if pad else 0, fill=0x5A)
    planes = s.planes([torch.from_numpy(b) for b in s.bufs])
    f = YuvFrames.nv12(*planes, width=W) if layout == "nv12" else YuvFrames.i420(*planes, width=W)
    return f, yc.to_rgb(y, u, v, yc.TABLE["bt601", False]), s


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_encode_frames_on_yuv_equals_encode_frames_on_the_rgb_it_converts_to(layout):
    eng = YuvEngine(N=5)
    f, rgb, s = video(40, layout)
    wi, gi = {}, {}
    want = encode.encode_frames_with(eng, rgb, 4, 4, [1, 2, 3], frame_cap=30, info=wi)
    eng.asked = []
    got = encode.encode_frames_with(eng, f, 4, 4, [1, 2, 3], frame_cap=30, info=gi)
    assert torch.equal(got, want) and gi == wi and gi["frames_in"] == 40 and gi["frames_resized"] == 30
    kept = encode.frame_indices(eng.cfg, 40, 4, 30)
    assert eng.asked == [kept] and eng.bytes_uploaded == 30 * (H * W + 2 * (H // 2) * (W // 2))
    # the frames a1 drops and all padding overwritten: the same tokens; a kept frame does count
    for fill in (0xFF, 0x00):
        for b, frame in zip(s.bufs, (s.y_frame, s.c_frame, s.c_frame)):
            for t in range(40):
                if t not in kept:
                    b[t * frame:(t + 1) * frame] = fill
        assert torch.equal(encode.encode_frames_with(eng, f, 4, 4, [1, 2, 3], frame_cap=30), want)
    s.bufs[0][kept[3] * s.y_frame] ^= 0x80
    assert not torch.equal(encode.encode_frames_with(eng, f, 4, 4, [1, 2, 3], frame_cap=30), want)


def test_prompts_export_and_image_forms_take_a_yuvframes():
    eng = YuvEngine(K=3, H=8, N=5, max_len=400, max_num_segments=6)
    f, rgb, _ = video(40)
    prompts = [dict(budget_text_len=4, n_text_tokens=4, prompt_ids=[5]),
               dict(budget_text_len=4, n_text_tokens=30, prompt_ids=[7, 8, 9, 10])]
    want = encode.encode_frames_prompts_with(eng, rgb, prompts, frame_cap=30, pad_fraction=1.0)
    got = encode.encode_frames_prompts_with(eng, f, prompts, frame_cap=30, pad_fraction=1.0)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    eng = YuvEngine(N=5)
    a, b = encode.export_features_from_frames_with(eng, f, slab=16), encode.export_features_from_frames_with(eng, rgb, slab=16)
    assert torch.equal(a.siglip, b.siglip) and torch.equal(a.dino, b.dino) and a.image_size == b.image_size == SIZE and a.frames == 40
    i1, i2 = {}, {}
    assert torch.equal(encode.encode_frames_with(eng, f[2:3], None, 4, None, info=i1, image=True),
                       encode.encode_frames_with(eng, rgb[2:3], None, 4, None, info=i2, image=True)) and i1 == i2
    with pytest.raises(ValueError, match="one frame"):
        encode.encode_frames_with(eng, f, None, 4, None, image=True)


# ------------------------------------------------------------------------------------------------ the mixin
class YuvMixinEngine(_YuvFrames, FeatureMixinEngine):
    def encode_frames(self, frames, *a, **kw):
        self.entered = getattr(self, "entered", []) + [type(frames).__name__]
        return encode.encode_frames_with(self, frames, *a, **kw)


def test_mixin_hands_yuvframes_to_encode_frames():
    (f1, rgb1, _), (f2, rgb2, _) = video(90, "nv12"), video(30, "i420", seed=9, pad=False)
    lm = feature_lm(tdc_frame_inputs=True)
    eng = lm.get_model()._tdc_encoder = YuvMixinEngine(K=3, H=8)
    want = call(lm, [[torch.from_numpy(rgb1), torch.from_numpy(rgb2)], None], 2, [[1, 2], [3, 4, 5]])
    eng.entered = []
    same_tuple(call(lm, [[f1, f2], None], 2, [[1, 2], [3, 4, 5]]), want)
    assert eng.entered == ["YuvFrames", "YuvFrames"] and eng.kinds[-2:] == ["yuv", "yuv"]
    # single images: images[0] itself is a YuvFrames, sliced per sample
    want_im = call(lm, [torch.from_numpy(rgb2[:3]), None], 3)
    eng.entered = []
    same_tuple(call(lm, [f2[:3], None], 3), want_im)
    assert eng.entered == ["YuvFrames"] * 3


@pytest.mark.parametrize("other,v", [("tdc_feature_inputs", True), ("tdc_shard_frames", True), ("tdc_batch_frames", 512),
                                     ("tdc_shard_cache_bytes", 1 << 30), ("tdc_batch_prompts", 4)])
def test_forbidden_combinations_still_raise_before_any_engine_call(other, v):
    lm = feature_lm(tdc_frame_inputs=True, **{other: v})
    lm.get_model()._tdc_encoder = Untouchable()
    with pytest.raises(ValueError) as ei:
        call(lm, [[video(30)[0]], None])
    assert "tdc_frame_inputs" in str(ei.value) and other in str(ei.value)


# ------------------------------------------------------------------------------------------------ host-side checks of the funnel
def test_preprocess_selected_checks_a_yuvframes_on_the_host_before_any_launch():
    f = video(6)[0]
    towers = (dict(R=2, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)),) * 2
    for idx in ([0, 6], [-1, 2], [2, 1], []):
        with pytest.raises(ValueError, match="idx"):
            preprocess.preprocess_selected(f, idx, towers)       # no GPU here: raised before one would be needed
    with pytest.raises(ValueError, match="slab"):
        preprocess.preprocess_selected(f, None, towers, slab=0)
    with pytest.raises(ValueError, match="float16"):
        preprocess.preprocess_selected(f, None, towers, dtype=torch.float32)
