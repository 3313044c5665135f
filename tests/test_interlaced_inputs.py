"""CPU: encode from interlaced video.  The numpy restatement of the field rebuild
(tests/interlace_cases.py) against exact rational arithmetic on every input the formula can see, and the host logic of
preprocess.Interlaced: its refusals, shapes, slicing, nesting with Oriented, and the field views of every wrapped kind and
layout - the same object over row-sliced planes of the same memory."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
import interlace_cases as ic
from tdc_video_amd import encode, lib, ops, preprocess

Interlaced, Oriented, RgbFrames, YuvFrames = preprocess.Interlaced, preprocess.Oriented, preprocess.RgbFrames, preprocess.YuvFrames


# ------------------------------------------------------------------------------------------------ the definition
def exact_linear(a, b):
    """(a + b + 1) >> 1 as the rounded-half-up mean, in rationals"""
    return int((Fraction(a + b, 2) + Fraction(1, 2)).__floor__())


def exact_cubic(s1, s2):
    """the (-1, 9, 9, -1) / 16 filter on the sums s1 = F[m] + F[m+1], s2 = F[m-1] + F[m+2]: rounded half up, clipped"""
    return min(max(int((Fraction(9 * s1 - s2, 16) + Fraction(1, 2)).__floor__()), 0), 255)


def test_linear_restatement_on_all_65536_pairs():
    F = ic.linear_pairs()
    row = ic.rebuild(F, 0, "linear")[0, 1].reshape(-1)[:65536]
    want = np.array([exact_linear(j >> 8, j & 255) for j in range(65536)], np.uint8)
    assert np.array_equal(row, want)
    a, b = np.arange(65536) >> 8, np.arange(65536) & 255          # and in int64, without the rationals
    assert np.array_equal(row, ((a + b + 1) // 2).astype(np.uint8))


def test_cubic_restatement_on_all_511_x_511_pairs_of_sums():
    F = ic.cubic_pairs()
    assert F.shape == (ic.CUBIC_FRAMES, 4, ic.CUBIC_W, 3) and F.shape[2] <= 65535
    s1, s2 = ic.cubic_sums()
    flat = F.astype(np.int64).transpose(1, 0, 2, 3).reshape(4, -1)
    assert np.array_equal(flat[1] + flat[2], s1) and np.array_equal(flat[0] + flat[3], s2)        # the frames hold what they claim
    pairs = set(zip(s1[:511 * 511].tolist(), s2[:511 * 511].tolist()))
    assert len(pairs) == 511 * 511 and min(pairs) == (0, 0) and max(pairs) == (510, 510)
    got = ic.rebuild(F, 0, "cubic")[:, 3].reshape(-1)
    table = {}
    want = np.array([table.setdefault(p, exact_cubic(*p)) for p in zip(s1.tolist(), s2.tolist())], np.uint8)
    assert np.array_equal(got, want)
    floor_div = np.clip((9 * s1 - s2 + 8) // 16, 0, 255)           # int64 floor division: the same everywhere
    assert np.array_equal(got, floor_div.astype(np.uint8))
    assert got.min() == 0 and got.max() == 255 and (9 * s1 - s2 + 8).min() == -502 and (9 * s1 - s2 + 8).max() == 4598


@pytest.mark.parametrize("fill", ic.FILLS)
@pytest.mark.parametrize("parity", [0, 1])
def test_restatement_keeps_the_field_and_clamps_at_both_ends(parity, fill):
    for Hf in (1, 2, 3, 7):
        F = ic.random_fields(2, Hf, 5)
        O = ic.rebuild(F, parity, fill)
        assert O.shape == (2, 2 * Hf, 5, 3) and O.dtype == np.uint8 and O.flags["C_CONTIGUOUS"]
        assert np.array_equal(O[:, parity::2], F)                 # the kept rows: exact copies
        made = O[:, 1 - parity::2].astype(int)
        f = F.astype(int)
        for k in range(Hf):                                        # the made rows, tap by tap in Python integers
            m = k - parity
            t = [f[:, min(max(i, 0), Hf - 1)] for i in (m - 1, m, m + 1, m + 2)]
            want = (t[1] + t[2] + 1) // 2 if fill == "linear" else np.clip((9 * (t[1] + t[2]) - t[0] - t[3] + 8) // 16, 0, 255)
            assert np.array_equal(made[:, k], want), (Hf, k)
    for v in (0, 1, 127, 254, 255):                                # a constant column stays constant
        assert np.array_equal(ic.rebuild(ic.constant(v), parity, fill), np.full((2, 10, 7, 3), v, np.uint8))
    if fill == "cubic":
        O = ic.rebuild(ic.alternating(), parity, fill)[:, 1 - parity::2]
        assert O.min() == 0 and O.max() == 255 and set(np.unique(O[:2, 2:-2])) == {128}   # 0 / 255 rows: (9 * 255 - 255 + 8) >> 4


def test_field_views_of_the_layouts_in_numpy():
    top, bottom = ic.random_fields(2, 3, 4, seed=1), ic.random_fields(2, 3, 4, seed=2)
    for layout in ic.LAYOUTS:
        S = ic.weave(top, bottom, layout)
        assert S.shape == (2, 6, 4, 3)
        assert np.array_equal(ic.field_of(S, 0, layout), top) and np.array_equal(ic.field_of(S, 1, layout), bottom)
    assert np.array_equal(ic.weave(top, bottom, "interleaved")[:, 0::2], top)
    assert np.array_equal(ic.weave(top, bottom, "sequential_tb")[:, :3], top)
    assert np.array_equal(ic.weave(top, bottom, "sequential_bt")[:, :3], bottom)


# ------------------------------------------------------------------------------------------------ the container
def _np_ptr(a):
    return a.__array_interface__["data"][0]


def test_interlaced_describes_frames_without_copying():
    a = ic.random_fields(6, 8, 6)                                   # as frames: [6, 8, 6, 3]
    t = torch.from_numpy(a)
    for field in ic.FIELDS:
        for fill in ic.FILLS:
            for layout in ic.LAYOUTS:
                x = Interlaced(t, field, fill, layout)
                p = ic.FIELDS.index(field)
                assert x.shape == (6, 8, 6, 3) and x.frames.data_ptr() == t.data_ptr() and not x.is_cuda
                assert (x.field, x.fill, x.layout, x.parity) == (field, fill, layout, p)
                s = x[2:5]
                assert s.shape == (3, 8, 6, 3) and (s.field, s.fill, s.layout) == (field, fill, layout)
                assert s.frames.data_ptr() == t[2:5].data_ptr() and x[1:2].shape[0] == 1
                f = x.field_frames()
                rows = ic.field_index(8, p, layout)
                assert tuple(f.shape) == (6, 4, 6, 3) and f.data_ptr() == t.data_ptr() + int(rows[0]) * 18
                assert np.array_equal(f.numpy(), ic.field_of(a, p, layout))
                assert f.stride(1) == (36 if layout == "interleaved" else 18) and f.stride(2) == 3
                assert encode.frames_size(x) == (6, (8, 6)) and encode.FrameSource(x).image_size == (8, 6)
    assert Interlaced(a).frames.data_ptr() == _np_ptr(a)             # a numpy array, not copied either
    d = Interlaced(a)
    assert (d.field, d.fill, d.layout) == ("top", "linear", "interleaved")
    with pytest.raises(TypeError, match="slice"):
        d[0]
    with pytest.raises(TypeError, match="slice"):
        d[::2]


def test_is_interlaced_is_by_members_and_tells_the_kinds_apart():
    a = ic.random_fields(2, 4, 6)
    x = Interlaced(a)
    o = Oriented(a, 90)
    r = RgbFrames(a, "hwc", "bgr")
    y = YuvFrames.nv12(np.zeros((2, 4, 6), np.uint8), np.zeros((2, 2, 6), np.uint8))
    assert preprocess.is_interlaced(x) and not any(preprocess.is_interlaced(v) for v in (a, torch.from_numpy(a), o, r, y, None))
    assert not preprocess.is_oriented(x) and not preprocess.is_rgb_frames(x) and not preprocess.is_yuv_frames(x)

    class Double:                                                   # the package imported under another name: no isinstance
        frames, field, fill, layout, parity, shape = a, "top", "linear", "interleaved", 0, (2, 4, 6, 3)
    assert preprocess.is_interlaced(Double())


def test_nesting_with_oriented():
    a = ic.random_fields(3, 4, 6)
    x = Interlaced(a, "bottom", "cubic")
    o = Oriented(x, 90, True)
    assert o.shape == (3, 6, 4, 3) and preprocess.is_interlaced(o.frames) and o.frames.frames.data_ptr() == _np_ptr(a)
    assert o[1:3].shape == (2, 6, 4, 3) and o[1:3].frames.fill == "cubic" and not o.is_cuda
    assert encode.FrameSource(o).image_size == (6, 4)
    with pytest.raises(ValueError, match="Oriented"):
        Interlaced(Oriented(a, 90))
    with pytest.raises(ValueError, match="Oriented"):
        Interlaced(Oriented(a))                                      # the identity too: one rule
    with pytest.raises(ValueError, match="Interlaced already"):
        Interlaced(x)
    with pytest.raises(ValueError):
        RgbFrames(x)


def test_refusals():
    a = ic.random_fields(2, 4, 6)
    for kw in (dict(field="even"), dict(field=0), dict(fill="nearest"), dict(fill=1), dict(layout="alternate"), dict(layout=None)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Interlaced(a, **kw)
    with pytest.raises(ValueError, match="even"):
        Interlaced(ic.random_fields(2, 5, 6))                        # H odd
    with pytest.raises(ValueError, match="even"):
        Interlaced(RgbFrames.chw(np.zeros((2, 3, 5, 6), np.uint8)))
    with pytest.raises(ValueError, match="uint8"):
        Interlaced(a.astype(np.float32))
    y6, uv6 = np.zeros((2, 6, 8), np.uint8), np.zeros((2, 3, 8), np.uint8)
    with pytest.raises(ValueError, match="multiple of 4"):
        Interlaced(YuvFrames.nv12(y6, uv6))                          # 4:2:0 at H % 4 == 2: chroma fields of 2 and 1 rows
    assert Interlaced(YuvFrames.nv12(y6, np.zeros((2, 6, 8), np.uint8), subsampling="422")).shape == (2, 6, 8, 3)     # 4:2:2: H even is enough
    assert Interlaced(YuvFrames.yuy2(np.zeros((2, 6, 16), np.uint8))).shape == (2, 6, 8, 3)
    y8, uv8 = np.zeros((2, 8, 8), np.uint8), np.zeros((2, 4, 8), np.uint8)
    with pytest.raises(ValueError, match="linear"):
        Interlaced(YuvFrames.nv12(y8, uv8, upsample="linear"))       # interpolated 4:2:0 chroma with per-field siting: out of scope
    assert Interlaced(YuvFrames.nv12(y8, uv8)).shape == (2, 8, 8, 3)
    ok = Interlaced(YuvFrames.nv12(y8, np.zeros((2, 8, 8), np.uint8), subsampling="422", upsample="linear"))      # 4:2:2: horizontal only
    assert ok.field_frames().upsample == "linear" and ok.field_frames().interpolates
    assert Interlaced(YuvFrames.yuy2(np.zeros((2, 6, 16), np.uint8), upsample="linear")).field_frames().interpolates


# ------------------------------------------------------------------------------------------------ the field views
@pytest.mark.parametrize("layout", ic.LAYOUTS)
@pytest.mark.parametrize("parity", [0, 1])
def test_field_views_share_memory_and_keep_every_parameter(parity, layout):
    rng = np.random.RandomState(3)
    field = ic.FIELDS[parity]

    def first(n):
        return int(ic.field_index(n, parity, layout)[0])

    # RgbFrames: pitched BGRA rows, and channel-first planes
    bgra = rng.randint(0, 256, (3, 8, 10, 4)).astype(np.uint8)
    r = RgbFrames(bgra[:, :, :6], "hwc", "bgra")
    f = Interlaced(r, field, "linear", layout).field_frames()
    assert preprocess.is_rgb_frames(f) and f.shape == (3, 4, 6, 3) and (f.layout, f.order, f.index) == ("hwc", "bgra", (2, 1, 0))
    assert f.data.data_ptr() == _np_ptr(bgra) + first(8) * 40 and np.array_equal(f.data.numpy(), ic.field_of(bgra[:, :, :6], parity, layout))
    chw = rng.randint(0, 256, (3, 3, 8, 6)).astype(np.uint8)
    f = Interlaced(RgbFrames.chw(chw, "rgb"), field, "cubic", layout).field_frames()
    assert f.shape == (3, 4, 6, 3) and f.layout == "chw" and f.data.data_ptr() == _np_ptr(chw) + first(8) * 6
    assert np.array_equal(f.data.numpy(), ic.field_of(chw, parity, layout, axis=2))
    assert f[1:2].data.data_ptr() == f.data[1:2].data_ptr()
    # an identity RgbFrames: the field of its tensor
    hwc = rng.randint(0, 256, (3, 8, 6, 3)).astype(np.uint8)
    f = Interlaced(RgbFrames(hwc), field, "linear", layout).field_frames()
    assert f.is_identity and f.data.data_ptr() == _np_ptr(hwc) + first(8) * 18
    # NV12 with a pitch: luma and chroma split the same way, plane by plane
    y, uv = rng.randint(0, 256, (3, 8, 16)).astype(np.uint8), rng.randint(0, 256, (3, 4, 16)).astype(np.uint8)
    src = YuvFrames.nv12(y, uv, width=10, matrix="bt709", full_range=True, siting="center")
    f = Interlaced(src, field, "linear", layout).field_frames()
    assert preprocess.is_yuv_frames(f) and f.shape == (3, 4, 10, 3) and f.is_420_8bit and f.c_step == 2
    assert (f.matrix, f.full_range, f.siting, f.upsample, f.coef) == ("bt709", True, "center", "replicate", src.coef)
    assert f.y.data_ptr() == _np_ptr(y) + first(8) * 16 and f.chroma[0].data_ptr() == _np_ptr(uv) + first(4) * 16
    got = [p.numpy() for p in f.planes()]
    assert np.array_equal(got[0], ic.field_of(y, parity, layout)[:, :, :10]) and np.array_equal(got[1], ic.field_of(uv, parity, layout)[:, :, :10])
    # I420 10-bit 4:2:2 PQ: three planes, chroma at full height
    y = rng.randint(0, 1024, (2, 4, 6)).astype(np.uint16)
    u, v = rng.randint(0, 1024, (2, 4, 3)).astype(np.uint16), rng.randint(0, 1024, (2, 4, 3)).astype(np.uint16)
    src = YuvFrames.i420(y, u, v, matrix="bt2020", bits=10, subsampling="422", transfer="pq", peak_nits=600.0, sdr_white=150.0)
    f = Interlaced(src, field, "cubic", layout).field_frames()
    assert f.shape == (2, 2, 6, 3) and (f.bits, f.subsampling, f.transfer, f.peak_nits, f.sdr_white, f.primaries) == (10, "422", "pq", 600.0, 150.0, "bt2020")
    assert f.hdr == src.hdr and f.coef == src.coef and not f.msb_aligned
    assert [p.data_ptr() for p in (f.y,) + f.chroma] == [_np_ptr(y) + first(4) * 12, _np_ptr(u) + first(4) * 6, _np_ptr(v) + first(4) * 6]
    assert np.array_equal(f.chroma[1].numpy().view(np.uint16), ic.field_of(v, parity, layout))
    # packed: YUY2 and v210
    yuy2 = rng.randint(0, 256, (2, 6, 20)).astype(np.uint8)
    src = YuvFrames.yuy2(yuy2, width=8, matrix="bt709")
    f = Interlaced(src, field, "linear", layout).field_frames()
    assert type(f).__name__ == "PackedYuvFrames" and f.shape == (2, 3, 8, 3) and (f.fmt, f.name, f.matrix) == ("yuyv", "yuyv", "bt709")
    assert f.y.data_ptr() == _np_ptr(yuy2) + first(6) * 20 and np.array_equal(f.planes()[0].numpy(), ic.field_of(yuy2, parity, layout)[:, :, :16])
    v210 = rng.randint(0, 1 << 30, (2, 4, 32)).astype(np.uint32)
    src = YuvFrames.v210(v210, 12, transfer="hlg", matrix="bt2020")
    f = Interlaced(src, field, "linear", layout).field_frames()
    assert f.shape == (2, 2, 12, 3) and (f.fmt, f.bits, f.transfer) == ("v210", 10, "hlg") and f.y.data_ptr() == _np_ptr(v210) + first(4) * 128
    assert np.array_equal(f.planes()[0].numpy().view(np.uint32), ic.field_of(v210, parity, layout)[:, :, :8])


def test_field_rows_of_preprocess_equal_the_restated_index():
    for n in (2, 4, 6, 10):
        for layout in ic.LAYOUTS:
            for p in (0, 1):
                assert np.array_equal(np.arange(n)[preprocess.field_rows(n, p, layout)], ic.field_index(n, p, layout))
    assert preprocess.FIELDS == ic.FIELDS and preprocess.FIELD_LAYOUTS == ic.LAYOUTS and ops.FIELD_FILLS == {"linear": 0, "cubic": 1}
    assert sorted(ops.FIELD_FILLS) == sorted(ic.FILLS)


def test_which_field_views_the_kernel_can_read_in_place():
    f = torch.from_numpy(ic.random_fields(3, 8, 6))
    chw = f.permute(0, 3, 1, 2).contiguous()
    rgba = torch.cat([f, f[..., :1]], 3)
    for layout in ic.LAYOUTS:
        for p in (0, 1):
            rows = preprocess.field_rows(8, p, layout)
            assert ops.field_pixels_dense(f[:, rows]) and ops.field_pixels_dense(f[1:2, rows]) and ops.field_pixels_dense(f[:, rows, 1:5])
            assert not ops.field_pixels_dense(chw.permute(0, 2, 3, 1)[:, rows])      # a pixel's bytes a plane apart
            assert not ops.field_pixels_dense(rgba[..., :3][:, rows])                # pixels four bytes apart
    assert ops.field_pixels_dense(rgba[:, :, :1, :3])                                 # one pixel per row: no pixel stride to speak of
    assert preprocess.check_frames(chw.permute(0, 2, 3, 1)) is not None and Interlaced(rgba[..., :3]).shape == (3, 8, 6, 3)


def test_the_entry_point_is_declared():
    assert "tdc_field_to_frame" in lib.SIGNATURES and len(lib.SIGNATURES["tdc_field_to_frame"][1]) == 10
