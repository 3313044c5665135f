"""CPU: encode from packed YUV surfaces.  The layouts of yuv_packed_cases against the issue's worked
vectors and their own inverse, junk invariance, the YuvFrames.packed container (shapes, default widths, slicing, planes() cut
to the read set, every refusal), the host gather of a packed surface (kept frames only, the stated byte count), an Oriented
around one, and the planar constructors as they were."""
import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
import yuv_cases as yc
import yuv_hibit_cases as hc
import yuv_packed_cases as pc
from tdc_video_amd import encode, ops, preprocess
from test_features import Untouchable, feature_lm
from test_frame_inputs import call

YuvFrames = preprocess.YuvFrames
WIDTHS = (1, 2, 5, 6, 7, 8, 24, 50)
EVERY = [(f, bits, msb) for f in pc.FORMATS for bits, msb in pc.DEPTHS[f]]


# ------------------------------------------------------------------------------------------------ the layouts
def test_the_v210_worked_vector():
    cb, y, cr = np.array([0x101, 0x102, 0x103]), np.arange(0x201, 0x207), np.array([0x301, 0x302, 0x303])
    rows = pc.pack_rows(y.reshape(1, 1, 6), cb.reshape(1, 1, 3), cr.reshape(1, 1, 3), "v210", 10)
    assert rows.dtype == np.uint32 and rows.reshape(-1).tolist() == [0x30180501, 0x20340a02, 0x10381302, 0x206c0e05]
    for junk in (0, 3 << 30):                                     # bits 30-31 are ignored
        Y, U, V = pc.unpack(rows | np.uint32(junk), "v210", 10, False, 6)
        assert Y.reshape(-1).tolist() == y.tolist() and U.reshape(-1).tolist() == cb.tolist() and V.reshape(-1).tolist() == cr.tolist()


def test_the_y410_worked_vector():
    one = lambda x: np.array([[[x]]])
    rows = pc.pack_rows(one(0x201), one(0x101), one(0x301), "y410", 10)
    assert rows.dtype == np.uint32 and int(rows[0, 0, 0]) | 3 << 30 == 0xf0180501
    Y, U, V = pc.unpack(np.array([[[0xf0180501]]], np.uint32), "y410", 10, False, 1)
    assert (int(U[0, 0, 0]), int(Y[0, 0, 0]), int(V[0, 0, 0])) == (0x101, 0x201, 0x301)


def test_the_byte_orders_are_what_the_names_spell():
    y, u, v = np.array([[[1, 2]]], np.uint8), np.array([[[3]]], np.uint8), np.array([[[4]]], np.uint8)
    want = {"yuyv": [1, 3, 2, 4], "yvyu": [1, 4, 2, 3], "uyvy": [3, 1, 4, 2], "vyuy": [4, 1, 3, 2]}
    for fmt, row in want.items():
        assert pc.pack_rows(y, u, v, fmt, 8).reshape(-1).tolist() == row
    assert (pc.pack_rows(y, u, v, "y210", 10, True).reshape(-1) >> 6).tolist() == want["yuyv"]
    assert pc.pack_rows(y, u, v, "y210", 12, False).reshape(-1).tolist() == want["yuyv"]
    y1 = y[:, :, :1]
    assert pc.pack_rows(y1, u, v, "vuya", 8).reshape(-1).tolist() == [4, 3, 1, 0]
    assert pc.pack_rows(y1, u, v, "ayuv", 8).reshape(-1).tolist() == [0, 1, 3, 4]
    assert (pc.pack_rows(y1, u, v, "y416", 12, True).reshape(-1) >> 4).tolist() == [3, 1, 4, 0]


@pytest.mark.parametrize("fmt,bits,msb", EVERY)
def test_unpack_inverts_pack_and_ignores_the_junk(fmt, bits, msb):
    for W in WIDTHS:
        y, u, v = pc.random_planes(2, 3, W, fmt, bits)
        G, P = pc.geometry(fmt)
        assert pc.row_words(fmt, W) == -(-W // P) * G
        surfaces = [pc.pack(y, u, v, fmt, bits, msb, pitch=pc.row_words(fmt, W) + 3, gap=5, fill=fill, junk=junk)
                    for fill, junk in ((0x00, None), (0xFF, 1), (0xA5, 2))]
        for s in surfaces:
            for got, want in zip(pc.unpack(s.rows(), fmt, bits, msb, W), (y, u, v)):
                assert got.dtype == want.dtype and np.array_equal(got, want), (W, s.pitch)
        ignores = fmt in ("y410", "v210", "vuya", "ayuv", "y416", "y210") or W % P
        assert np.array_equal(surfaces[1].rows(), surfaces[2].rows()) == (not ignores), W
        # everything outside the read set holds the fill
        outside = np.ones(surfaces[1].buf.shape, bool)
        b = outside.itemsize
        np.lib.stride_tricks.as_strided(outside, (2, 3, s.row), (s.frame * b, s.pitch * b, b))[...] = False
        assert np.all(surfaces[1].buf.view(np.uint8).reshape(-1, surfaces[1].buf.itemsize)[outside] == 0xFF)


# ------------------------------------------------------------------------------------------------ the container
def frames_over(s, flat=None, **kw):
    """the YuvFrames a caller would build over the whole-pitch surface of s"""
    return YuvFrames.packed(s.plane(s.tensor() if flat is None else flat), s.fmt, width=s.W, bits=s.bits, msb_aligned=s.msb, **kw)


@pytest.mark.parametrize("fmt,bits,msb", EVERY)
def test_packed_describes_a_surface_without_copying(fmt, bits, msb):
    T, H, W = 5, 4, 7
    y, u, v = pc.random_planes(T, H, W, fmt, bits)
    row = pc.row_words(fmt, W)
    s = pc.pack(y, u, v, fmt, bits, msb, pitch=row + 6, gap=9, fill=0x5A, junk=1)
    flat = s.tensor()
    f = frames_over(s, flat, matrix="bt709")
    G, P = pc.geometry(fmt)
    assert preprocess.is_yuv_frames(f) and isinstance(f, YuvFrames) and f.shape == (T, H, W, 3) and not f.is_cuda
    assert f.y.device.type == "cpu" and f.y.data_ptr() == flat.data_ptr() and f.coef == hc.TABLE["bt709", False, bits]
    assert (f.bits, f.msb_aligned, f.subsampling, f.chroma) == (bits, msb, pc.sub(fmt), ())
    assert encode.frames_size(f) == (T, (H, W)) and encode.FrameSource(f).T0 == T
    planes = f.planes()
    assert len(planes) == 1 and tuple(planes[0].shape) == (T, H, row) and planes[0].data_ptr() == flat.data_ptr()
    assert np.array_equal(planes[0].numpy().view(s.dtype), s.rows())
    g = f[1:3]
    assert isinstance(g, YuvFrames) and g.shape == (2, H, W, 3) and g.y.data_ptr() == s.plane(flat)[1].data_ptr()
    assert (g.fmt, g.bits, g.msb_aligned, g.matrix, g.coef) == (f.fmt, bits, msb, "bt709", f.coef)
    with pytest.raises(TypeError):
        f[0]
    # the default width: the row's whole groups; v210 has none
    if fmt == "v210":
        with pytest.raises(ValueError, match="width"):
            YuvFrames.packed(s.plane(flat), fmt)
    else:
        d = YuvFrames.packed(s.plane(flat), fmt, bits=bits, msb_aligned=msb)
        assert d.shape == (T, H, (row + 6) // G * P, 3)
    # numpy words are taken over the same memory
    n = YuvFrames.packed(s.rows(), fmt, width=W, bits=bits, msb_aligned=msb)
    assert n.y.data_ptr() == s.buf.ctypes.data and n.y.dtype == {1: torch.uint8, 2: torch.int16, 4: torch.int32}[s.buf.itemsize]
    assert tuple(n.y.stride()) == (s.frame, s.pitch, 1)
    wide = getattr(torch, "uint%d" % (8 * s.buf.itemsize), None)
    if s.buf.itemsize > 1 and wide is not None:
        t = YuvFrames.packed(s.plane(flat).view(wide), fmt, width=W, bits=bits, msb_aligned=msb)
        assert t.y.dtype == flat.dtype and t.y.data_ptr() == flat.data_ptr()
    # an Oriented around it has the upright shape
    o = preprocess.Oriented(f, rotate=90)
    assert o.shape == (T, W, H, 3) and preprocess.Oriented(f, rotate=180, hflip=True).shape == (T, H, W, 3) and o[1:2].shape == (1, W, H, 3)


def test_the_named_forms_and_the_names_taken():
    b = np.zeros((2, 3, 16), np.uint8)
    w = np.zeros((2, 3, 16), np.uint16)
    d = np.zeros((2, 3, 16), np.uint32)
    assert (YuvFrames.yuy2(b).fmt, YuvFrames.uyvy(b).fmt, YuvFrames.ayuv(b).fmt) == ("yuyv", "uyvy", "vuya")
    assert YuvFrames.yuy2(b).shape == (2, 3, 8, 3) and YuvFrames.ayuv(b).shape == (2, 3, 4, 3)
    f = YuvFrames.y210(w)
    assert (f.fmt, f.bits, f.msb_aligned, f.shape) == ("y210", 10, True, (2, 3, 8, 3))
    f = YuvFrames.y210(w, bits=12, msb_aligned=False, matrix="bt2020", transfer="pq")
    assert (f.bits, f.msb_aligned, f.transfer) == (12, False, "pq") and f.hdr is not None
    f = YuvFrames.y410(d)
    assert (f.fmt, f.bits, f.msb_aligned, f.shape) == ("y410", 10, False, (2, 3, 16, 3))
    f = YuvFrames.v210(d, 23, matrix="bt2020", transfer="hlg")
    assert (f.fmt, f.bits, f.shape, f.subsampling) == ("v210", 10, (2, 3, 23, 3), "422") and f.planes()[0].shape == (2, 3, 16)
    assert YuvFrames.v210(d, 13).planes()[0].shape == (2, 3, 12)
    for name, (fmt, bits) in {"yuy2": ("yuyv", 8), "vuyx": ("vuya", 8), "y212": ("y210", 12), "y412": ("y416", 12)}.items():
        f = YuvFrames.packed(b if bits == 8 else w, name)
        assert (f.fmt, f.bits) == (fmt, bits)
    for name in ("y216", "y416"):
        assert YuvFrames.packed(w, name, bits=10).bits == 10 and YuvFrames.packed(w, name, bits=12, msb_aligned=False).bits == 12
        with pytest.raises(ValueError, match="bits"):
            YuvFrames.packed(w, name)


def test_packed_refusals_name_the_argument():
    b = np.zeros((2, 3, 16), np.uint8)
    w = np.zeros((2, 3, 16), np.uint16)
    d = np.zeros((2, 3, 16), np.uint32)
    bad = [("data", lambda: YuvFrames.yuy2(w)),                                              # the word type against the format
           ("data", lambda: YuvFrames.y210(b)),
           ("data", lambda: YuvFrames.y410(w)),
           ("data", lambda: YuvFrames.v210(b, 6)),
           ("data", lambda: YuvFrames.y410(d.astype(np.int64))),
           ("data", lambda: YuvFrames.yuy2(torch.zeros(2, 3, 16, dtype=torch.int16))),
           ("data", lambda: YuvFrames.y210(torch.zeros(2, 3, 16, dtype=torch.uint8))),
           ("data", lambda: YuvFrames.yuy2(b[0])),                                           # rank
           ("data", lambda: YuvFrames.yuy2(np.zeros((2, 3, 32), np.uint8)[:, :, ::2])),      # last dimension not dense
           ("data", lambda: YuvFrames.yuy2([[1, 2, 3, 4]])),
           ("fmt", lambda: YuvFrames.packed(b, "yuv2")),
           ("fmt", lambda: YuvFrames.packed(b, "ayuv64")),
           ("bits", lambda: YuvFrames.packed(b, "yuyv", bits=10)),
           ("bits", lambda: YuvFrames.packed(w, "y210", bits=8)),
           ("bits", lambda: YuvFrames.packed(w, "y210", bits=16)),
           ("bits", lambda: YuvFrames.packed(w, "y212", bits=10)),
           ("bits", lambda: YuvFrames.packed(d, "y410", bits=12)),
           ("bits", lambda: YuvFrames.packed(d, "v210", width=6, bits=12)),
           ("bits", lambda: YuvFrames.packed(w, "y416", bits=True)),
           ("msb_aligned", lambda: YuvFrames.packed(b, "yuyv", msb_aligned=True)),
           ("msb_aligned", lambda: YuvFrames.packed(d, "y410", msb_aligned=True)),
           ("msb_aligned", lambda: YuvFrames.packed(d, "v210", width=6, msb_aligned=True)),
           ("msb_aligned", lambda: YuvFrames.packed(w, "y210", msb_aligned=1)),
           ("width", lambda: YuvFrames.yuy2(b, width=9)),                                    # a row shorter than the width's groups
           ("width", lambda: YuvFrames.ayuv(b, width=5)),
           ("width", lambda: YuvFrames.y210(w, width=9)),
           ("width", lambda: YuvFrames.y410(d, width=17)),
           ("width", lambda: YuvFrames.v210(d, 25)),
           ("width", lambda: YuvFrames.v210(d, 0)),
           ("width", lambda: YuvFrames.packed(d, "v210")),
           ("matrix", lambda: YuvFrames.yuy2(b, matrix="bt2020")),                           # bt2020 at 8 bits
           ("matrix", lambda: YuvFrames.ayuv(b, matrix="bt2020")),
           ("matrix", lambda: YuvFrames.y210(w, matrix="bt470")),
           ("transfer", lambda: YuvFrames.yuy2(b, transfer="pq")),                           # HDR at 8 bits
           ("transfer", lambda: YuvFrames.ayuv(b, transfer="hlg")),
           ("transfer", lambda: YuvFrames.y210(w, transfer="gamma")),
           ("full_range", lambda: YuvFrames.y410(d, full_range=1)),
           ("primaries", lambda: YuvFrames.y410(d, primaries="p3"))]
    for name, make in bad:
        with pytest.raises(ValueError, match=name):
            make()
    # the widest width a row takes, and one past a group boundary that it still takes
    assert YuvFrames.yuy2(b, width=7).planes()[0].shape == (2, 3, 16) and YuvFrames.v210(d, 24).shape == (2, 3, 24, 3)
    assert YuvFrames.y210(w, matrix="bt2020").coef == hc.TABLE["bt2020", False, 10]


def test_ops_refuses_before_the_library_is_asked():
    t = torch.zeros(2, 3, 16, dtype=torch.uint8)
    coef = hc.TABLE["bt709", False, 8]
    for args in ((t, "yuy2", coef, 3, 8, 8, False), (t, "yuyv", coef, 3, 8, 10, False), (t, "yuyv", coef, 3, 8, 8, True),
                 (t, "yuyv", coef, 3, 8, 8, False)):                      # the last: a host tensor
        with pytest.raises(AssertionError):
            ops.yuv_packed_to_rgb(*args)
    assert ops.yuv_packed_words("v210", 7) == 8 and ops.yuv_packed_words("yuyv", 7) == 16 and ops.yuv_packed_words("y410", 7) == 7


def test_the_c_abi_declares_the_packed_entry():
    from tdc_video_amd import lib as L
    assert "tdc_yuv_packed_to_rgb" in L.SIGNATURES
    assert [n for n, _ in L.YuvPacked._fields_] == ["base", "frame", "pitch", "format", "bits", "msb_aligned"]
    assert set(L.YUV_PACKED_FORMATS) == set(pc.FORMATS) == set(ops.YUV_PACKED)
    assert sorted(L.YUV_PACKED_FORMATS.values()) == list(range(10))


# ------------------------------------------------------------------------------------------------ the gather and the byte count
IDX = [0, 2, 3, 7]


@pytest.mark.parametrize("fmt,bits,msb", [("yuyv", 8, False), ("uyvy", 8, False), ("y210", 10, True), ("vuya", 8, False),
                                          ("y410", 10, False), ("y416", 12, False), ("v210", 10, False)])
@pytest.mark.parametrize("h,w", [(4, 6), (3, 5), (2, 24)])
def test_gather_reads_only_the_kept_frames_read_set_and_counts_its_bytes(monkeypatch, fmt, bits, msb, h, w):
    gather = preprocess.gather_planes                             # no GPU here: selected_planes stages in pageable memory
    monkeypatch.setattr(preprocess, "gather_planes", lambda yuv, idx, pin=True: gather(yuv, idx, pin=False))
    y, u, v = pc.random_planes(9, h, w, fmt, bits)
    row = pc.row_words(fmt, w)
    staged = []
    for fill in (0xFF, 0x00):
        s = pc.pack(y, u, v, fmt, bits, msb, pitch=row + 3, gap=7, fill=fill, junk=5)
        for t in range(9):                                        # the dropped frames are poisoned too
            if t not in IDX:
                s.buf[t * s.frame:(t + 1) * s.frame].view(np.uint8)[...] = fill
        f = frames_over(s)
        out, stage = gather(f, IDX, pin=False)
        size = s.buf.itemsize
        assert len(out) == 1 and stage.numel() == len(IDX) * h * row and stage.element_size() == size and stage.is_contiguous()
        for got, want in zip(pc.unpack(out[0].numpy().view(s.dtype), fmt, bits, msb, w), (y, u, v)):
            assert np.array_equal(got, want[IDX])
        staged.append(stage.clone())
        planes, uploaded = preprocess.selected_planes(f, IDX, torch.device("cpu"))
        assert uploaded == len(IDX) * h * row * size
        if w % pc.geometry(fmt)[1] == 0:
            assert uploaded == len(IDX) * h * w * pc.BYTES_PER_PIXEL[fmt]
        assert [tuple(p.shape) for p in planes] == [(len(IDX), h, row)]
        _, uploaded = preprocess.selected_planes(f, None, torch.device("cpu"))
        assert uploaded == 9 * h * row * size
    assert torch.equal(*staged)


def test_the_stated_bytes_per_pixel_at_720_by_1280():
    for fmt, want in (("yuyv", 2), ("v210", 8.0 / 3), ("y210", 4), ("vuya", 4), ("y410", 4)):
        nbytes = ops.yuv_packed_words(fmt, 1280) * ops.YUV_PACKED[fmt][0]
        assert want <= nbytes / 1280.0 < want + 0.01, fmt


# ------------------------------------------------------------------------------------------------ routing
def test_a_packed_surface_issues_one_packed_conversion_and_a_planar_one_what_it_issued(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "yuv420_to_rgb", lambda *a, **k: calls.append("tdc_yuv420_to_rgb"))
    monkeypatch.setattr(ops, "yuv_to_rgb", lambda *a, **k: calls.append("tdc_yuv_to_rgb"))
    monkeypatch.setattr(ops, "yuv_hdr_to_rgb", lambda *a, **k: calls.append("tdc_yuv_hdr_to_rgb"))
    monkeypatch.setattr(ops, "yuv_packed_to_rgb", lambda surface, fmt, coef, H, W, bits, msb_aligned, hdr=None, out=None:
                        calls.append(("tdc_yuv_packed_to_rgb", tuple(surface.shape), fmt, coef, H, W, bits, msb_aligned, hdr is not None)))
    monkeypatch.setattr(preprocess, "hdr_lut", lambda *a: None)
    y, u, v = pc.random_planes(2, 4, 7, "v210", 10)
    s = pc.pack(y, u, v, "v210", 10, pitch=16)
    f = frames_over(s, matrix="bt2020")
    f.to_rgb(list(f.planes()), None)
    g = frames_over(s, matrix="bt2020", transfer="hlg")
    g.to_rgb(list(g.planes()), None)
    assert calls == [("tdc_yuv_packed_to_rgb", (2, 4, 8), "v210", hc.TABLE["bt2020", False, 10], 4, 7, 10, False, False),
                     ("tdc_yuv_packed_to_rgb", (2, 4, 8), "v210", g.coef, 4, 7, 10, False, True)]
    del calls[:]
    y, u, v = yc.random_planes(2, 3, 5)
    p = YuvFrames.i420(y, u, v)
    p.to_rgb(list(p.planes()), None)
    y, u, v = hc.random_planes(2, 3, 5, 10, "422")
    q = YuvFrames.i420(y, u, v, bits=10, subsampling="422")
    q.to_rgb(list(q.planes()), None)
    r = YuvFrames.i420(y, u, v, bits=10, subsampling="422", matrix="bt2020", transfer="pq")
    r.to_rgb(list(r.planes()), None)
    assert calls == ["tdc_yuv420_to_rgb", "tdc_yuv_to_rgb", "tdc_yuv_hdr_to_rgb"]


def test_the_planar_constructors_build_what_they_built():
    y, u, v = yc.random_planes(2, 3, 5)
    f = YuvFrames.i420(y, u, v)
    assert type(f) is YuvFrames and (f.bits, f.msb_aligned, f.subsampling, f.coef, f.is_420_8bit, f.c_step) == \
        (8, False, "420", yc.TABLE["bt601", False], True, 1)
    assert [tuple(p.shape) for p in f.planes()] == [(2, 3, 5), (2, 2, 3), (2, 2, 3)] and type(f[0:1]) is YuvFrames
    y, u, v = hc.random_planes(3, 4, 6, 10)
    uv = np.stack([u, v], -1).reshape(3, 2, 6)
    f = YuvFrames.p010(y, uv, matrix="bt2020")
    assert type(f) is YuvFrames and (f.bits, f.msb_aligned, f.c_step, f.coef) == (10, True, 2, hc.TABLE["bt2020", False, 10])
    assert [tuple(p.shape) for p in f.planes()] == [(3, 4, 6), (3, 2, 6)]
    assert not hasattr(f, "fmt")


def test_preprocess_selected_checks_a_packed_surface_on_the_host_before_any_launch():
    y, u, v = pc.random_planes(6, 4, 6, "yuyv", 8)
    f = frames_over(pc.pack(y, u, v, "yuyv", 8))
    towers = (dict(R=2, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)),) * 2
    for idx in ([0, 6], [-1, 2], [2, 1], []):
        with pytest.raises(ValueError, match="idx"):
            preprocess.preprocess_selected(f, idx, towers)       # no GPU here: raised before one would be needed
    with pytest.raises(ValueError, match="slab"):
        preprocess.preprocess_selected(f, None, towers, slab=0)


@pytest.mark.parametrize("other,v", [("tdc_shard_frames", True), ("tdc_batch_frames", 512), ("tdc_batch_prompts", 4)])
def test_sharded_batched_and_multi_prompt_configs_refuse_a_packed_surface_as_they_refuse_frames(other, v):
    lm = feature_lm(tdc_frame_inputs=True, **{other: v})
    lm.get_model()._tdc_encoder = Untouchable()
    y, u, v_ = pc.random_planes(30, 4, 6, "yuyv", 8)
    with pytest.raises(ValueError) as ei:
        call(lm, [[frames_over(pc.pack(y, u, v_, "yuyv", 8))], None])
    assert "tdc_frame_inputs" in str(ei.value) and other in str(ei.value)
