"""CPU: encode from 10/12-bit and 4:2:2 / 4:4:4 YUV surfaces.  The generalised definition against real
arithmetic for all 18 settings, the coefficient table, the 8-bit 4:2:0 case against section 19's definition, the YuvFrames
container on the new kinds, the host gather of 16-bit planes with pitches, bytes_uploaded, the routing between the two entry
points, and the frames funnel on the engine double of test_frame_inputs."""
import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
import yuv_cases as yc
import yuv_hibit_cases as hc
from tdc_video_amd import encode, ops, preprocess
from test_features import FeatureEngine
from test_frame_inputs import SIZE, _Frames

YuvFrames = preprocess.YuvFrames
H, W = SIZE                                                       # (4, 6): the engine double's frames


# ------------------------------------------------------------------------------------------------ the definition
def chroma_lattice(bits):
    """about 64 x 64 chroma values, the extremes and the values around the middle among them"""
    top = (1 << bits) - 1
    return np.unique(np.concatenate([np.linspace(0, top, 61).round().astype(np.int64), hc.edge_values(bits)]))


@pytest.mark.parametrize("matrix,full_range,bits", hc.SETTINGS)
def test_definition_against_real_arithmetic(matrix, full_range, bits):
    coef = hc.TABLE[matrix, full_range, bits]
    s = bits - 8
    c = chroma_lattice(bits)
    U, V = np.meshgrid(c, c)
    worst, acc = 0, 0
    for y0 in range(0, 1 << bits, 256):
        Yb, Ub, Vb = np.broadcast_arrays(np.arange(y0, y0 + 256)[:, None, None], U[None], V[None])
        got = hc.channels(Yb, Ub, Vb, coef, bits)
        for g, r in zip(got, hc.real_channels(Yb, Ub, Vb, matrix, full_range, bits)):
            want = np.clip(np.floor(r + 0.5), 0, 255)
            worst = max(worst, int(np.abs(g.astype(np.int64) - want.astype(np.int64)).max()))
        acc = max([acc] + [int(np.abs(a).max()) for a in hc.accumulators(Yb, Ub, Vb, coef, bits)])
    assert worst <= 1, worst
    assert acc < {8: 3.7e7, 10: 1.5e8, 12: 5.9e8}[bits], acc      # the issue's bounds at 10 and 12; 2^24 * 2.2 at 8: all inside int32
    # the refusal bound of the C entry is an upper bound of every accumulator
    y_off, cy, crv, cgu, cgv, cbu = coef
    assert acc <= (cy << bits) + (max(crv, cgu + cgv, cbu) << (bits - 1)) + (1 << (15 + s)) < 1 << 31
    # the grey axis
    Y = np.arange(1 << bits)
    mid = np.full(1 << bits, 1 << (bits - 1))
    r, g, b = hc.channels(Y, mid, mid, coef, bits)
    assert np.array_equal(r, g) and np.array_equal(g, b)
    if full_range:
        assert r[0] == 0 and r[-1] == 255 and np.all(np.diff(r.astype(int)) >= 0)
    else:
        assert r[16 << s] == 0 and r[235 << s] == 255 and r[0] == 0 and r[-1] == 255


@pytest.mark.parametrize("matrix,full_range,bits", hc.SETTINGS)
def test_yuv_coefficients_equal_the_table(matrix, full_range, bits):
    assert preprocess.yuv_coefficients(matrix, full_range, bits) == hc.TABLE[matrix, full_range, bits]
    if bits == 8:
        assert preprocess.yuv_coefficients(matrix, full_range) == hc.TABLE[matrix, full_range, 8]
        if matrix != "bt2020":
            assert preprocess.yuv_coefficients(matrix, full_range, bits=8) == yc.TABLE[matrix, full_range]


def test_yuv_coefficients_refuse_other_bits():
    for bits in (9, 16, 0, True, "10"):
        with pytest.raises(ValueError, match="bits"):
            preprocess.yuv_coefficients("bt709", False, bits)


@pytest.mark.parametrize("H_,W_", [(3, 5), (4, 6), (1, 1)])
def test_at_8_bits_420_the_definition_is_section_19s(H_, W_):
    y, u, v = yc.random_planes(2, H_, W_)
    for key, coef in yc.TABLE.items():
        assert hc.TABLE[key + (8,)] == coef
        assert np.array_equal(hc.to_rgb(y, u, v, coef, 8, "420"), yc.to_rgb(y, u, v, coef))
    Y, U, V = np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 3), np.arange(0, 256, 7))
    for a, b in zip(hc.channels(Y, U, V, yc.TABLE["bt709", False]), yc.channels(Y, U, V, yc.TABLE["bt709", False])):
        assert np.array_equal(a, b)


def test_to_rgb_replicates_chroma_by_the_subsampling():
    for sub in hc.SUB:
        sx, sy = hc.SUB[sub]
        y, u, v = hc.random_planes(2, 3, 5, 10, sub)
        coef = hc.TABLE["bt2020", False, 10]
        rgb = hc.to_rgb(y, u, v, coef, 10, sub)
        for (t, yy, xx) in ((0, 0, 0), (1, 2, 4), (0, 1, 3), (1, 2, 1)):
            want = [int(c) for c in hc.channels(y[t, yy, xx], u[t, yy >> sy, xx >> sx], v[t, yy >> sy, xx >> sx], coef, 10)]
            assert rgb[t, yy, xx].tolist() == want


def test_junk_outside_the_sample_is_not_part_of_the_surface_samples():
    """the helper's own words(): the sample survives, the other bits differ between two seeds"""
    y, u, v = hc.random_planes(1, 4, 6, 10)
    for msb in (False, True):
        a, b = (hc.Surface(y, u, v, 10, msb, junk=k) for k in (1, 2))
        shift = 6 if msb else 0
        assert not np.array_equal(a.bufs[0], b.bufs[0])
        assert np.array_equal((a.bufs[0] >> shift) & 1023, y.reshape(-1)) and np.array_equal((b.bufs[0] >> shift) & 1023, y.reshape(-1))


# ------------------------------------------------------------------------------------------------ the container
def surface_frames(s, flats=None, **kw):
    """the YuvFrames a caller would build over the surface s"""
    planes = s.planes(s.tensors() if flats is None else flats)
    make = YuvFrames.i420 if s.layout == "planar" else YuvFrames.nv12
    return make(*planes, width=s.W, bits=s.bits, msb_aligned=s.msb, subsampling=s.sub, **kw)


def test_yuvframes_describes_the_new_kinds_without_copying():
    y, u, v = hc.random_planes(5, 4, 6, 10)
    s = hc.Surface(y, u, v, 10, True, "420", "uv", y_pitch=8, c_pitch=10, y_gap=16, c_gap=4, junk=0)
    flats = s.tensors()
    py, puv = s.planes(flats)
    f = YuvFrames.p010(py, puv, width=6, matrix="bt2020")
    assert f.shape == (5, 4, 6, 3) and not f.is_cuda and f.bits == 10 and f.msb_aligned and f.subsampling == "420"
    assert f.coef == hc.TABLE["bt2020", False, 10] and f.sample_size == 2 and not f.is_420_8bit
    assert encode.frames_size(f) == (5, (4, 6)) and encode.FrameSource(f).T0 == 5 and preprocess.is_yuv_frames(f)
    assert f.y.data_ptr() == flats[0].data_ptr() and f.chroma[0].data_ptr() == flats[1].data_ptr()
    g = f[1:3]
    assert isinstance(g, YuvFrames) and g.shape == (2, 4, 6, 3) and g.y.data_ptr() == py[1].data_ptr()
    assert (g.bits, g.msb_aligned, g.subsampling, g.matrix, g.coef) == (10, True, "420", "bt2020", f.coef)
    assert [tuple(p.shape) for p in g.planes()] == [(2, 4, 6), (2, 2, 6)]
    with pytest.raises(TypeError):
        f[0]
    # numpy uint16 planes are taken over the same memory too; p016 names its bits
    yw, uvw = s.bufs[0][:s.y_frame * 5].reshape(5, -1)[:, :32].reshape(5, 4, 8), s.bufs[1][:s.c_frame * 5].reshape(5, -1)[:, :20].reshape(5, 2, 10)
    n = YuvFrames.p016(yw, uvw, bits=12, width=6)
    assert n.bits == 12 and n.msb_aligned and n.y.dtype == torch.int16 and n.y.data_ptr() == yw.ctypes.data
    if hasattr(torch, "uint16"):
        t = YuvFrames.p010(py.view(torch.uint16), puv.view(torch.uint16), width=6)
        assert t.y.dtype == torch.int16 and t.y.data_ptr() == py.data_ptr()
    # 4:2:2 and 4:4:4: the chroma extents follow the sub-sampling, at odd sizes too
    for sub, shapes in (("422", [(2, 3, 5), (2, 3, 3), (2, 3, 3)]), ("444", [(2, 3, 5), (2, 3, 5), (2, 3, 5)]),
                        ("420", [(2, 3, 5), (2, 2, 3), (2, 2, 3)])):
        for bits in (8, 10, 12):
            y, u, v = hc.random_planes(2, 3, 5, bits, sub)
            f = YuvFrames.i420(y, u, v, bits=bits, subsampling=sub, matrix="bt709", full_range=True)
            assert f.shape == (2, 3, 5, 3) and f.coef == hc.TABLE["bt709", True, bits] and f.c_step == 1
            assert [tuple(p.shape) for p in f.planes()] == shapes
            assert f.is_420_8bit == (bits == 8 and sub == "420")
    y, u, v = hc.random_planes(2, 3, 5, 8, "444")
    uv = np.stack([u, v], -1).reshape(2, 3, 10)
    assert [tuple(p.shape) for p in YuvFrames.nv12(y, uv, subsampling="444").planes()] == [(2, 3, 5), (2, 3, 10)]
    # the old constructors' defaults are what they were
    y, u, v = yc.random_planes(2, 3, 5)
    f = YuvFrames.i420(y, u, v)
    assert (f.bits, f.msb_aligned, f.subsampling, f.coef, f.is_420_8bit) == (8, False, "420", yc.TABLE["bt601", False], True)


def test_yuvframes_refusals_of_the_new_kinds_name_what_is_wrong():
    y, u, v = hc.random_planes(3, 4, 6, 10)
    uv = np.stack([u, v], -1).reshape(3, 2, 6)
    y8, u8, v8 = yc.random_planes(3, 4, 6)
    uv8 = np.stack([u8, v8], -1).reshape(3, 2, 6)
    bad = [("y", lambda: YuvFrames.p010(y8, uv)),                                          # the sample type against the bits
           ("uv", lambda: YuvFrames.p010(y, uv8)),
           ("y", lambda: YuvFrames.nv12(y, uv)),
           ("u", lambda: YuvFrames.i420(y8, u, v8)),
           ("y", lambda: YuvFrames.p010(y.astype(np.int32), uv)),
           ("y", lambda: YuvFrames.p010(torch.zeros(3, 4, 6, dtype=torch.uint8), uv)),
           ("y", lambda: YuvFrames.p010(y[0], uv)),                                         # rank
           ("uv", lambda: YuvFrames.p010(y, uv[:, :, :5])),                                 # extents
           ("uv", lambda: YuvFrames.nv12(y, uv, bits=10, subsampling="422")),               # 4:2:2 wants H chroma rows
           ("u must be", lambda: YuvFrames.i420(y, u, v, bits=10, subsampling="444")),
           ("v must be", lambda: YuvFrames.i420(y, np.zeros((3, 4, 6), np.uint16), v, bits=10, subsampling="444")),
           ("u", lambda: YuvFrames.i420(y8, u8, v8, subsampling="422")),
           ("uv", lambda: YuvFrames.p010(y, np.zeros((3, 2, 12), np.uint16)[:, :, ::2])),   # last dimension not dense
           ("bits", lambda: YuvFrames.nv12(y, uv, bits=9)),
           ("bits", lambda: YuvFrames.nv12(y, uv, bits=16)),
           ("bits", lambda: YuvFrames.p016(y, uv, bits=8)),
           ("bits", lambda: YuvFrames.p016(y, uv, bits=16)),
           ("msb_aligned", lambda: YuvFrames.nv12(y8, uv8, msb_aligned=True)),
           ("msb_aligned", lambda: YuvFrames.nv12(y, uv, bits=10, msb_aligned=1)),
           ("subsampling", lambda: YuvFrames.nv12(y8, uv8, subsampling="440")),
           ("subsampling", lambda: YuvFrames.nv12(y8, uv8, subsampling=420)),
           ("matrix", lambda: YuvFrames.p010(y, uv, matrix="bt470")),
           ("width", lambda: YuvFrames.p010(y, uv, width=7)),
           ("full_range", lambda: YuvFrames.p010(y, uv, full_range=1))]
    for name, make in bad:
        with pytest.raises(ValueError, match=name):
            make()
    meta = torch.empty(3, 2, 6, dtype=torch.int16, device="meta")
    with pytest.raises(ValueError, match="uv is on meta"):
        YuvFrames.p010(y, meta)
    assert YuvFrames.p010(y, uv, matrix="bt2020").coef == hc.TABLE["bt2020", False, 10]
    assert YuvFrames.p016(y, uv, bits=12, matrix="bt2020", full_range=True).coef == hc.TABLE["bt2020", True, 12]


# ------------------------------------------------------------------------------------------------ the gather and the byte count
IDX = [0, 2, 3, 7]
KINDS = [(10, True, "420", "uv"), (10, False, "444", "planar"), (12, False, "422", "planar"), (12, True, "420", "uv"),
         (8, False, "444", "planar"), (8, False, "422", "uv")]


def samples_of(plane, s):
    """a gathered plane (torch uint8 / int16) -> its samples as numpy ints"""
    a = plane.numpy()
    if s.bits == 8:
        return a.astype(np.int64)
    return (a.view(np.uint16).astype(np.int64) >> (16 - s.bits if s.msb else 0)) & ((1 << s.bits) - 1)


@pytest.mark.parametrize("bits,msb,sub,layout", KINDS)
@pytest.mark.parametrize("h,w", [(4, 6), (3, 5)])
def test_gather_reads_neither_dropped_frames_nor_padding_and_counts_bytes(monkeypatch, bits, msb, sub, layout, h, w):
    gather = preprocess.gather_planes                             # no GPU here: selected_planes stages in pageable memory
    monkeypatch.setattr(preprocess, "gather_planes", lambda yuv, idx, pin=True: gather(yuv, idx, pin=False))
    y, u, v = hc.random_planes(9, h, w, bits, sub)
    hc_, wc = hc.chroma_shape(h, w, sub)
    cs = 1 if layout == "planar" else 2
    size = 1 if bits == 8 else 2
    staged = []
    for fill in (0xFF, 0x00):
        yy, uu, vv = (p.copy() for p in (y, u, v))
        for p in (yy, uu, vv):                                    # the dropped frames hold the fill too
            p[[t for t in range(9) if t not in IDX]] = fill | fill << 8 if bits > 8 else fill
        s = hc.Surface(yy & ((1 << bits) - 1), uu & ((1 << bits) - 1), vv & ((1 << bits) - 1), bits, msb, sub, layout,
                       y_pitch=w + 3, c_pitch=cs * wc + 3, y_gap=7, c_gap=5, fill=fill, junk=5)
        f = surface_frames(s)
        out, stage = gather(f, IDX, pin=False)
        assert stage.numel() == len(IDX) * (h * w + 2 * hc_ * wc) and stage.element_size() == size and stage.is_contiguous()
        assert np.array_equal(samples_of(out[0], s), y[IDX])
        if layout == "planar":
            assert np.array_equal(samples_of(out[1], s), u[IDX]) and np.array_equal(samples_of(out[2], s), v[IDX])
        else:
            assert np.array_equal(samples_of(out[1], s).reshape(len(IDX), hc_, wc, 2), np.stack([u[IDX], v[IDX]], -1))
        staged.append(stage.clone())
        # the byte count of the funnel: exactly the kept frames' samples, padding removed (the "device" here is the host)
        planes, uploaded = preprocess.selected_planes(f, IDX, torch.device("cpu"))
        assert uploaded == len(IDX) * (h * w + 2 * hc_ * wc) * size
        assert [tuple(p.shape) for p in planes] == [tuple(p[IDX].shape) for p in f.planes()]
        _, uploaded = preprocess.selected_planes(f, None, torch.device("cpu"))
        assert uploaded == 9 * (h * w + 2 * hc_ * wc) * size
    assert torch.equal(*staged)


# ------------------------------------------------------------------------------------------------ routing
@pytest.mark.parametrize("bits,msb,sub,layout", KINDS + [(8, False, "420", "uv"), (8, False, "420", "planar")])
def test_only_8_bit_420_goes_to_the_old_entry(monkeypatch, bits, msb, sub, layout):
    calls = []
    monkeypatch.setattr(ops, "yuv420_to_rgb", lambda y, u, v, c_step, coef, H, W, out=None: calls.append(("tdc_yuv420_to_rgb", c_step, coef, H, W)))
    monkeypatch.setattr(ops, "yuv_to_rgb", lambda y, u, v, c_step, coef, H, W, bits=8, msb_aligned=False, subsampling="420", out=None:
                        calls.append(("tdc_yuv_to_rgb", c_step, coef, H, W, bits, msb_aligned, subsampling)))
    y, u, v = hc.random_planes(2, 4, 6, bits, sub)
    f = surface_frames(hc.Surface(y, u, v, bits, msb, sub, layout), matrix="bt709")
    f.to_rgb(list(f.planes()), None)
    coef = hc.TABLE["bt709", False, bits]
    cs = 1 if layout == "planar" else 2
    if bits == 8 and sub == "420":
        assert calls == [("tdc_yuv420_to_rgb", cs, coef, 4, 6)]
    else:
        assert calls == [("tdc_yuv_to_rgb", cs, coef, 4, 6, bits, msb, sub)]


def test_the_c_abi_declares_the_new_entry_and_keeps_the_old():
    from tdc_video_amd import lib as L
    assert "tdc_yuv_to_rgb" in L.SIGNATURES and "tdc_yuv420_to_rgb" in L.SIGNATURES
    names = [n for n, _ in L.YuvPlanes._fields_]
    assert names[:8] == [n for n, _ in L.Yuv420Planes._fields_] and names[8:] == ["bits", "msb_aligned", "sub_x", "sub_y"]


# ------------------------------------------------------------------------------------------------ the frames funnel
class _HibitFrames(_Frames):
    """the engine double's pixels_from_frames: a YuvFrames of any kind goes through the product's host gather, then the numpy
    definition on the samples masked out of the gathered words"""

    def pixels_from_frames(self, frames, idx=None):
        if not preprocess.is_yuv_frames(frames):
            return _Frames.pixels_from_frames(self, frames, idx)
        keep = list(range(frames.shape[0])) if idx is None else list(idx)
        planes, stage = preprocess.gather_planes(frames, keep, pin=False)
        self.bytes_uploaded = stage.numel() * stage.element_size()
        y = samples_of(planes[0], frames_kind(frames))
        if frames.c_step == 2:
            c = samples_of(planes[1], frames_kind(frames))
            u, v = c[..., 0::2], c[..., 1::2]
        else:
            u, v = (samples_of(p, frames_kind(frames)) for p in planes[1:])
        rgb = hc.to_rgb(y, u, v, frames.coef, frames.bits, frames.subsampling)
        px = _Frames.pixels_from_frames(self, rgb, None)
        self.asked[-1] = None if idx is None else list(idx)
        return px


class frames_kind:
    def __init__(self, f):
        self.bits, self.msb = f.bits, f.msb_aligned


class HibitEngine(_HibitFrames, FeatureEngine):
    pass


@pytest.mark.parametrize("bits,msb,sub,layout", [(10, True, "420", "uv"), (10, False, "444", "planar")])
def test_encode_frames_on_the_new_kinds_equals_encode_frames_on_the_rgb_they_convert_to(bits, msb, sub, layout):
    eng = HibitEngine(N=5)
    y, u, v = hc.random_planes(40, H, W, bits, sub, seed=3)
    s = hc.Surface(y, u, v, bits, msb, sub, layout, y_pitch=W + 2, y_gap=3, fill=0x5A, junk=11)
    f = surface_frames(s, matrix="bt2020")
    rgb = hc.to_rgb(y, u, v, hc.TABLE["bt2020", False, bits], bits, sub)
    wi, gi = {}, {}
    want = encode.encode_frames_with(eng, rgb, 4, 4, [1, 2, 3], frame_cap=30, info=wi)
    eng.asked = []
    got = encode.encode_frames_with(eng, f, 4, 4, [1, 2, 3], frame_cap=30, info=gi)
    assert torch.equal(got, want) and gi == wi and gi["frames_in"] == 40 and gi["frames_resized"] == 30
    kept = encode.frame_indices(eng.cfg, 40, 4, 30)
    hc_, wc = hc.chroma_shape(H, W, sub)
    assert eng.asked == [kept] and eng.bytes_uploaded == 30 * (H * W + 2 * hc_ * wc) * 2
    # other junk in the ignored bits, the dropped frames and the padding overwritten: the same tokens
    s2 = hc.Surface(y, u, v, bits, msb, sub, layout, y_pitch=W + 2, y_gap=3, fill=0xFF, junk=12)
    for b, frame in zip(s2.bufs, (s2.y_frame, s2.c_frame, s2.c_frame)):
        for t in range(40):
            if t not in kept:
                b[t * frame:(t + 1) * frame] = 0xFFFF
    assert torch.equal(encode.encode_frames_with(eng, surface_frames(s2, matrix="bt2020"), 4, 4, [1, 2, 3], frame_cap=30), want)
    i1, i2 = {}, {}
    assert torch.equal(encode.encode_frames_with(eng, f[2:3], None, 4, None, info=i1, image=True),
                       encode.encode_frames_with(eng, rgb[2:3], None, 4, None, info=i2, image=True)) and i1 == i2


def test_preprocess_selected_checks_the_new_kinds_on_the_host_before_any_launch():
    y, u, v = hc.random_planes(6, H, W, 10)
    f = surface_frames(hc.Surface(y, u, v, 10, True))
    towers = (dict(R=2, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)),) * 2
    for idx in ([0, 6], [-1, 2], [2, 1], []):
        with pytest.raises(ValueError, match="idx"):
            preprocess.preprocess_selected(f, idx, towers)       # no GPU here: raised before one would be needed
    with pytest.raises(ValueError, match="slab"):
        preprocess.preprocess_selected(f, None, towers, slab=0)
