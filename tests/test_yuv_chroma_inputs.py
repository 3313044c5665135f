"""CPU: encode from YUV with interpolated chroma.  The numpy statement of the sited upsampling
(yuv_chroma_cases): its weights, its symmetries and its precision against real arithmetic for all 18 settings, four sitings
and both sub-samplings; the new keywords of YuvFrames / PackedYuvFrames; and the routing of to_rgb between the replicate and
the linear entry points."""
import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
import yuv_chroma_cases as cc
import yuv_hibit_cases as hc
import yuv_packed_cases as pc
from tdc_video_amd import ops, preprocess

YuvFrames = preprocess.YuvFrames
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (4, 6), (6, 16)]


# ------------------------------------------------------------------------------------------------ the weights
@pytest.mark.parametrize("sub", cc.SUBS)
@pytest.mark.parametrize("site", sorted(cc.SITES))
def test_weights_sum_to_16_and_a_constant_plane_stays_constant(sub, site):
    for H, W in SHAPES:
        Hc, Wc = hc.chroma_shape(H, W, sub)
        assert np.all(cc.weighted(np.ones((1, Hc, Wc), np.int64), H, W, sub, cc.SITES[site]) == 16)
        for bits in hc.BITS:
            for value in hc.edge_values(bits):
                c = np.full((2, Hc, Wc), value, np.uint16)
                assert np.all(cc.upsample(c, H, W, sub, cc.SITES[site]) == value), (H, W, bits, value)


def test_every_tap_stays_inside_the_plane_and_the_tables_are_the_stated_ones():
    for n_pix in range(1, 12):
        n = (n_pix + 1) >> 1
        for sited in (0, 1):
            ia, wa, ib, wb = cc.taps(n_pix, n, sited, 1)
            assert ia.min() >= 0 and ia.max() <= n - 1 and ib.min() >= 0 and ib.max() <= n - 1 and np.all(wa + wb == 4)
    ia, wa, ib, wb = cc.taps(6, 3, 0, 1)
    assert ia.tolist() == [0, 0, 1, 1, 2, 2] and wa.tolist() == [4, 2, 4, 2, 4, 2]
    assert ib.tolist()[1::2] == [1, 2, 2] and wb.tolist() == [0, 2, 0, 2, 0, 2]
    ia, wa, ib, wb = cc.taps(6, 3, 1, 1)
    assert ia.tolist() == [0, 0, 1, 1, 2, 2] and wa.tolist() == [3] * 6 and ib.tolist() == [0, 1, 0, 2, 1, 2] and wb.tolist() == [1] * 6
    ia, wa, ib, wb = cc.taps(5, 5, 1, 0)                          # an axis that is not sub-sampled: weight 4 on its own sample
    assert ia.tolist() == list(range(5)) and wa.tolist() == [4] * 5 and wb.tolist() == [0] * 5


def test_even_positions_of_a_co_sited_axis_return_the_sample_itself():
    for bits in hc.BITS:
        _, u, _ = hc.random_planes(2, 6, 10, bits, "420")
        up = cc.upsample(u, 6, 10, "420", cc.SITES["topleft"])
        assert np.array_equal(up[:, ::2, ::2], u)
        assert np.array_equal(cc.upsample(u, 6, 10, "420", cc.SITES["top"])[:, ::2], cc.upsample(u, 3, 10, "422", cc.SITES["top"]))
        _, u, _ = hc.random_planes(2, 5, 10, bits, "422")
        assert np.array_equal(cc.upsample(u, 5, 10, "422", cc.SITES["left"])[:, :, ::2], u)
        # 4:2:2: the vertical siting changes nothing
        assert np.array_equal(cc.upsample(u, 5, 10, "422", cc.SITES["left"]), cc.upsample(u, 5, 10, "422", cc.SITES["topleft"]))
        assert np.array_equal(cc.upsample(u, 5, 10, "422", cc.SITES["center"]), cc.upsample(u, 5, 10, "422", cc.SITES["top"]))


def test_centred_siting_commutes_with_mirroring_and_co_sited_does_not():
    H, W = 6, 10                                                  # even sizes: the mirrored picture has whole chroma blocks
    _, u, _ = hc.random_planes(3, H, W, 10, "420")
    c = cc.SITES["center"]
    assert np.array_equal(cc.upsample(u[:, :, ::-1], H, W, "420", c), cc.upsample(u, H, W, "420", c)[:, :, ::-1])
    assert np.array_equal(cc.upsample(u[:, ::-1], H, W, "420", c), cc.upsample(u, H, W, "420", c)[:, ::-1])
    for name, axis in (("left", 2), ("topleft", 2), ("topleft", 1), ("top", 1)):
        s = cc.SITES[name]
        flip = (slice(None),) * axis + (slice(None, None, -1),)
        assert not np.array_equal(cc.upsample(u[flip], H, W, "420", s), cc.upsample(u, H, W, "420", s)[flip]), name
    # left is centred down the rows, top across them
    assert np.array_equal(cc.upsample(u[:, ::-1], H, W, "420", cc.SITES["left"]), cc.upsample(u, H, W, "420", cc.SITES["left"])[:, ::-1])
    assert np.array_equal(cc.upsample(u[:, :, ::-1], H, W, "420", cc.SITES["top"]), cc.upsample(u, H, W, "420", cc.SITES["top"])[:, :, ::-1])


def test_an_impulse_spreads_by_the_stated_weights():
    c = np.zeros((1, 3, 3), np.uint16)
    c[0, 1, 1] = 1023
    r = lambda w: (w * 1023 + 8) >> 4
    up = cc.upsample(c, 6, 6, "420", cc.SITES["topleft"])[0]
    assert up[2, 2] == 1023 and up[2, 1] == r(8) and up[2, 3] == r(8) and up[1, 1] == r(4) and up[3, 3] == r(4) and up[2, 4] == 0
    up = cc.upsample(c, 6, 6, "420", cc.SITES["center"])[0]
    assert up[2, 2] == r(9) and up[3, 3] == r(9) and up[2, 1] == r(3) and up[1, 1] == r(1) and up[4, 4] == r(1) and up[0, 0] == 0
    up = cc.upsample(c, 6, 6, "420", cc.SITES["left"])[0]
    assert up[2, 2] == r(12) and up[2, 3] == r(6) and up[1, 2] == r(4) and up[1, 1] == r(2) and up[4, 3] == r(2)


# ------------------------------------------------------------------------------------------------ precision
@pytest.mark.parametrize("matrix,full_range,bits", hc.SETTINGS)
def test_every_byte_is_within_the_stated_bound_of_the_real_valued_conversion(matrix, full_range, bits):
    """the rounded real-valued matrix on the REAL-VALUED interpolated chroma: within 2 at 8 bits (rounding C' to a byte costs up
    to half a chroma step, times a coefficient of about 2.1), within 1 at 10 and 12 bits"""
    coef = hc.TABLE[matrix, full_range, bits]
    bound = 2 if bits == 8 else 1
    for sub in cc.SUBS:
        y, u, v = hc.random_planes(2, 37, 50, bits, sub)
        for name, site in cc.SITES.items():
            got = cc.to_rgb(y, u, v, coef, bits, sub, site)
            ur, vr = (cc.upsample_real(c, 37, 50, sub, site) for c in (u, v))
            worst = 0
            for k, r in enumerate(hc.real_channels(y, ur, vr, matrix, full_range, bits)):
                want = np.clip(np.floor(r + 0.5), 0, 255).astype(np.int64)
                worst = max(worst, int(np.abs(got[..., k].astype(np.int64) - want).max()))
            assert worst <= bound, (sub, name, worst)


# ------------------------------------------------------------------------------------------------ the container
def packed_frames(fmt="yuyv", bits=8, **kw):
    y, u, v = pc.random_planes(3, 4, 12, fmt, bits)
    s = pc.pack(y, u, v, fmt, bits, fmt in ("y210", "y416") and bits != 8)
    return YuvFrames.packed(s.plane(s.tensor()), fmt, width=12, bits=bits, **kw)


def test_the_new_keywords_default_to_what_was_and_are_kept_by_slicing():
    y, u, v = hc.random_planes(5, 4, 6, 8)
    f = YuvFrames.i420(y, u, v)
    assert (f.upsample, f.siting, f.interpolates) == ("replicate", "left", False)
    uv = np.stack([u, v], -1).reshape(5, 2, 6)
    for make in (lambda **k: YuvFrames.i420(y, u, v, **k), lambda **k: YuvFrames.nv12(y, uv, **k), lambda **k: YuvFrames(y, (uv,), 2, **k)):
        for site in cc.SITES:
            g = make(upsample="linear", siting=site)
            assert (g.upsample, g.siting, g.interpolates) == ("linear", site, True)
            h = g[1:3]
            assert (h.upsample, h.siting, h.shape) == ("linear", site, (2, 4, 6, 3))
            assert make(siting=site).interpolates is False and make(siting=site)[0:1].siting == site
    yw, uw, vw = hc.random_planes(5, 4, 6, 10)
    uvw = np.stack([uw, vw], -1).reshape(5, 2, 6)
    for g in (YuvFrames.p010(yw, uvw, upsample="linear", siting="topleft"), YuvFrames.p016(yw, uvw, 10, upsample="linear", siting="topleft")):
        assert (g.upsample, g.siting) == ("linear", "topleft") and (g[2:].upsample, g[2:].siting) == ("linear", "topleft")
    assert preprocess.CHROMA_SITES == cc.SITES
    # packed: every named constructor, and the slice
    data = packed_frames().y
    for g in (YuvFrames.yuy2(data, upsample="linear", siting="center"), YuvFrames.uyvy(data, upsample="linear", siting="center"),
              YuvFrames.packed(data, "yvyu", upsample="linear", siting="center"),
              preprocess.PackedYuvFrames(data, "vyuy", upsample="linear", siting="center")):
        assert (g.upsample, g.siting, g.interpolates) == ("linear", "center", True)
        assert (g[1:2].upsample, g[1:2].siting) == ("linear", "center")
    assert packed_frames("y210", 10, upsample="linear").interpolates and packed_frames("v210", 10, upsample="linear")[0:2].interpolates
    f = packed_frames()
    assert (f.upsample, f.siting, f.interpolates) == ("replicate", "left", False)
    # 4:4:4: accepted, nothing to interpolate
    y4, u4, v4 = hc.random_planes(2, 4, 6, 8, "444")
    assert YuvFrames.i420(y4, u4, v4, subsampling="444", upsample="linear").interpolates is False
    for fmt, bits in (("vuya", 8), ("ayuv", 8), ("y410", 10), ("y416", 12)):
        g = packed_frames(fmt, bits, upsample="linear", siting="top")
        assert g.upsample == "linear" and g.interpolates is False
    d8 = packed_frames("vuya").y
    assert YuvFrames.ayuv(d8, upsample="linear").upsample == "linear"
    assert YuvFrames.y410(packed_frames("y410", 10).y, upsample="linear", siting="top").siting == "top"
    assert YuvFrames.y210(packed_frames("y210", 10).y, upsample="linear").interpolates
    assert YuvFrames.v210(packed_frames("v210", 10).y, 12, upsample="linear", siting="topleft").siting == "topleft"


def test_refusals_name_the_argument():
    y, u, v = hc.random_planes(2, 4, 6, 8)
    data = packed_frames().y
    for bad in ("bilinear", "Linear", None, 1, ""):
        with pytest.raises(ValueError, match="upsample"):
            YuvFrames.i420(y, u, v, upsample=bad)
        with pytest.raises(ValueError, match="upsample"):
            YuvFrames.yuy2(data, upsample=bad)
    for bad in ("bottom", "bottomleft", "centre", None, (0, 1), 0):
        with pytest.raises(ValueError, match="siting"):
            YuvFrames.i420(y, u, v, siting=bad)
        with pytest.raises(ValueError, match="siting"):
            YuvFrames.packed(data, "yuyv", upsample="linear", siting=bad)


# ------------------------------------------------------------------------------------------------ routing
def _spy(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "yuv420_to_rgb", lambda y, u, v, c_step, coef, H, W, out=None: calls.append(("tdc_yuv420_to_rgb", c_step, coef, H, W)))
    monkeypatch.setattr(ops, "yuv_to_rgb", lambda y, u, v, c_step, coef, H, W, bits=8, msb_aligned=False, subsampling="420", out=None:
                        calls.append(("tdc_yuv_to_rgb", c_step, coef, H, W, bits, msb_aligned, subsampling)))
    monkeypatch.setattr(ops, "yuv_hdr_to_rgb", lambda y, u, v, c_step, coef, H, W, bits, msb_aligned, subsampling, hdr, out=None:
                        calls.append(("tdc_yuv_hdr_to_rgb", c_step, coef, H, W, bits, msb_aligned, subsampling, sorted(hdr))))
    monkeypatch.setattr(ops, "yuv_packed_to_rgb", lambda surface, fmt, coef, H, W, bits, msb_aligned, hdr=None, out=None:
                        calls.append(("tdc_yuv_packed_to_rgb", tuple(surface.shape), fmt, coef, H, W, bits, msb_aligned, hdr is not None)))
    monkeypatch.setattr(ops, "yuv_linear_to_rgb", lambda y, u, v, c_step, coef, H, W, bits, msb_aligned, subsampling, site, hdr=None, out=None:
                        calls.append(("tdc_yuv_linear_to_rgb", c_step, coef, H, W, bits, msb_aligned, subsampling, site, hdr is not None)))
    monkeypatch.setattr(ops, "yuv_packed_linear_to_rgb", lambda surface, fmt, coef, H, W, bits, msb_aligned, site, hdr=None, out=None:
                        calls.append(("tdc_yuv_packed_linear_to_rgb", tuple(surface.shape), fmt, coef, H, W, bits, msb_aligned, site, hdr is not None)))
    monkeypatch.setattr(preprocess, "hdr_lut", lambda *a: None)
    return calls


KINDS = [(8, False, "420", "uv"), (8, False, "420", "planar"), (8, False, "422", "uv"), (10, True, "420", "uv"), (12, False, "422", "planar")]


@pytest.mark.parametrize("bits,msb,sub,layout", KINDS)
def test_linear_issues_the_new_call_with_the_site_and_replicate_the_old_ones(monkeypatch, bits, msb, sub, layout):
    calls = _spy(monkeypatch)
    y, u, v = hc.random_planes(2, 4, 6, bits, sub)
    s = hc.Surface(y, u, v, bits, msb, sub, layout)
    planes = s.planes(s.tensors())
    make = YuvFrames.i420 if layout == "planar" else YuvFrames.nv12
    kw = dict(width=6, bits=bits, msb_aligned=msb, subsampling=sub, matrix="bt709")
    coef, cs = hc.TABLE["bt709", False, bits], 1 if layout == "planar" else 2
    old = ("tdc_yuv420_to_rgb", cs, coef, 4, 6) if bits == 8 and sub == "420" else ("tdc_yuv_to_rgb", cs, coef, 4, 6, bits, msb, sub)
    for name, site in cc.SITES.items():
        del calls[:]
        f = make(*planes, upsample="linear", siting=name, **kw)
        f.to_rgb(list(f.planes()), None)
        f[0:1].to_rgb(list(f[0:1].planes()), None)
        assert calls == [("tdc_yuv_linear_to_rgb", cs, coef, 4, 6, bits, msb, sub, site, False)] * 2
        del calls[:]
        for g in (make(*planes, siting=name, **kw), make(*planes, upsample="replicate", siting=name, **kw), make(*planes, **kw)):
            g.to_rgb(list(g.planes()), None)
        assert calls == [old] * 3
    if bits != 8:                                                 # HDR: the descriptor travels with the new call
        code = preprocess.yuv_code_coefficients("bt2020", False, bits)
        kw = dict(kw, matrix="bt2020", transfer="pq")
        del calls[:]
        f = make(*planes, upsample="linear", siting="topleft", **kw)
        f.to_rgb(list(f.planes()), None)
        g = make(*planes, siting="topleft", **kw)
        g.to_rgb(list(g.planes()), None)
        assert calls[0] == ("tdc_yuv_linear_to_rgb", cs, code, 4, 6, bits, msb, sub, (0, 0), True)
        assert calls[1][:8] == ("tdc_yuv_hdr_to_rgb", cs, code, 4, 6, bits, msb, sub) and len(calls) == 2


def test_linear_on_444_issues_the_old_call(monkeypatch):
    calls = _spy(monkeypatch)
    y, u, v = hc.random_planes(2, 4, 6, 10, "444")
    f = YuvFrames.i420(y, u, v, bits=10, subsampling="444", matrix="bt709", upsample="linear", siting="center")
    f.to_rgb(list(f.planes()), None)
    assert calls == [("tdc_yuv_to_rgb", 1, hc.TABLE["bt709", False, 10], 4, 6, 10, False, "444")]
    del calls[:]
    for fmt, bits in (("vuya", 8), ("y410", 10), ("y416", 12)):
        g = packed_frames(fmt, bits, upsample="linear", siting="center")
        g.to_rgb(list(g.planes()), None)
    assert [c[0] for c in calls] == ["tdc_yuv_packed_to_rgb"] * 3


@pytest.mark.parametrize("fmt,bits", [("yuyv", 8), ("uyvy", 8), ("y210", 10), ("y210", 12), ("v210", 10)])
def test_packed_linear_issues_the_new_call_and_replicate_the_old_one(monkeypatch, fmt, bits):
    calls = _spy(monkeypatch)
    msb = fmt == "y210"
    coef = hc.TABLE["bt601", False, bits]
    shape = (3, 4, pc.row_words(fmt, 12))
    for name, site in cc.SITES.items():
        del calls[:]
        f = packed_frames(fmt, bits, upsample="linear", siting=name)
        f.to_rgb(list(f.planes()), None)
        assert calls == [("tdc_yuv_packed_linear_to_rgb", shape, fmt, coef, 4, 12, bits, msb, site, False)]
        del calls[:]
        for g in (packed_frames(fmt, bits, siting=name), packed_frames(fmt, bits)):
            g.to_rgb(list(g.planes()), None)
        assert calls == [("tdc_yuv_packed_to_rgb", shape, fmt, coef, 4, 12, bits, msb, False)] * 2
    if bits != 8:
        del calls[:]
        f = packed_frames(fmt, bits, upsample="linear", siting="left", matrix="bt2020", transfer="hlg")
        f.to_rgb(list(f.planes()), None)
        assert calls == [("tdc_yuv_packed_linear_to_rgb", shape, fmt, preprocess.yuv_code_coefficients("bt2020", False, bits), 4, 12, bits,
                          msb, (0, 1), True)]


def test_the_c_abi_declares_both_symbols():
    import ctypes as C
    from tdc_video_amd import lib as L
    assert "tdc_yuv_linear_to_rgb" in L.SIGNATURES and "tdc_yuv_packed_linear_to_rgb" in L.SIGNATURES
    assert [n for n, _ in L.ChromaSite._fields_] == ["sit_x", "sit_y"] and C.sizeof(L.ChromaSite) == 8
    for name, first in (("tdc_yuv_linear_to_rgb", L.YuvPlanes), ("tdc_yuv_packed_linear_to_rgb", L.YuvPacked)):
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args[:4] == [C.POINTER(first), C.POINTER(L.YuvCoef), C.POINTER(L.HdrDesc), C.POINTER(L.ChromaSite)]
        assert args[4:] == [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    # the four replicate entries are what they were
    for name in ("tdc_yuv420_to_rgb", "tdc_yuv_to_rgb", "tdc_yuv_hdr_to_rgb", "tdc_yuv_packed_to_rgb"):
        assert name in L.SIGNATURES
