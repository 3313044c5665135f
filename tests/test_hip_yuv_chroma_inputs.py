"""GPU (-m gpu): encode from YUV with interpolated chroma.  tdc_yuv_linear_to_rgb and
tdc_yuv_packed_linear_to_rgb against the numpy statement of the sited upsampling (yuv_chroma_cases) and, byte for byte, against
the replicate entries on 4:4:4 device planes holding the upsampled samples - designed inputs, four sitings, both
sub-samplings, every depth, layout and form, the shapes where a neighbour's index can go wrong - their refusals, their memory
contracts, and the frames funnel on the tiny fixture engine of test_hip_frame_inputs.  Every comparison is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import memcheck
import test_hip_memory_contract as contract
import yuv_chroma_cases as cc
import yuv_hdr_cases as hd
import yuv_hibit_cases as hc
import yuv_packed_cases as pc
from test_hip_frame_inputs import IDX, R, fx, reference_pixels, towers  # noqa: F401  (fx: the engine fixture)
from test_hip_orient_inputs import _Traced
from test_hip_yuv_hdr_inputs import setting
from test_hip_yuv_hibit_inputs import DEPTHS, LAYOUTS, aligned, ragged
from test_hip_yuv_packed_inputs import aligned as packed_aligned, ragged as packed_ragged

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (2, 8), (4, 16), (5, 24), (6, 16), (4, 20)]
PACKED = [(f, bits, msb) for f in ("yuyv", "yvyu", "uyvy", "vyuy", "y210", "v210") for bits, msb in pc.DEPTHS[f]]
PACKED_WIDTHS = [2, 6, 8, 10, 24, 26, 48]          # v210's last group has 1, 3, 1, 2, 3, 1, 3 live pairs; 8, 24, 48: the vector forms
REPLICATE = ("tdc_yuv420_to_rgb", "tdc_yuv_to_rgb", "tdc_yuv_hdr_to_rgb", "tdc_yuv_packed_to_rgb")


def linear(s, flats, coef, site, hdr=None, out=None):
    """one tdc_yuv_linear_to_rgb call on the surface s, whose buffers are the flat device tensors `flats`"""
    from tdc_video_amd import ops
    y, u, v = s.views(flats)
    return ops.yuv_linear_to_rgb(y, u, v, s.c_step, coef, s.H, s.W, s.bits, s.msb, s.sub, site, hdr=hdr, out=out)


def packed_linear(s, flat, coef, site, hdr=None, out=None):
    """one tdc_yuv_packed_linear_to_rgb call on the packed surface s, whose buffer is the flat device tensor `flat`"""
    from tdc_video_amd import ops
    return ops.yuv_packed_linear_to_rgb(s.view(flat), s.fmt, coef, s.H, s.W, s.bits, s.msb, site, hdr=hdr, out=out)


def replicate_444(y, u, v, bits, sub, site, coef, hdr=None):
    """the parent's entries on 4:4:4 device planes holding the upsampled samples: tdc_yuv_to_rgb, or tdc_yuv_hdr_to_rgb"""
    from tdc_video_amd import ops
    H, W = y.shape[1:]
    s = hc.Surface(y, cc.upsample(u, H, W, sub, site), cc.upsample(v, H, W, sub, site), bits, False, "444", "planar")
    yv, uv, vv = s.views(s.tensors("cuda"))
    if hdr is not None:
        return ops.yuv_hdr_to_rgb(yv, uv, vv, 1, coef, H, W, bits, False, "444", hdr)
    return ops.yuv_to_rgb(yv, uv, vv, 1, coef, H, W, bits, False, "444")


def three(y, u, v, bits, msb, sub, lay):
    """aligned pitches and gaps (the vector form where W % 8 == 0), the smallest pitches with odd gaps (WORD), dense"""
    return aligned(y, u, v, bits, msb, sub, lay), ragged(y, u, v, bits, msb, sub, lay), hc.Surface(y, u, v, bits, msb, sub, lay, junk=9)


# ---------------------------------------------------------------------------------------------------- values and shapes
@pytest.mark.parametrize("bits,msb", DEPTHS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_sitings_layouts_and_forms_equal_the_definition_and_the_444_entry(H, W, bits, msb):
    """T = 3 with frame strides larger than the planes and random bits outside the samples; every siting, 4:2:0 and 4:2:2,
    uv / vu / planar, all three forms: the numpy definition, hence each other and tdc_yuv_to_rgb on the upsampled planes."""
    from tdc_video_amd import ops
    coefs = (hc.TABLE["bt2020" if bits != 8 else "bt601", False, bits], hc.TABLE["bt709", True, bits])
    for sub in cc.SUBS:
        y, u, v = hc.random_planes(3, H, W, bits, sub)
        for k, (name, site) in enumerate(sorted(cc.SITES.items())):
            coef = coefs[k & 1]
            want = torch.from_numpy(cc.to_rgb(y, u, v, coef, bits, sub, site)).cuda()
            assert torch.equal(replicate_444(y, u, v, bits, sub, site, coef), want), (sub, name)
            for lay in LAYOUTS:
                for s in three(y, u, v, bits, msb, sub, lay):
                    assert torch.equal(linear(s, s.tensors("cuda"), coef, site), want), (sub, name, lay, s.y_pitch, s.c_pitch)
            s = aligned(y, u, v, bits, msb, sub, LAYOUTS[k % 3])          # one frame of three, through the view's offset
            yv, uv, vv = s.views(s.tensors("cuda"))
            got = ops.yuv_linear_to_rgb(yv[1:2], uv[1:2], vv[1:2], s.c_step, coef, H, W, bits, msb, sub, site)
            assert torch.equal(got, want[1:2]), (sub, name)


@pytest.mark.parametrize("bits,msb", DEPTHS)
@pytest.mark.parametrize("sub", cc.SUBS)
def test_designed_inputs_equal_the_definition(bits, msb, sub):
    """impulses at every corner, edge and the interior, the 0 / max checkerboard, ramps, and three frames that differ in every
    sample (a halo from the wrong frame shows), at shapes of one WORD column, two vector units and a width that is no multiple
    of 8"""
    coef = hc.TABLE["bt709", False, bits]
    for H, W in [(3, 5), (4, 16), (6, 16), (5, 24), (4, 20)]:
        for case, (y, u, v) in cc.designed(H, W, bits, sub).items():
            surfaces = [make(y, u, v, bits, msb, sub, lay) for lay in ("uv", "planar") for make in (aligned, ragged)]
            flats = [s.tensors("cuda") for s in surfaces]
            for name, site in cc.SITES.items():
                want = torch.from_numpy(cc.to_rgb(y, u, v, coef, bits, sub, site)).cuda()
                for s, f in zip(surfaces, flats):
                    assert torch.equal(linear(s, f, coef, site), want), (H, W, case, name, s.layout, s.y_pitch)


@pytest.mark.parametrize("transfer", hd.TRANSFERS)
@pytest.mark.parametrize("bits,msb", [d for d in DEPTHS if d[0] != 8])
def test_with_a_descriptor_the_bytes_are_the_hdr_entrys_on_the_upsampled_planes(bits, msb, transfer):
    coef = hd.code_coefficients("bt2020", False, bits)
    _, hdr = setting(transfer, bits)
    for H, W in [(1, 1), (3, 5), (2, 8), (4, 16), (5, 24), (4, 20)]:
        for sub in cc.SUBS:
            y, u, v = hc.random_planes(3, H, W, bits, sub)
            for name, site in cc.SITES.items():
                ref = replicate_444(y, u, v, bits, sub, site, coef, hdr)
                for lay in ("uv", "planar"):
                    for make in (aligned, ragged):
                        s = make(y, u, v, bits, msb, sub, lay)
                        assert torch.equal(linear(s, s.tensors("cuda"), coef, site, hdr), ref), (H, W, sub, name, lay, s.y_pitch)


# ---------------------------------------------------------------------------------------------------- packed
@pytest.mark.parametrize("fmt,bits,msb", PACKED)
def test_packed_equals_the_definition_and_the_planar_entry_on_the_unpacked_samples(fmt, bits, msb):
    """H = 3, T = 3.  The group form (ragged, dense) and the vector form (aligned, W % 8 == 0), junk in bits 30-31, in the bits
    of a word outside the sample and in the tail of the last group."""
    coef = hc.TABLE["bt709", False, bits]
    for W in PACKED_WIDTHS:
        y, u, v = pc.random_planes(3, 3, W, fmt, bits)
        for k, (name, site) in enumerate(sorted(cc.SITES.items())):
            want = torch.from_numpy(cc.to_rgb(y, u, v, coef, bits, "422", site)).cuda()
            p = hc.Surface(y, u, v, bits, False, "422", "planar")
            assert torch.equal(linear(p, p.tensors("cuda"), coef, site), want), (W, name)
            for s in (packed_aligned(y, u, v, fmt, bits, msb), packed_ragged(y, u, v, fmt, bits, msb), pc.pack(y, u, v, fmt, bits, msb, junk=9 + k)):
                assert torch.equal(packed_linear(s, s.tensor("cuda"), coef, site), want), (W, name, s.pitch, s.frame)
        from tdc_video_amd import ops
        s = packed_aligned(y, u, v, fmt, bits, msb)                # one frame of three, through the view's offset
        got = ops.yuv_packed_linear_to_rgb(s.view(s.tensor("cuda"))[1:2], fmt, coef, 3, W, bits, msb, site)
        assert torch.equal(got, want[1:2]), W


@pytest.mark.parametrize("fmt,bits,msb,transfer", [("v210", 10, False, "hlg"), ("y210", 12, True, "pq")])
def test_packed_with_a_descriptor_equals_the_planar_linear_entry(fmt, bits, msb, transfer):
    coef = hd.code_coefficients("bt2020", False, bits)
    _, hdr = setting(transfer, bits)
    for W in PACKED_WIDTHS:
        y, u, v = pc.random_planes(2, 3, W, fmt, bits)
        p = hc.Surface(y, u, v, bits, False, "422", "planar")
        for name, site in cc.SITES.items():
            ref = linear(p, p.tensors("cuda"), coef, site, hdr)
            assert torch.equal(ref, replicate_444(y, u, v, bits, "422", site, coef, hdr)), (W, name)
            for s in (packed_aligned(y, u, v, fmt, bits, msb), packed_ragged(y, u, v, fmt, bits, msb)):
                assert torch.equal(packed_linear(s, s.tensor("cuda"), coef, site, hdr), ref), (W, name, s.pitch)


# ---------------------------------------------------------------------------------------------------- the memory contracts
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  The two functions below are entered there under their
# own names (not test_ names: that module collects nothing new).
@contract.covers("tdc_yuv_linear_to_rgb")
def yuv_linear_to_rgb_memory_contract(H, W, bits, msb, sub, siting, transfer):
    """tdc_yuv_linear_to_rgb: rgb in a guarded arena - nothing outside [T, H, W, 3] changes; the planes in poisoned arenas
    whose pitch padding, sample after an odd chroma row and gaps between frames hold 0x00, then 0xFF, and - with a descriptor -
    the table in a poisoned arena of its own: identical output, so no neighbour comes from outside the replicate read set."""
    T = 2
    site = cc.SITES[siting]
    y, u, v = hc.random_planes(T, H, W, bits, sub, seed=1)
    if transfer == "sdr":
        coef, tab, hdr = hc.TABLE["bt709", False, bits], None, None
        want = torch.from_numpy(cc.to_rgb(y, u, v, coef, bits, sub, site)).cuda()
    else:
        coef = hd.code_coefficients("bt2020", False, bits)
        tab, hdr = setting(transfer, bits)
        want = replicate_444(y, u, v, bits, sub, site, coef, hdr)
    for lay in LAYOUTS:
        for make in (aligned, ragged):
            results = []
            for pattern in memcheck.PATTERNS:
                s = make(y, u, v, bits, msb, sub, lay, fill=pattern, junk=4, gaps=(16, 16) if make is aligned else (7, 5))
                flats = [memcheck.poisoned(t, 256, 256, fill=pattern)[0] for t in s.tensors("cuda")]
                h = hdr and dict(hdr, lut=memcheck.poisoned(torch.from_numpy(tab).cuda(), 64, 64, fill=pattern)[0])
                out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
                linear(s, flats, coef, site, h, out=out)
                torch.cuda.synchronize()
                memcheck.assert_untouched(arena)
                assert torch.equal(out, want), (lay, s.y_pitch, pattern)
                results.append(out.clone())
            assert torch.equal(*results)


@contract.covers("tdc_yuv_packed_linear_to_rgb")
def yuv_packed_linear_to_rgb_memory_contract(H, W, fmt, bits, msb, siting, transfer):
    """tdc_yuv_packed_linear_to_rgb: rgb in a guarded arena; the surface in a poisoned arena whose pitch padding and gaps
    between frames hold 0x00, then 0xFF, other junk in every ignored bit and in the tail of the last group: identical output."""
    T = 2
    site = cc.SITES[siting]
    y, u, v = pc.random_planes(T, H, W, fmt, bits, seed=1)
    if transfer == "sdr":
        coef, tab, hdr = hc.TABLE["bt709", False, bits], None, None
        want = torch.from_numpy(cc.to_rgb(y, u, v, coef, bits, "422", site)).cuda()
    else:
        coef = hd.code_coefficients("bt2020", False, bits)
        tab, hdr = setting(transfer, bits)
        want = replicate_444(y, u, v, bits, "422", site, coef, hdr)
    for make in (packed_aligned, packed_ragged):
        results = []
        for pattern in memcheck.PATTERNS:
            s = make(y, u, v, fmt, bits, msb, fill=pattern, junk=4 + (pattern & 1), gap=16 if make is packed_aligned else 5)
            flat = memcheck.poisoned(s.tensor("cuda"), 256, 256, fill=pattern)[0]
            h = hdr and dict(hdr, lut=memcheck.poisoned(torch.from_numpy(tab).cuda(), 64, 64, fill=pattern)[0])
            out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
            packed_linear(s, flat, coef, site, h, out=out)
            torch.cuda.synchronize()
            memcheck.assert_untouched(arena)
            assert torch.equal(out, want), (make.__name__, s.pitch, pattern)
            results.append(out.clone())
        assert torch.equal(*results)


contract.yuv_linear_to_rgb_memory_contract = yuv_linear_to_rgb_memory_contract
contract.yuv_packed_linear_to_rgb_memory_contract = yuv_packed_linear_to_rgb_memory_contract


@pytest.mark.parametrize("bits,msb,sub,siting,transfer", [(8, False, "420", "left", "sdr"), (8, False, "422", "center", "sdr"),
                                                          (10, True, "420", "topleft", "pq"), (10, False, "420", "center", "sdr"),
                                                          (12, False, "422", "top", "hlg"), (12, True, "420", "center", "sdr")])
@pytest.mark.parametrize("H,W", [(3, 5), (6, 16), (5, 24)])
def test_memory_contract(H, W, bits, msb, sub, siting, transfer):
    yuv_linear_to_rgb_memory_contract(H, W, bits, msb, sub, siting, transfer)


@pytest.mark.parametrize("fmt,bits,msb,siting,transfer", [("yuyv", 8, False, "left", "sdr"), ("vyuy", 8, False, "center", "sdr"),
                                                          ("y210", 10, True, "center", "sdr"), ("y210", 12, False, "left", "pq"),
                                                          ("v210", 10, False, "left", "sdr"), ("v210", 10, False, "center", "hlg")])
@pytest.mark.parametrize("H,W", [(3, 5), (6, 16), (5, 24), (3, 32)])
def test_packed_memory_contract(H, W, fmt, bits, msb, siting, transfer):
    yuv_packed_linear_to_rgb_memory_contract(H, W, fmt, bits, msb, siting, transfer)


# ---------------------------------------------------------------------------------------------------- refusals
def test_badarg_before_any_launch():
    from tdc_video_amd import lib as L
    lib = L.load()
    T, H, W = 2, 4, 6
    y, u, v = hc.random_planes(T, H, W, 10)
    s = hc.Surface(y, u, v, 10, True, "420", "uv", 8, 8, 8, 8)    # in samples: pitches of 16 bytes, frames of 80 and 48
    flats = s.tensors("cuda")
    out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
    yp, up = flats[0].data_ptr(), flats[1].data_ptr()
    good_p = dict(y=yp, u=up, v=up + 2, y_frame=2 * s.y_frame, c_frame=2 * s.c_frame, y_pitch=16, c_pitch=16, c_step=4,
                  bits=10, msb_aligned=1, sub_x=1, sub_y=1)
    good_c = dict(zip(("y_off", "cy", "crv", "cgu", "cgv", "cbu"), hc.TABLE["bt2020", False, 10]))
    _, hdr = setting("pq", 10)
    good_h = dict(lut=hdr["lut"].data_ptr(), ootf_scale=1.0, ootf_exp=0.0, luma=(C.c_float * 3)(*hd.LUMA), inv_p2=0.04,
                  gamut=(C.c_float * 9)(*hd.GAMUT["bt2020"]))
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rc(p=None, c=None, h=None, site=(0, 1), dims=(T, H, W), rgb=out.data_ptr(), null=None):
        ps, cs = L.YuvPlanes(**dict(good_p, **(p or {}))), L.YuvCoef(**dict(good_c, **(c or {})))
        hs = None if h is None else C.byref(L.HdrDesc(**dict(good_h, **h)))
        return lib.tdc_yuv_linear_to_rgb(None if null == "p" else C.byref(ps), None if null == "c" else C.byref(cs), hs,
                                         None if null == "s" else C.byref(L.ChromaSite(*site)), *dims, C.c_void_p(rgb), stream())

    for site in cc.SITES.values():                               # taken: every siting, 4:2:0 and 4:2:2, with and without a descriptor
        assert rc(site=site) == 0 and rc(site=site, h={}) == 0
    rows4 = torch.zeros(2 * 4 * 8, dtype=torch.int16, device="cuda")          # 4:2:2: four chroma rows a frame
    assert rc(p=dict(sub_y=0, u=rows4.data_ptr(), v=rows4.data_ptr() + 2, c_frame=4 * 16)) == 0
    torch.cuda.synchronize()
    arena.buf.fill_(arena.fill)
    bad = [rc(null="s"), rc(site=(-1, 0)), rc(site=(2, 0)), rc(site=(0, -1)), rc(site=(0, 2)), rc(site=(2, 2), h={})]
    bad += [rc(p=dict(sub_x=0, sub_y=0, c_frame=4 * 16, c_pitch=32))]                                         # 4:4:4
    # several of what tdc_yuv_to_rgb refuses
    bad += [rc(null="p"), rc(null="c"), rc(rgb=0), rc(p=dict(y=0)), rc(p=dict(u=0)), rc(dims=(0, H, W)), rc(dims=(T, 65536, W)),
            rc(dims=(T, H, -1)), rc(p=dict(y_pitch=10)), rc(p=dict(c_pitch=10)), rc(p=dict(c_frame=16 + 8)), rc(p=dict(c_step=3)),
            rc(p=dict(bits=9)), rc(p=dict(sub_x=0, sub_y=1)), rc(p=dict(msb_aligned=2)), rc(p=dict(y=yp + 1)), rc(c=dict(y_off=16)),
            rc(c=dict(cy=-1)), rc(c=dict(cbu=(1 << 18) + 1)), rc(p=dict(sub_y=0))]
    # with a descriptor: bits = 8 and what tdc_yuv_hdr_to_rgb refuses about it
    bad += [rc(p=dict(bits=8, msb_aligned=0, c_step=2, y_pitch=8, c_pitch=8, y_frame=s.y_frame, c_frame=s.c_frame), c=dict(y_off=16), h={}),
            rc(h=dict(lut=0)), rc(h=dict(inv_p2=0.0)), rc(h=dict(ootf_exp=1.0)), rc(h=dict(ootf_scale=float("nan")))]
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad      # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(T, dtype=torch.bool))
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_yuv_linear_to_rgb")
    # 8 bits without a descriptor is taken (the replicate path sends it to tdc_yuv420_to_rgb; this entry takes it itself)
    assert rc(p=dict(bits=8, msb_aligned=0, c_step=2, y_pitch=8, c_pitch=8, y_frame=s.y_frame, c_frame=s.c_frame), c=dict(y_off=16)) == 0
    torch.cuda.synchronize()


def test_packed_badarg_before_any_launch():
    from tdc_video_amd import lib as L
    lib = L.load()
    F = L.YUV_PACKED_FORMATS
    T, H, W = 2, 4, 6
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    _, hdr = setting("pq", 10)
    out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
    rows = {"yuyv": 12, "yvyu": 12, "uyvy": 12, "vyuy": 12, "y210": 24, "vuya": 24, "ayuv": 24, "y410": 24, "y416": 48, "v210": 16}
    good_h = dict(lut=hdr["lut"].data_ptr(), ootf_scale=1.0, ootf_exp=0.0, luma=(C.c_float * 3)(*hd.LUMA), inv_p2=0.04,
                  gamut=(C.c_float * 9)(*hd.GAMUT["bt2020"]))

    def rc(fmt="y210", p=None, c=None, h=None, site=(0, 1), dims=(T, H, W), rgb=out.data_ptr(), null=None, bits=None):
        b = bits if bits is not None else pc.DEPTHS[fmt][0][0]
        good_p = dict(base=base, frame=3 * rows[fmt] + rows[fmt], pitch=rows[fmt], format=F[fmt], bits=b,
                      msb_aligned=int(fmt in ("y210", "y416")))
        coef = hc.TABLE["bt709", False, b] if b in (8, 10, 12) else hc.TABLE["bt709", False, 10]
        ps = L.YuvPacked(**dict(good_p, **(p or {})))
        cs = L.YuvCoef(**dict(dict(zip(("y_off", "cy", "crv", "cgu", "cgv", "cbu"), coef)), **(c or {})))
        hs = None if h is None else C.byref(L.HdrDesc(**dict(good_h, **h)))
        return lib.tdc_yuv_packed_linear_to_rgb(None if null == "p" else C.byref(ps), None if null == "c" else C.byref(cs), hs,
                                                None if null == "s" else C.byref(L.ChromaSite(*site)), *dims, C.c_void_p(rgb),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))

    for fmt in ("yuyv", "yvyu", "uyvy", "vyuy", "y210", "v210"):  # the 4:2:2 formats are taken at their smallest strides
        for site in cc.SITES.values():
            assert rc(fmt, site=site) == 0, fmt
    assert rc("y210", h={}) == 0 and rc("v210", h={}, site=(1, 1)) == 0 and rc("y210", bits=12, c=dict(y_off=256)) == 0
    torch.cuda.synchronize()
    arena.buf.fill_(arena.fill)
    bad = [rc(null="s"), rc(site=(-1, 0)), rc(site=(2, 1)), rc(site=(0, -1)), rc(site=(1, 2)), rc("v210", site=(2, 2), h={})]
    bad += [rc(f) for f in ("vuya", "ayuv", "y410", "y416")]                                                  # the 4:4:4 formats
    # several of what tdc_yuv_packed_to_rgb refuses
    bad += [rc(null="p"), rc(null="c"), rc(rgb=0), rc(p=dict(base=0)), rc(dims=(0, H, W)), rc(dims=(T, -1, W)), rc(dims=(T, H, 65536)),
            rc(p=dict(format=-1)), rc(p=dict(format=10)), rc("yuyv", bits=10), rc("y210", bits=8), rc("v210", bits=12),
            rc("yuyv", p=dict(msb_aligned=1)), rc(p=dict(msb_aligned=2)), rc("y210", p=dict(base=base + 1)), rc("v210", p=dict(pitch=18)),
            rc("v210", p=dict(frame=66))]
    bad += [rc(f, p=dict(pitch=rows[f] - pc.FORMATS[f][0]().itemsize)) for f in ("yuyv", "y210", "v210")]
    bad += [rc(f, p=dict(frame=4 * rows[f] - pc.FORMATS[f][0]().itemsize)) for f in ("uyvy", "y210", "v210")]
    bad += [rc(c=dict(y_off=1)), rc(c=dict(cy=-1)), rc(c=dict(crv=(1 << 18) + 1)), rc("yuyv", h={}), rc(h=dict(lut=0)),
            rc(h=dict(inv_p2=1.5)), rc("v210", h=dict(ootf_exp=0.2, ootf_scale=-1.0))]
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad      # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(T, dtype=torch.bool))
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_yuv_packed_linear_to_rgb")


# ---------------------------------------------------------------------------------------------------- the funnel
#        kind -> (siting, transfer)
FUNNEL = {"nv12": ("left", "sdr"), "p010_pq": ("topleft", "pq"), "v210": ("left", "sdr")}


def frames_over(kind, y, u, v, device, **kw):
    """the video as a YuvFrames of `kind`: on the device over a surface with pitches and gaps, or over dense pinned host
    memory; kw: upsample / siting, or nothing for the object as it was built before they existed"""
    from tdc_video_amd import preprocess as pp
    W = y.shape[2]
    if kind == "v210":
        s = packed_aligned(y, u, v, "v210", 10, False, fill=0xFF) if device == "cuda" else pc.pack(y, u, v, "v210", 10, junk=6)
        return pp.YuvFrames.v210(s.plane(s.tensor("cuda") if device == "cuda" else s.tensor(pin=True)), W, matrix="bt709", **kw)
    bits, msb = (8, False) if kind == "nv12" else (10, True)
    s = aligned(y, u, v, bits, msb, "420", "uv", fill=0xFF) if device == "cuda" else hc.Surface(y, u, v, bits, msb, "420", "uv", junk=6)
    planes = s.planes(s.tensors("cuda") if device == "cuda" else s.tensors(pin=True))
    if kind == "nv12":
        return pp.YuvFrames.nv12(*planes, width=W, matrix="bt709", **kw)
    return pp.YuvFrames.p010(*planes, width=W, matrix="bt2020", transfer="pq", **kw)


def planes_of(kind, T0, H, W, seed=0):
    bits, sub = {"nv12": (8, "420"), "p010_pq": (10, "420"), "v210": (10, "422")}[kind]
    return hc.random_planes(T0, H, W, bits, sub, seed)


def definition_rgb(kind, y, u, v):
    """the RGB frames of the definition -> host uint8.  SDR: numpy.  PQ: tdc_yuv_hdr_to_rgb on 4:4:4 device planes of the
    upsampled samples (its own tests hold it within 1 of the fp64 definition, which fixes no bytes to compare with)."""
    siting, transfer = FUNNEL[kind]
    bits, sub = {"nv12": (8, "420"), "p010_pq": (10, "420"), "v210": (10, "422")}[kind]
    if transfer == "sdr":
        return torch.from_numpy(cc.to_rgb(y, u, v, hc.TABLE["bt709", False, bits], bits, sub, cc.SITES[siting]))
    from tdc_video_amd import preprocess as pp
    f = frames_over(kind, y, u, v, "cuda")
    hdr = dict(f.hdr, lut=pp.hdr_lut(transfer, bits, f.peak_nits, f.sdr_white, "cuda"))
    return replicate_444(y, u, v, bits, sub, cc.SITES[siting], f.coef, hdr).cpu()


@pytest.mark.parametrize("kind", sorted(FUNNEL))
def test_preprocess_selected_issues_one_linear_launch_per_slab_and_equals_the_definitions_rgb(kind, monkeypatch):
    from tdc_video_amd import lib as L, preprocess as pp
    log = []
    monkeypatch.setattr(L, "_lib", _Traced(L.load(), log))
    new = "tdc_yuv_packed_linear_to_rgb" if kind == "v210" else "tdc_yuv_linear_to_rgb"
    siting = FUNNEL[kind][0]
    for H, W in [(90, 160), (45, 81)]:
        y, u, v = planes_of(kind, 16, H, W)
        want = reference_pixels(definition_rgb(kind, y, u, v)[IDX])
        for device in ("cuda", "pinned"):
            src = frames_over(kind, y, u, v, device, upsample="linear", siting=siting)
            for slab in (1, 7):
                del log[:]
                got = pp.preprocess_selected(src, IDX, towers(), torch.float16, slab)
                for g, w in zip(got, want):
                    assert g.is_cuda and tuple(g.shape) == (10, 3, R, R) and memcheck.same_bits(g, w), (device, slab, H, W)
                names = [c[0] for c in log]
                assert names.count(new) == -(-10 // slab) and not any(n in names for n in REPLICATE + ("tdc_pack_rgb",))
            # upsample="replicate", whatever the siting says: the launches of the object built without the new arguments
            logs = []
            for kw in ({}, dict(upsample="replicate", siting="top"), dict(siting="center")):
                del log[:]
                pp.preprocess_selected(frames_over(kind, y, u, v, device, **kw), IDX, towers(), torch.float16, 7)
                logs.append(list(log))
            assert logs[0] == logs[1] == logs[2] and new not in [c[0] for c in logs[0]]
            assert sum(c[0] in REPLICATE for c in logs[0]) == 2


@functools.lru_cache(maxsize=None)
def video(kind, H=90, W=160, T0=40):
    """one video of scenes of five frames -> (its linear sources on the device and in pinned memory, the definition's RGB)"""
    bits = 8 if kind == "nv12" else 10
    y, u, v = planes_of(kind, T0, H, W, seed=4)
    for t in range(T0):                                           # scenes of five frames, so that the segmentation has cuts to find
        if t % 5:
            y[t] = np.clip(y[t - t % 5].astype(np.int32) + (y[t] % 29).astype(np.int32) - 14, 0, (1 << bits) - 1)
            u[t], v[t] = u[t - t % 5], v[t - t % 5]
    kw = dict(upsample="linear", siting=FUNNEL[kind][0])
    return ({d: frames_over(kind, y, u, v, d, **kw) for d in ("cuda", "pinned")}, definition_rgb(kind, y, u, v),
            frames_over(kind, y, u, v, "cuda", siting=FUNNEL[kind][0]))


@pytest.mark.parametrize("kind", sorted(FUNNEL))
def test_every_frames_entry_equals_the_same_call_on_the_definitions_rgb(fx, kind):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc, pid = fx["enc"], fx["pid"]
    srcs, rgb, rep = video(kind)
    wi, ti = {}, {}
    want = enc.encode_frames(rgb, 9, 8, pid, frame_cap=30, info=wi)
    turned = enc.encode_frames(pp.Oriented(rgb, rotate=90), 9, 8, pid, frame_cap=30, info=ti)
    c = enc.new_cache(1 << 30)
    i0 = {}
    assert torch.equal(enc.encode_frames(rgb, 9, 8, pid, frame_cap=30, info=i0, cache=c), want)      # first asked as RGB
    assert i0["cache"]["frames_encoded"] == 30
    for name, src in srcs.items():
        gi, oi, hi = {}, {}, {}
        assert src.upsample == "linear" and src.interpolates
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=gi), want), name
        assert gi == wi and gi["frames_resized"] == 30
        assert torch.equal(enc.encode_frames(pp.Oriented(src, rotate=90), 9, 8, pid, frame_cap=30, info=oi), turned), name
        assert oi == ti
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=hi, cache=c), want), name
        assert hi["cache"]["frames_encoded"] == 0 and hi["cache"]["frames_hit"] == hi["cache"]["frames"] == 30
    i1, i2 = {}, {}
    assert torch.equal(enc.encode_frames(srcs["cuda"][3:4], None, 8, None, image=True, info=i1),
                       enc.encode_frames(rgb[3:4], None, 8, None, image=True, info=i2)) and i1 == i2
    qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid), dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:])]
    for a, b in zip(enc.encode_frames_prompts(srcs["pinned"], qs, frame_cap=30, pad_fraction=1.0),
                    enc.encode_frames_prompts(rgb, qs, frame_cap=30, pad_fraction=1.0)):
        assert torch.equal(a, b)
    w = enc.export_features_from_frames(rgb, slab=16)
    g = enc.export_features_from_frames(srcs["cuda"], slab=16)
    assert g.signature == w.signature and memcheck.same_bits(g.siglip, w.siglip) and memcheck.same_bits(g.dino, w.dino)
    # the replicate route of the same planes is other pixels: the keyword is not silently ignored
    assert rep.upsample == "replicate" and not torch.equal(enc.encode_frames(rep, 9, 8, pid, frame_cap=30), want)
