"""GPU (-m gpu): encode from packed YUV surfaces - YUY2, UYVY, Y210, AYUV, Y410, Y416, v210.
tdc_yuv_packed_to_rgb against the numpy definition on the unpacked planes (yuv_packed_cases: only the layout is new), byte for
byte against tdc_yuv_to_rgb and tdc_yuv_hdr_to_rgb on device planes of the same samples, the shapes where indexing can go
wrong in every form of the kernel, the lattice, its memory contract and its refusals; then the frames funnel and the tiny
fixture engine of test_hip_frame_inputs: everything behind the conversion is the RGB frames path, so every comparison is bit
for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import memcheck
import test_hip_memory_contract as contract
import yuv_cases as yc
import yuv_hdr_cases as hd
import yuv_hibit_cases as hc
import yuv_packed_cases as pc
from test_hip_boundary import loaded_lm
from test_hip_frame_inputs import IDX, R, _call, _same, fx, reference_pixels, towers  # noqa: F401  (fx: the engine fixture)
from test_hip_orient_inputs import _Traced
from test_hip_yuv_hdr_inputs import setting, worst_and_share

pytestmark = pytest.mark.gpu

EVERY = [(f, bits, msb) for f in pc.FORMATS for bits, msb in pc.DEPTHS[f]]
SHAPES = [(1, 1), (2, 8), (3, 5), (5, 24), (4, 20), (6, 16)]
V210_WIDTHS = [6, 7, 12, 48, 50, 32, 40]       # the issue's, and the two tails of the 24-pixel form: 8 and 16 pixels
COEFS = (("bt2020", False), ("bt709", True))


def coef_of(k, bits):
    matrix, full_range = COEFS[k]
    return hc.TABLE["bt601" if matrix == "bt2020" and bits == 8 else matrix, full_range, bits]


def convert(s, flat, coef, hdr=None, out=None):
    """one tdc_yuv_packed_to_rgb call on the surface s, whose buffer is the flat device tensor `flat`"""
    from tdc_video_amd import ops
    return ops.yuv_packed_to_rgb(s.view(flat), s.fmt, coef, s.H, s.W, s.bits, s.msb, hdr=hdr, out=out)


def aligned(y, u, v, fmt, bits, msb, fill=0xA5, junk=7, gap=64):
    """a pitch and a frame stride that are multiples of 16 bytes: the 16-byte forms wherever W allows"""
    b = pc.FORMATS[fmt][0]().itemsize
    row = pc.row_words(fmt, y.shape[2]) * b
    pitch = (row + 15) // 16 * 16 + 16
    return pc.pack(y, u, v, fmt, bits, msb, pitch // b, (16 - (y.shape[1] * pitch) % 16) % 16 // b + gap // b, fill, junk)


def ragged(y, u, v, fmt, bits, msb, fill=0xA5, junk=8, gap=3):
    """the smallest pitch that leaves padding and an odd gap, in words: every row and frame at another alignment (the group form)"""
    return pc.pack(y, u, v, fmt, bits, msb, pc.row_words(fmt, y.shape[2]) + 1, gap, fill, junk)


def three(y, u, v, fmt, bits, msb):
    return aligned(y, u, v, fmt, bits, msb), ragged(y, u, v, fmt, bits, msb), pc.pack(y, u, v, fmt, bits, msb, junk=9)


def planar(y, u, v, fmt, bits, coef, hdr=None):
    """the parent's entries on device planes holding the same samples -> rgb"""
    from tdc_video_amd import ops
    s = hc.Surface(y, u, v, bits, False, pc.sub(fmt), "planar")
    yv, uv, vv = s.views(s.tensors("cuda"))
    if hdr is not None:
        return ops.yuv_hdr_to_rgb(yv, uv, vv, 1, coef, s.H, s.W, bits, False, pc.sub(fmt), hdr)
    return ops.yuv_to_rgb(yv, uv, vv, 1, coef, s.H, s.W, bits, False, pc.sub(fmt))


# ---------------------------------------------------------------------------------------------------- shapes and values
def shapes_of(fmt):
    return SHAPES + ([(3, w) for w in V210_WIDTHS] if fmt == "v210" else [])


@pytest.mark.parametrize("fmt,bits,msb", EVERY)
def test_shapes_pitches_frame_strides_and_junk_equal_the_definition_and_the_planar_entry(fmt, bits, msb):
    """T = 3.  Aligned pitch and gaps (the 16-byte forms where W allows), the smallest pitch that leaves padding with odd
    gaps (the group form) and a dense surface all equal the definition, hence each other, and tdc_yuv_to_rgb on planes."""
    for H, W in shapes_of(fmt):
        y, u, v = pc.random_planes(3, H, W, fmt, bits)
        for k in range(2):
            coef = coef_of(k, bits)
            want = torch.from_numpy(pc.to_rgb(y, u, v, coef, fmt, bits)).cuda()
            assert torch.equal(planar(y, u, v, fmt, bits, coef), want)
            for s in three(y, u, v, fmt, bits, msb):
                assert torch.equal(convert(s, s.tensor("cuda"), coef), want), (H, W, k, s.pitch, s.frame)
        s = aligned(y, u, v, fmt, bits, msb)                      # one frame of three, through the view's offset
        from tdc_video_amd import ops
        got = ops.yuv_packed_to_rgb(s.view(s.tensor("cuda"))[1:2], fmt, coef, H, W, bits, msb)
        assert torch.equal(got, want[1:2]), (H, W)


@pytest.mark.parametrize("transfer", hd.TRANSFERS)
@pytest.mark.parametrize("fmt,bits,msb", [e for e in EVERY if e[1] != 8])
def test_with_a_descriptor_the_bytes_are_the_hdr_entrys_and_within_1_of_the_definition(fmt, bits, msb, transfer):
    coef = hd.code_coefficients("bt2020", False, bits)
    tab, hdr = setting(transfer, bits)
    for H, W in [s for s in shapes_of(fmt) if s not in ((1, 1), (4, 20))]:
        y, u, v = pc.random_planes(3, H, W, fmt, bits)
        ref = planar(y, u, v, fmt, bits, coef, hdr)
        worst, share = worst_and_share(ref, pc.hdr_to_rgb(y, u, v, coef, fmt, bits, tab, hdr))
        print("tdc_yuv_packed_to_rgb %s %s %d bits %dx%d: largest difference from the fp64 definition %d, differing share %.3g"
              % (fmt, transfer, bits, H, W, worst, share))
        assert worst <= 1
        for s in three(y, u, v, fmt, bits, msb):
            assert torch.equal(convert(s, s.tensor("cuda"), coef, hdr), ref), (H, W, s.pitch, s.frame)


# ---------------------------------------------------------------------------------------------------- the lattice
@pytest.mark.parametrize("fmt,bits,msb", [("vuya", 8, False), ("y410", 10, False), ("v210", 10, False), ("y416", 12, True),
                                          ("y416", 12, False)])
def test_the_lattice_equals_the_definition(fmt, bits, msb):
    y, u, v = hc.lattice(bits)
    if pc.sub(fmt) == "422":                                     # the chroma of a lattice row is one value: every other sample
        u, v = u[:, :, ::2], v[:, :, ::2]
    for k in range(2):
        coef = coef_of(k, bits)
        want = torch.from_numpy(pc.to_rgb(y, u, v, coef, fmt, bits)).cuda()
        for s in (aligned(y, u, v, fmt, bits, msb), ragged(y, u, v, fmt, bits, msb)):
            assert torch.equal(convert(s, s.tensor("cuda"), coef), want), (k, s.pitch)


# ---------------------------------------------------------------------------------------------------- the memory contract
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  tdc_yuv_packed_to_rgb's is the function below: it is
# entered there under its own name (not a test_ name: that module collects nothing new).
@contract.covers("tdc_yuv_packed_to_rgb")
def yuv_packed_to_rgb_memory_contract(H, W, fmt, bits, msb, transfer):
    """tdc_yuv_packed_to_rgb: rgb in a guarded arena - nothing outside [T, H, W, 3] changes; the surface in a poisoned arena
    whose pitch padding and gaps between frames hold 0x00, then 0xFF, other junk in every ignored bit and sample, and - with
    a descriptor - the table of exactly 2^bits floats in a poisoned arena of its own: identical output, in both forms."""
    T = 2
    y, u, v = pc.random_planes(T, H, W, fmt, bits, seed=1)
    if transfer == "sdr":
        coef, tab, hdr = hc.TABLE["bt709", False, bits], None, None
        want = torch.from_numpy(pc.to_rgb(y, u, v, coef, fmt, bits)).cuda()
    else:
        coef = hd.code_coefficients("bt2020", False, bits)
        tab, hdr = setting(transfer, bits)
        want = planar(y, u, v, fmt, bits, coef, hdr)
    for make in (aligned, ragged):
        results = []
        for pattern in memcheck.PATTERNS:
            s = make(y, u, v, fmt, bits, msb, fill=pattern, junk=4 + (pattern & 1), gap=16 if make is aligned else 5)
            flat = memcheck.poisoned(s.tensor("cuda"), 256, 256, fill=pattern)[0]
            h = hdr and dict(hdr, lut=memcheck.poisoned(torch.from_numpy(tab).cuda(), 64, 64, fill=pattern)[0])
            out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
            convert(s, flat, coef, h, out=out)
            torch.cuda.synchronize()
            memcheck.assert_untouched(arena)
            assert torch.equal(out, want), (make.__name__, s.pitch, pattern)
            results.append(out.clone())
        assert torch.equal(*results)


contract.yuv_packed_to_rgb_memory_contract = yuv_packed_to_rgb_memory_contract


@pytest.mark.parametrize("fmt,bits,msb,transfer", [("yuyv", 8, False, "sdr"), ("vyuy", 8, False, "sdr"), ("y210", 10, True, "sdr"),
                                                   ("y210", 12, False, "pq"), ("vuya", 8, False, "sdr"), ("ayuv", 8, False, "sdr"),
                                                   ("y416", 12, True, "sdr"), ("y416", 10, False, "hlg"), ("y410", 10, False, "sdr"),
                                                   ("y410", 10, False, "pq"), ("v210", 10, False, "sdr"), ("v210", 10, False, "hlg")])
@pytest.mark.parametrize("H,W", [(3, 5), (6, 16), (5, 24)])
def test_memory_contract(H, W, fmt, bits, msb, transfer):
    yuv_packed_to_rgb_memory_contract(H, W, fmt, bits, msb, transfer)


@pytest.mark.parametrize("transfer", ["sdr", "pq"])
@pytest.mark.parametrize("H,W", [(4, 32), (3, 40), (2, 48)])
def test_memory_contract_of_the_v210_rows_that_end_in_groups(H, W, transfer):
    yuv_packed_to_rgb_memory_contract(H, W, "v210", 10, False, transfer)


# ---------------------------------------------------------------------------------------------------- refusals
def test_badarg_before_any_launch():
    from tdc_video_amd import lib as L
    lib = L.load()
    F = L.YUV_PACKED_FORMATS
    T, H, W = 2, 4, 6
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    tab, hdr = setting("pq", 10)
    out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
    # per format: the smallest pitch and frame stride that are enough for 4 x 6, in bytes
    rows = {"yuyv": 12, "yvyu": 12, "uyvy": 12, "vyuy": 12, "y210": 24, "vuya": 24, "ayuv": 24, "y410": 24, "y416": 48, "v210": 16}
    good_h = dict(lut=hdr["lut"].data_ptr(), ootf_scale=1.0, ootf_exp=0.0, luma=(C.c_float * 3)(*hd.LUMA), inv_p2=0.04,
                  gamut=(C.c_float * 9)(*hd.GAMUT["bt2020"]))

    def rc(fmt="y210", p=None, c=None, h=None, dims=(T, H, W), rgb=out.data_ptr(), null=None, bits=None):
        b = bits if bits is not None else pc.DEPTHS[fmt][0][0]
        good_p = dict(base=base, frame=3 * rows[fmt] + rows[fmt], pitch=rows[fmt], format=F[fmt], bits=b,
                      msb_aligned=int(fmt in ("y210", "y416")))
        coef = hc.TABLE["bt709", False, b] if b in (8, 10, 12) else hc.TABLE["bt709", False, 10]
        ps = L.YuvPacked(**dict(good_p, **(p or {})))
        cs = L.YuvCoef(**dict(dict(zip(("y_off", "cy", "crv", "cgu", "cgv", "cbu"), coef)), **(c or {})))
        hs = None if h is None else C.byref(L.HdrDesc(**dict(good_h, **h)))
        return lib.tdc_yuv_packed_to_rgb(None if null == "p" else C.byref(ps), None if null == "c" else C.byref(cs), hs, *dims,
                                         C.c_void_p(rgb), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    # every format is taken at its smallest strides, with and without a descriptor where it has one
    for fmt in F:
        assert rc(fmt) == 0, fmt
    assert rc("y210", h={}) == 0 and rc("v210", h={}) == 0 and rc("y410", h={}) == 0 and rc("y416", bits=12, c=dict(y_off=256)) == 0
    torch.cuda.synchronize()
    arena.buf.fill_(arena.fill)
    bad = [rc(null="p"), rc(null="c"), rc(rgb=0), rc(p=dict(base=0))]                                          # a null pointer
    for i in range(3):                                                                                         # T, H, W
        for n in (0, -1, 65536):
            dims = [T, H, W]
            dims[i] = n
            bad.append(rc(dims=tuple(dims)))
    bad += [rc(p=dict(format=f)) for f in (-1, 10, 255)]                                                       # an unknown format
    bad += [rc("yuyv", bits=b) for b in (10, 12, 0)] + [rc("vuya", bits=10)]                                   # bits the format does not take
    bad += [rc("y210", bits=b) for b in (8, 9, 16)] + [rc("y416", bits=b) for b in (8, 14)]
    bad += [rc("y410", bits=b) for b in (8, 12)] + [rc("v210", bits=b) for b in (8, 12)]
    bad += [rc(f, p=dict(msb_aligned=1)) for f in ("yuyv", "uyvy", "vuya", "ayuv", "y410", "v210")]            # msb_aligned
    bad += [rc(p=dict(msb_aligned=2)), rc(p=dict(msb_aligned=-1))]
    bad += [rc("y210", p=dict(base=base + 1)), rc("y210", p=dict(pitch=25)), rc("y210", p=dict(frame=97)),     # the word size
            rc("y416", p=dict(base=base + 1)), rc("y416", p=dict(pitch=49)), rc("y416", p=dict(frame=193)),
            rc("y410", p=dict(base=base + 2)), rc("y410", p=dict(pitch=26)), rc("y410", p=dict(frame=98)),
            rc("v210", p=dict(base=base + 2)), rc("v210", p=dict(pitch=18)), rc("v210", p=dict(frame=66))]
    bad += [rc(f, p=dict(pitch=rows[f] - pc.FORMATS[f][0]().itemsize)) for f in F]                             # pitch below the read set
    bad += [rc(f, p=dict(frame=4 * rows[f] - pc.FORMATS[f][0]().itemsize)) for f in F]                         # the last row not cleared
    bad += [rc(p=dict(frame=0)), rc(p=dict(frame=-96))]
    bad += [rc(c=dict(y_off=1)), rc(c=dict(y_off=16)), rc("yuyv", c=dict(y_off=64)), rc(c=dict(y_off=-64))]     # y_off, coefficients
    for k in ("cy", "crv", "cgu", "cgv", "cbu"):
        bad += [rc(c={k: -1}), rc(c={k: (1 << 18) + 1})]
    bad += [rc(f, h={}) for f in ("yuyv", "uyvy", "vuya", "ayuv")]                                             # with h: bits = 8
    nan, inf = float("nan"), float("inf")
    bad += [rc(h=dict(lut=0)), rc(h=dict(lut=hdr["lut"].data_ptr() + 2)), rc(h=dict(ootf_scale=nan)), rc(h=dict(ootf_exp=inf)),
            rc(h=dict(inv_p2=nan)), rc(h=dict(luma=(C.c_float * 3)(0.2, nan, 0.1))), rc(h=dict(gamut=(C.c_float * 9)(*([1.0] * 8 + [inf])))),
            rc(h=dict(inv_p2=0.0)), rc(h=dict(inv_p2=1.5)), rc(h=dict(ootf_exp=-0.1)), rc(h=dict(ootf_exp=1.0)),
            rc(h=dict(ootf_exp=0.2, ootf_scale=0.0)), rc("v210", h=dict(ootf_exp=0.2, ootf_scale=-1.0))]
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad      # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(T, dtype=torch.bool))
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_yuv_packed_to_rgb")
    # the largest coefficients are taken, as tdc_yuv_to_rgb takes them
    assert rc("y416", bits=12, c=dict(cy=1 << 18, cbu=1 << 18, crv=0, y_off=256)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the funnel
FUNNEL = {"yuy2": ("yuyv", 8, False, "sdr"), "y210": ("y210", 10, True, "sdr"), "y410": ("y410", 10, False, "sdr"),
          "v210": ("v210", 10, False, "sdr"), "v210_hlg": ("v210", 10, False, "hlg")}


def frames_over(s, flat, transfer="sdr"):
    from tdc_video_amd import preprocess as pp
    return pp.YuvFrames.packed(s.plane(flat), s.fmt, width=s.W, bits=s.bits, msb_aligned=s.msb,
                               matrix="bt601" if s.bits == 8 else "bt2020", transfer=transfer)


def sources(y, u, v, kind):
    """the same video as packed YuvFrames over a device surface with a pitch and gaps, and over a dense pinned host one"""
    fmt, bits, msb, transfer = FUNNEL[kind]
    a = aligned(y, u, v, fmt, bits, msb, fill=0xFF)
    c = pc.pack(y, u, v, fmt, bits, msb, junk=6)
    return {"cuda": frames_over(a, a.tensor("cuda"), transfer), "pinned": frames_over(c, c.tensor(pin=True), transfer)}


def definition_rgb(y, u, v, kind):
    """the RGB frames the surface stands for -> host uint8.  SDR: the numpy definition.  HLG: what tdc_yuv_hdr_to_rgb writes for
    the same samples in planes (its own tests hold it within 1 of the fp64 definition, which fixes no bytes to compare with)"""
    fmt, bits, _, transfer = FUNNEL[kind]
    if transfer == "sdr":
        return torch.from_numpy(pc.to_rgb(y, u, v, hc.TABLE["bt601" if bits == 8 else "bt2020", False, bits], fmt, bits))
    from tdc_video_amd import preprocess as pp
    f = pp.YuvFrames.i420(y, u, v, bits=bits, subsampling=pc.sub(fmt), matrix="bt2020", transfer=transfer)
    hdr = dict(f.hdr, lut=pp.hdr_lut(transfer, bits, f.peak_nits, f.sdr_white, "cuda"))
    return planar(y, u, v, fmt, bits, f.coef, hdr).cpu()


@pytest.mark.parametrize("kind", sorted(FUNNEL))
def test_preprocess_selected_on_packed_surfaces_equals_process_images_of_the_definitions_rgb(kind, monkeypatch):
    from tdc_video_amd import lib as L, preprocess as pp
    fmt, bits = FUNNEL[kind][:2]
    log = []
    monkeypatch.setattr(L, "_lib", _Traced(L.load(), log))
    for H, W in [(90, 160), (45, 81)] + ([(45, 50)] if fmt == "v210" else []):
        y, u, v = pc.random_planes(16, H, W, fmt, bits)
        rgb = definition_rgb(y, u, v, kind)
        want = reference_pixels(rgb[IDX])
        nbytes = H * pc.row_words(fmt, W) * pc.FORMATS[fmt][0]().itemsize
        for name, src in sources(y, u, v, kind).items():
            for slab in (1, 7):
                stats = {}
                del log[:]
                got = pp.preprocess_selected(src, IDX, towers(), torch.float16, slab, stats=stats)
                assert len(got) == 2
                for g, w in zip(got, want):
                    assert g.is_cuda and tuple(g.shape) == (10, 3, R, R) and memcheck.same_bits(g, w), (name, slab, H, W)
                assert stats == dict(frames_in=16, frames_resized=10, bytes_uploaded=0 if name == "cuda" else 10 * nbytes)
                # one conversion launch per slab, and no planar one
                names = [c[0] for c in log]
                assert names.count("tdc_yuv_packed_to_rgb") == -(-10 // slab)
                assert not any(n in names for n in ("tdc_yuv_to_rgb", "tdc_yuv420_to_rgb", "tdc_yuv_hdr_to_rgb", "tdc_pack_rgb"))
    # idx=None: a device surface is read in place through its strides
    stats = {}
    got = pp.preprocess_selected(sources(y, u, v, kind)["cuda"], None, towers(), torch.float16, 7, stats=stats)
    assert all(memcheck.same_bits(g, w) for g, w in zip(got, reference_pixels(rgb))) and stats["bytes_uploaded"] == 0


def test_a_planar_yuvframes_still_issues_what_it_issued(monkeypatch):
    from tdc_video_amd import lib as L, preprocess as pp
    log = []
    monkeypatch.setattr(L, "_lib", _Traced(L.load(), log))
    y8, u8, v8 = yc.random_planes(16, 90, 160)
    y, u, v = hc.random_planes(16, 90, 160, 10, "422")
    for src, name in ((pp.YuvFrames.i420(y8, u8, v8), "tdc_yuv420_to_rgb"),
                      (pp.YuvFrames.i420(y, u, v, bits=10, subsampling="422"), "tdc_yuv_to_rgb"),
                      (pp.YuvFrames.i420(y, u, v, bits=10, subsampling="422", matrix="bt2020", transfer="pq"), "tdc_yuv_hdr_to_rgb")):
        del log[:]
        pp.preprocess_selected(src, IDX, towers(), torch.float16, 4)
        conversions = [c[0] for c in log if "yuv" in c[0] or c[0] == "tdc_pack_rgb"]
        assert conversions == [name] * 3, (name, conversions)


# ---------------------------------------------------------------------------------------------------- through the engine
@functools.lru_cache(maxsize=None)
def video(kind, H=90, W=160, T0=40):
    """one video of scenes of five frames -> (its packed sources, the planar YuvFrames over host-unpacked planes, the
    definition's RGB frames)"""
    from tdc_video_amd import preprocess as pp
    fmt, bits, _, transfer = FUNNEL[kind]
    y, u, v = pc.random_planes(T0, H, W, fmt, bits, seed=4)
    for t in range(T0):                                           # scenes of five frames, so that the segmentation has cuts to find
        if t % 5:
            y[t] = np.clip(y[t - t % 5].astype(np.int32) + (y[t] % 29).astype(np.int32) - 14, 0, (1 << bits) - 1)
            u[t], v[t] = u[t - t % 5], v[t - t % 5]
    srcs = sources(y, u, v, kind)
    yy, uu, vv = pc.unpack(next(iter(srcs.values())).y.cpu().numpy().view(pc.FORMATS[fmt][0]), fmt, bits, FUNNEL[kind][2], W)
    planes = pp.YuvFrames.i420(yy, uu, vv, bits=bits, subsampling=pc.sub(fmt), matrix="bt601" if bits == 8 else "bt2020", transfer=transfer)
    return srcs, planes, definition_rgb(y, u, v, kind)


@pytest.mark.parametrize("kind", ["yuy2", "v210", "v210_hlg"])
def test_encode_frames_bare_and_oriented_equals_the_planar_call_and_hits_the_cache(fx, kind):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc, pid = fx["enc"], fx["pid"]
    srcs, planes, rgb = video(kind)
    wi, ti = {}, {}
    want = enc.encode_frames(planes, 9, 8, pid, frame_cap=30, info=wi)
    turned = enc.encode_frames(pp.Oriented(planes, rotate=90), 9, 8, pid, frame_cap=30, info=ti)
    c = enc.new_cache(1 << 30)
    i0 = {}
    assert torch.equal(enc.encode_frames(rgb, 9, 8, pid, frame_cap=30, info=i0, cache=c), want)      # first asked as RGB
    assert i0["cache"]["frames_encoded"] == 30
    for name, src in srcs.items():
        gi, oi, hi = {}, {}, {}
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=gi), want), name
        assert gi == wi and gi["frames_resized"] == 30
        assert torch.equal(enc.encode_frames(pp.Oriented(src, rotate=90), 9, 8, pid, frame_cap=30, info=oi), turned), name
        assert oi == ti
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=hi, cache=c), want), name
        assert hi["cache"]["frames_encoded"] == 0 and hi["cache"]["frames_hit"] == hi["cache"]["frames"] == 30
    i1, i2 = {}, {}
    assert torch.equal(enc.encode_frames(srcs["cuda"][3:4], None, 8, None, image=True, info=i1),
                       enc.encode_frames(planes[3:4], None, 8, None, image=True, info=i2)) and i1 == i2
    qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid), dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:])]
    for a, b in zip(enc.encode_frames_prompts(srcs["pinned"], qs, frame_cap=30, pad_fraction=1.0),
                    enc.encode_frames_prompts(planes, qs, frame_cap=30, pad_fraction=1.0)):
        assert torch.equal(a, b)
    w = enc.export_features_from_frames(planes, slab=16)
    g = enc.export_features_from_frames(srcs["cuda"], slab=16)
    assert g.signature == w.signature and memcheck.same_bits(g.siglip, w.siglip) and memcheck.same_bits(g.dino, w.dino)


def test_mixin_frame_inputs_take_a_packed_surface(fx):  # noqa: F811
    srcs, planes, rgb = video("yuy2")
    lm = loaded_lm(fx["W"], fx["o"], tdc_frame_cap=30)
    ids = torch.from_numpy(fx["o"]["input_ids"])
    lm.get_model().tdc_engine().frame_towers = towers()
    lm.get_model().config.tdc_frame_inputs = True
    want = _call(lm, ids, [[rgb], None], (90, 160), [fx["pid"]])
    _same(_call(lm, ids, [[srcs["pinned"]], None], (90, 160), [fx["pid"]]), want)
    _same(_call(lm, ids, [[srcs["cuda"]], [None]], (90, 160), [fx["pid"]]), want)
