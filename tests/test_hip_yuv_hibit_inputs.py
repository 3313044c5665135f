"""GPU (-m gpu): encode from 10/12-bit and 4:2:2 / 4:4:4 YUV surfaces.  tdc_yuv_to_rgb against the numpy
statement of the conversion (yuv_hibit_cases) - the lattice of every luma value by the chroma values where the arithmetic
turns, every 10-bit (U, V) pair, the shapes where indexing can go wrong in both forms of the kernel, 8-bit 4:2:0 against the
older entry's bytes, its refusals and its memory contract - and the frames funnel on the tiny fixture engine of
test_hip_frame_inputs: everything behind the conversion is the RGB frames path, so every comparison is bit for bit against the
same call on the definition's RGB frames."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import memcheck
import test_hip_memory_contract as contract
import yuv_cases as yc
import yuv_hibit_cases as hc
from test_hip_frame_inputs import IDX, R, fx, reference_pixels, towers  # noqa: F401  (fx: the engine fixture)

pytestmark = pytest.mark.gpu

LAYOUTS = ("uv", "vu", "planar")
# bits, msb_aligned: the alignment only exists for 16-bit words
DEPTHS = [(8, False), (10, False), (10, True), (12, False), (12, True)]


def convert(s, flats, coef, out=None):
    """one tdc_yuv_to_rgb call on the surface s, whose buffers are the flat device tensors `flats`"""
    from tdc_video_amd import ops
    y, u, v = s.views(flats)
    return ops.yuv_to_rgb(y, u, v, s.c_step, coef, s.H, s.W, s.bits, s.msb, s.sub, out=out)


def up16(n):
    return (n + 15) // 16 * 16


def aligned(y, u, v, bits, msb, sub, layout, fill=0xA5, junk=7, gaps=(64, 32)):
    """pitches and frame strides that are multiples of 16 samples: the vector form wherever W % 8 == 0"""
    cs = 1 if layout == "planar" else 2
    Wc = hc.chroma_shape(y.shape[1], y.shape[2], sub)[1]
    return hc.Surface(y, u, v, bits, msb, sub, layout, up16(y.shape[2]) + 16, up16(cs * Wc) + 16, gaps[0], gaps[1], fill, junk)


def ragged(y, u, v, bits, msb, sub, layout, fill=0xA5, junk=8, gaps=(5, 3)):
    """the smallest pitches that leave padding, and gaps that put every frame at another alignment: the one-sample form"""
    cs = 1 if layout == "planar" else 2
    Wc = hc.chroma_shape(y.shape[1], y.shape[2], sub)[1]
    return hc.Surface(y, u, v, bits, msb, sub, layout, y.shape[2] + 3, cs * Wc + 1, gaps[0], gaps[1], fill, junk)


# ---------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("matrix,full_range,bits", hc.SETTINGS)
def test_the_lattice_equals_the_definition(matrix, full_range, bits):
    from tdc_video_amd import preprocess as pp
    coef = pp.yuv_coefficients(matrix, full_range, bits)
    assert coef == hc.TABLE[matrix, full_range, bits]
    y, u, v = hc.lattice(bits)
    want = torch.from_numpy(hc.to_rgb(y, u, v, coef, bits, "444")).cuda()
    for msb in ((False,) if bits == 8 else (False, True)):
        s = aligned(y, u, v, bits, msb, "444", "planar")
        assert torch.equal(convert(s, s.tensors("cuda"), coef), want), msb


@functools.lru_cache(maxsize=None)
def every_pair_on_device():
    y, u, v = hc.every_pair_10()
    s = hc.Surface(y, u, v, 10, True, "420", "uv", junk=3)         # P010 as the decoder writes it
    return (y, u, v), s, s.tensors("cuda")


@pytest.mark.parametrize("matrix,full_range", [("bt2020", False), ("bt709", True)])
def test_every_10_bit_chroma_pair_equals_the_definition(matrix, full_range):
    (y, u, v), s, flats = every_pair_on_device()
    coef = hc.TABLE[matrix, full_range, 10]
    want = torch.from_numpy(hc.to_rgb(y, u, v, coef, 10, "420")).cuda()
    assert torch.equal(convert(s, flats, coef), want)


# ---------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("bits,msb", DEPTHS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 8), (3, 5), (5, 24), (4, 20), (6, 16)])
def test_shapes_pitches_frame_strides_layouts_and_junk(H, W, bits, msb):
    """T = 3 with frame strides larger than the planes and random bits outside the samples.  Aligned pitches and gaps (the
    8-pixel form where W % 8 == 0), the smallest pitches with odd gaps (the one-sample form) and dense planes all equal the
    definition, hence each other."""
    from tdc_video_amd import ops
    coefs = (hc.TABLE["bt2020", False, bits], hc.TABLE["bt709", True, bits])
    for sub in hc.SUB:
        y, u, v = hc.random_planes(3, H, W, bits, sub)
        for k, coef in enumerate(coefs):
            want = torch.from_numpy(hc.to_rgb(y, u, v, coef, bits, sub)).cuda()
            for lay in LAYOUTS:
                for s in (aligned(y, u, v, bits, msb, sub, lay), ragged(y, u, v, bits, msb, sub, lay),
                          hc.Surface(y, u, v, bits, msb, sub, lay, junk=9)):
                    assert torch.equal(convert(s, s.tensors("cuda"), coef), want), (sub, lay, s.y_pitch, s.c_pitch)
                if k == 0:                                        # one frame of three, through the view's offset
                    s = aligned(y, u, v, bits, msb, sub, lay)
                    yv, uv, vv = s.views(s.tensors("cuda"))
                    got = ops.yuv_to_rgb(yv[1:2], uv[1:2], vv[1:2], s.c_step, coef, H, W, bits, msb, sub)
                    assert torch.equal(got, want[1:2]), (sub, lay)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (6, 16), (5, 24)])
def test_8_bit_420_through_the_new_entry_gives_the_old_entrys_bytes(H, W):
    from tdc_video_amd import ops
    y, u, v = yc.random_planes(3, H, W)
    for coef in yc.TABLE.values():
        for lay_old, lay in (("nv12", "uv"), ("nv21", "vu"), ("i420", "planar")):
            for pitches in ((up16(W) + 16, None, 64, 32), (W + 3, None, 5, 3)):
                cs = 1 if lay == "planar" else 2
                c_pitch = up16(cs * ((W + 1) // 2)) + 16 if pitches[0] % 16 == 0 else cs * ((W + 1) // 2) + 1
                old = yc.Surface(y, u, v, lay_old, pitches[0], c_pitch, pitches[2], pitches[3], fill=0x5A)
                new = hc.Surface(y, u, v, 8, False, "420", lay, pitches[0], c_pitch, pitches[2], pitches[3], fill=0x5A)
                assert all(np.array_equal(a, b) for a, b in zip(old.bufs, new.bufs))
                flats = [torch.from_numpy(b).cuda() for b in old.bufs]
                yv, uv, vv = old.views(flats)
                assert torch.equal(convert(new, flats, coef), ops.yuv420_to_rgb(yv, uv, vv, cs, coef, H, W)), (lay, pitches)


# ---------------------------------------------------------------------------------------------------- the memory contract
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  tdc_yuv_to_rgb's is the function below: it is entered
# there under its own name (not a test_ name: that module collects nothing new).
@contract.covers("tdc_yuv_to_rgb")
def yuv_to_rgb_memory_contract(H, W, bits, msb, sub):
    """tdc_yuv_to_rgb: rgb in a guarded arena - nothing outside [T, H, W, 3] changes; the planes in poisoned arenas whose
    pitch padding, sample after an odd chroma row and gaps between frames hold 0x00, then 0xFF - identical output."""
    T = 2
    coef = hc.TABLE["bt709", False, bits]
    y, u, v = hc.random_planes(T, H, W, bits, sub, seed=1)
    want = torch.from_numpy(hc.to_rgb(y, u, v, coef, bits, sub)).cuda()
    for lay in LAYOUTS:
        for make in (aligned, ragged):
            results = []
            for pattern in memcheck.PATTERNS:
                s = make(y, u, v, bits, msb, sub, lay, fill=pattern, junk=4, gaps=(16, 16) if make is aligned else (7, 5))
                flats = [memcheck.poisoned(t, 256, 256, fill=pattern)[0] for t in s.tensors("cuda")]
                out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
                convert(s, flats, coef, out=out)
                torch.cuda.synchronize()
                memcheck.assert_untouched(arena)
                assert torch.equal(out, want), (lay, s.y_pitch, pattern)
                results.append(out.clone())
            assert torch.equal(*results)


contract.yuv_to_rgb_memory_contract = yuv_to_rgb_memory_contract


@pytest.mark.parametrize("bits,msb,sub", [(10, True, "420"), (10, False, "444"), (12, False, "422"), (8, False, "444"), (8, False, "422"),
                                          (12, True, "444")])
@pytest.mark.parametrize("H,W", [(3, 5), (6, 16), (5, 24)])
def test_memory_contract(H, W, bits, msb, sub):
    yuv_to_rgb_memory_contract(H, W, bits, msb, sub)


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
    coef = hc.TABLE["bt2020", False, 10]
    good_c = dict(zip(("y_off", "cy", "crv", "cgu", "cgv", "cbu"), coef))

    def rc(p=None, c=None, dims=(T, H, W), rgb=out.data_ptr(), null=None):
        ps, cs = L.YuvPlanes(**dict(good_p, **(p or {}))), L.YuvCoef(**dict(good_c, **(c or {})))
        return lib.tdc_yuv_to_rgb(None if null == "p" else C.byref(ps), None if null == "c" else C.byref(cs), *dims,
                                  C.c_void_p(rgb), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    # what tdc_yuv420_to_rgb refuses
    bad = [rc(null="p"), rc(null="c"), rc(rgb=0), rc(p=dict(y=0)), rc(p=dict(u=0)), rc(p=dict(v=0))]
    for i in range(3):
        for n in (0, -1, 65536):
            dims = [T, H, W]
            dims[i] = n
            bad.append(rc(dims=tuple(dims)))
    bad += [rc(p=dict(y_pitch=10)), rc(p=dict(c_pitch=10)), rc(p=dict(c_step=2, c_pitch=4)),
            rc(p=dict(y_frame=3 * 16 + 10)), rc(p=dict(c_frame=16 + 8)), rc(p=dict(y_frame=0)), rc(p=dict(c_frame=-16)),
            rc(p=dict(c_step=0)), rc(p=dict(c_step=6)), rc(p=dict(c_step=1)), rc(p=dict(c_step=8)),
            rc(c=dict(y_off=1)), rc(c=dict(y_off=-64)), rc(c=dict(y_off=16)), rc(c=dict(y_off=256))]
    for k in ("cy", "crv", "cgu", "cgv", "cbu"):
        bad += [rc(c={k: -1}), rc(c={k: (1 << 18) + 1})]
    # bits, sub-sampling, alignment of the sample
    bad += [rc(p=dict(bits=b)) for b in (0, 9, 11, 14, 16, -10)]
    bad += [rc(p=dict(sub_x=0, sub_y=1)), rc(p=dict(sub_x=2, sub_y=1)), rc(p=dict(sub_x=1, sub_y=2)), rc(p=dict(sub_x=-1, sub_y=0)),
            rc(p=dict(msb_aligned=2)), rc(p=dict(msb_aligned=-1)),
            rc(p=dict(bits=8, msb_aligned=1, c_step=2, y_pitch=8, c_pitch=8), c=dict(y_off=16))]
    # 16-bit samples: an odd pointer, pitch, frame stride or c_step
    bad += [rc(p=dict(y=yp + 1)), rc(p=dict(u=up + 1, v=up + 3)), rc(p=dict(v=up + 1)), rc(p=dict(y_pitch=17)), rc(p=dict(c_pitch=17)),
            rc(p=dict(y_frame=2 * s.y_frame + 1)), rc(p=dict(c_frame=2 * s.c_frame + 1)), rc(p=dict(c_step=3))]
    # 4:2:2 and 4:4:4 need the chroma rows they name: the 4:2:0 frame stride clears two chroma rows, not four
    bad += [rc(p=dict(sub_y=0)), rc(p=dict(sub_x=0, sub_y=0))]
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad      # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(T, dtype=torch.bool))
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_yuv_to_rgb")
    # the smallest strides that are enough, and the largest coefficients, are taken: at 12 bits their accumulators stay below
    # 2^30 + 2^29 + 2^19, so the int32 bound of the header holds for every set the [0, 2^18] check lets through
    big = dict(cy=1 << 18, cbu=1 << 18, crv=0)
    assert rc(p=dict(y_frame=3 * 16 + 12, c_frame=16 + 10), c=big) == 0
    assert rc(p=dict(bits=12), c=dict(big, y_off=256)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the funnel
KINDS = {"p010": (10, True, "420", "uv"), "yuv444p10le": (10, False, "444", "planar")}
COEF = hc.TABLE["bt2020", False, 10]


def frames_over(s, flats):
    from tdc_video_amd import preprocess as pp
    planes = s.planes(flats)
    if s.msb:
        return pp.YuvFrames.p010(*planes, width=s.W, matrix="bt2020")
    return pp.YuvFrames.i420(*planes, width=s.W, matrix="bt2020", bits=s.bits, subsampling=s.sub)


def sources(y, u, v, kind):
    """the same video as YuvFrames over device surfaces with pitches and gaps, and over dense pinned host planes"""
    a = aligned(y, u, v, *KINDS[kind], fill=0xFF)
    c = hc.Surface(y, u, v, *KINDS[kind], junk=6)
    return {"cuda": frames_over(a, a.tensors("cuda")), "pinned": frames_over(c, c.tensors(pin=True))}


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("H,W", [(90, 160), (45, 81)])
def test_preprocess_selected_on_the_new_kinds_equals_process_images_of_the_definitions_rgb(H, W, kind):
    from tdc_video_amd import preprocess as pp
    bits, _, sub, _ = KINDS[kind]
    y, u, v = hc.random_planes(16, H, W, bits, sub)
    rgb = torch.from_numpy(hc.to_rgb(y, u, v, COEF, bits, sub))
    want = reference_pixels(rgb[IDX])
    want_all = reference_pixels(rgb)
    Hc, Wc = hc.chroma_shape(H, W, sub)
    nbytes = 2 * (H * W + 2 * Hc * Wc)
    for name, src in sources(y, u, v, kind).items():
        for slab in (1, 7, 64):
            stats = {}
            got = pp.preprocess_selected(src, IDX, towers(), torch.float16, slab, stats=stats)
            assert len(got) == 2
            for g, w in zip(got, want):
                assert g.is_cuda and tuple(g.shape) == (10, 3, R, R) and memcheck.same_bits(g, w), (name, slab)
            assert stats == dict(frames_in=16, frames_resized=10, bytes_uploaded=0 if name == "cuda" else 10 * nbytes)
        # idx=None: device surfaces are read in place through their strides, dense pinned planes uploaded as they lie
        stats = {}
        got = pp.preprocess_selected(src, None, towers(), torch.float16, 7, stats=stats)
        assert all(memcheck.same_bits(g, w) for g, w in zip(got, want_all)), name
        assert stats["bytes_uploaded"] == (0 if name == "cuda" else 16 * nbytes)


@functools.lru_cache(maxsize=None)
def video(kind, H=90, W=160, T0=40):
    """(the sources of one video of scenes of five frames, the definition's RGB frames)"""
    bits, _, sub, _ = KINDS[kind]
    y, u, v = hc.random_planes(T0, H, W, bits, sub, seed=4)
    for t in range(T0):                                           # scenes of five frames, so that the segmentation has cuts to find
        if t % 5:
            y[t] = np.clip(y[t - t % 5].astype(np.int32) + (y[t] % 29).astype(np.int32) - 14, 0, (1 << bits) - 1)
            u[t], v[t] = u[t - t % 5], v[t - t % 5]
    return sources(y, u, v, kind), torch.from_numpy(hc.to_rgb(y, u, v, COEF, bits, sub))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_encode_frames_and_a_cache_hit_from_the_rgb_first_call(fx, kind):  # noqa: F811
    enc, pid = fx["enc"], fx["pid"]
    srcs, rgb = video(kind)
    c = enc.new_cache(1 << 30)
    wi = {}
    want = enc.encode_frames(rgb, 9, 8, pid, frame_cap=30, info=wi)
    i0 = {}
    assert torch.equal(enc.encode_frames(rgb, 9, 8, pid, frame_cap=30, info=i0, cache=c), want)
    assert i0["cache"]["frames_encoded"] == 30
    for name, src in srcs.items():
        gi, hi = {}, {}
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=gi), want), name
        assert gi == wi and gi["frames_resized"] == 30
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=hi, cache=c), want), name
        assert hi["cache"]["frames_encoded"] == 0 and hi["cache"]["frames_hit"] == hi["cache"]["frames"] == 30
    i1, i2 = {}, {}
    assert torch.equal(enc.encode_frames(srcs["cuda"][3:4], None, 8, None, image=True, info=i1),
                       enc.encode_frames(rgb[3:4], None, 8, None, image=True, info=i2)) and i1 == i2
