"""GPU (-m gpu): encode from HDR video - PQ / HLG surfaces tone-mapped to SDR.  tdc_yuv_hdr_to_rgb
against the numpy definition (yuv_hdr_cases: stage A in integers, stage B in fp64 over the same float32 table) - every byte
within 1, the bound the contract derives -, the shapes, layouts and word alignments where the two kernel forms must give the
same bytes, its memory contract and its refusals; then the frames funnel and the tiny fixture engine of test_hip_frame_inputs:
everything behind the conversion launch is the RGB frames path, so those comparisons are bit for bit against the same call
on the RGB frames the kernel wrote."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import memcheck
import test_hip_memory_contract as contract
import yuv_hdr_cases as hd
import yuv_hibit_cases as hc
from test_hip_frame_inputs import IDX, R, fx, reference_pixels, towers  # noqa: F401  (fx: the engine fixture)
from test_hip_yuv_hibit_inputs import LAYOUTS, aligned, ragged

pytestmark = pytest.mark.gpu

# matrix, full_range, primaries: the two settings of the issue
COLOURS = [("bt2020", False, "bt2020"), ("bt709", True, "bt709")]


@functools.lru_cache(maxsize=None)
def setting(transfer, bits, primaries="bt2020"):
    """(the float32 table, the descriptor with the table on the device) - the helper's own, so that the kernel and the
    definition read the same table"""
    tab = hd.table(transfer, bits)
    return tab, dict(hd.descriptor(transfer, primaries), lut=torch.from_numpy(tab).cuda())


def convert(s, flats, coef, hdr, out=None):
    """one tdc_yuv_hdr_to_rgb call on the surface s, whose buffers are the flat device tensors `flats`"""
    from tdc_video_amd import ops
    y, u, v = s.views(flats)
    return ops.yuv_hdr_to_rgb(y, u, v, s.c_step, coef, s.H, s.W, s.bits, s.msb, s.sub, hdr, out=out)


def worst_and_share(got, want):
    d = (got.cpu().numpy().astype(np.int64) - want.astype(np.int64))
    return int(np.abs(d).max()), float((d != 0).mean())


# ---------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("matrix,full_range,primaries", COLOURS)
@pytest.mark.parametrize("bits", hd.BITS)
@pytest.mark.parametrize("transfer", hd.TRANSFERS)
def test_the_lattice_is_within_1_of_the_definition(transfer, bits, matrix, full_range, primaries):
    coef = hd.code_coefficients(matrix, full_range, bits)
    tab, hdr = setting(transfer, bits, primaries)
    y, u, v = hc.lattice(bits)
    want = hd.to_rgb(y, u, v, coef, bits, "444", tab, hdr)
    got = []
    for msb in (False, True):
        s = aligned(y, u, v, bits, msb, "444", "planar")
        got.append(convert(s, s.tensors("cuda"), coef, hdr))
        worst, share = worst_and_share(got[-1], want)
        print("tdc_yuv_hdr_to_rgb %s %d bits %s %s msb=%d: %d bytes, largest difference %d, differing share %.3g"
              % (transfer, bits, matrix, "full" if full_range else "limited", msb, want.size, worst, share))
        assert worst <= 1
    assert torch.equal(*got)


# ---------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("bits,msb", [(10, False), (10, True), (12, False), (12, True)])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 8), (3, 5), (5, 24), (4, 20), (6, 16)])
def test_shapes_layouts_and_forms_give_the_same_bytes(H, W, bits, msb):
    """T = 2 with frame strides larger than the planes and random bits outside the samples.  Every variant - interleaved in
    both orders, ragged pitches with odd gaps (the one-sample form), dense planes, the other word alignment, one frame
    through a view's offset - equals the aligned planar surface of the same samples (the 8-pixel form where W % 8 == 0), and
    that one is within 1 of the definition."""
    from tdc_video_amd import ops
    for k, (matrix, full_range, primaries) in enumerate(COLOURS):
        coef = hd.code_coefficients(matrix, full_range, bits)
        for transfer in hd.TRANSFERS:
            tab, hdr = setting(transfer, bits, primaries)
            for sub in hc.SUB:
                y, u, v = hc.random_planes(2, H, W, bits, sub)
                base = aligned(y, u, v, bits, msb, sub, "planar")
                ref = convert(base, base.tensors("cuda"), coef, hdr)
                assert worst_and_share(ref, hd.to_rgb(y, u, v, coef, bits, sub, tab, hdr))[0] <= 1, (transfer, sub)
                for lay in LAYOUTS:
                    for s in (aligned(y, u, v, bits, msb, sub, lay), ragged(y, u, v, bits, msb, sub, lay),
                              hc.Surface(y, u, v, bits, msb, sub, lay, junk=9), aligned(y, u, v, bits, not msb, sub, lay, junk=10)):
                        assert torch.equal(convert(s, s.tensors("cuda"), coef, hdr), ref), (transfer, sub, lay, s.y_pitch, s.c_pitch, s.msb)
                    if k == 0 and transfer == "pq":               # one frame of two, through the view's offset
                        s = aligned(y, u, v, bits, msb, sub, lay)
                        yv, uv, vv = s.views(s.tensors("cuda"))
                        got = ops.yuv_hdr_to_rgb(yv[1:2], uv[1:2], vv[1:2], s.c_step, coef, H, W, bits, msb, sub, hdr)
                        assert torch.equal(got, ref[1:2]), (sub, lay)


# ---------------------------------------------------------------------------------------------------- the memory contract
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  tdc_yuv_hdr_to_rgb's is the function below: it is
# entered there under its own name (not a test_ name: that module collects nothing new).
@contract.covers("tdc_yuv_hdr_to_rgb")
def yuv_hdr_to_rgb_memory_contract(H, W, bits, msb, sub, transfer):
    """tdc_yuv_hdr_to_rgb: rgb in a guarded arena - nothing outside [T, H, W, 3] changes; the planes in poisoned arenas
    whose pitch padding, sample after an odd chroma row and gaps between frames hold 0x00, then 0xFF, and the table of
    exactly 2^bits floats in a poisoned arena of its own - identical output."""
    T = 2
    coef = hd.code_coefficients("bt2020", False, bits)
    tab, hdr = setting(transfer, bits)
    y, u, v = hc.random_planes(T, H, W, bits, sub, seed=1)
    plain = aligned(y, u, v, bits, msb, sub, "planar")
    want = convert(plain, plain.tensors("cuda"), coef, hdr)
    assert worst_and_share(want, hd.to_rgb(y, u, v, coef, bits, sub, tab, hdr))[0] <= 1
    for lay in LAYOUTS:
        for make in (aligned, ragged):
            results = []
            for pattern in memcheck.PATTERNS:
                s = make(y, u, v, bits, msb, sub, lay, fill=pattern, junk=4, gaps=(16, 16) if make is aligned else (7, 5))
                flats = [memcheck.poisoned(t, 256, 256, fill=pattern)[0] for t in s.tensors("cuda")]
                lut = memcheck.poisoned(hdr["lut"], 256, 256, fill=pattern)[0]
                out, arena = memcheck.guarded((T, H, W, 3), torch.uint8, "cuda", 1, 1)
                convert(s, flats, coef, dict(hdr, lut=lut), out=out)
                torch.cuda.synchronize()
                memcheck.assert_untouched(arena)
                assert torch.equal(out, want), (lay, s.y_pitch, pattern)
                results.append(out.clone())
            assert torch.equal(*results)


contract.yuv_hdr_to_rgb_memory_contract = yuv_hdr_to_rgb_memory_contract


@pytest.mark.parametrize("bits,msb,sub,transfer", [(10, True, "420", "pq"), (10, False, "444", "hlg"), (12, False, "422", "pq"),
                                                   (12, True, "420", "hlg")])
@pytest.mark.parametrize("H,W", [(3, 5), (6, 16), (5, 24)])
def test_memory_contract(H, W, bits, msb, sub, transfer):
    yuv_hdr_to_rgb_memory_contract(H, W, bits, msb, sub, transfer)


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
    good_c = dict(zip(("y_off", "cy", "crv", "cgu", "cgv", "cbu"), hd.code_coefficients("bt2020", False, 10)))
    _, hlg = setting("hlg", 10)
    lut = hlg["lut"].data_ptr()
    good_h = dict(lut=lut, ootf_scale=hlg["ootf_scale"], ootf_exp=hlg["ootf_exp"], luma=hlg["luma"], inv_p2=hlg["inv_p2"],
                  gamut=hlg["gamut"])
    nan, inf = float("nan"), float("inf")

    def rc(p=None, c=None, h=None, dims=(T, H, W), rgb=out.data_ptr(), null=None):
        hv = dict(good_h, **(h or {}))
        hv["luma"], hv["gamut"] = (C.c_float * 3)(*hv["luma"]), (C.c_float * 9)(*hv["gamut"])
        ps, cs, hs = L.YuvPlanes(**dict(good_p, **(p or {}))), L.YuvCoef(**dict(good_c, **(c or {}))), L.HdrDesc(**hv)
        return lib.tdc_yuv_hdr_to_rgb(None if null == "p" else C.byref(ps), None if null == "c" else C.byref(cs),
                                      None if null == "h" else C.byref(hs), *dims, C.c_void_p(rgb),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))

    # what tdc_yuv_to_rgb refuses
    bad = [rc(null="p"), rc(null="c"), rc(null="h"), rc(rgb=0), rc(p=dict(y=0)), rc(p=dict(u=0)), rc(p=dict(v=0))]
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
    bad += [rc(p=dict(bits=b)) for b in (0, 9, 11, 14, 16, -10)]
    bad += [rc(p=dict(sub_x=0, sub_y=1)), rc(p=dict(sub_x=2, sub_y=1)), rc(p=dict(sub_x=1, sub_y=2)), rc(p=dict(sub_x=-1, sub_y=0)),
            rc(p=dict(msb_aligned=2)), rc(p=dict(msb_aligned=-1))]
    bad += [rc(p=dict(y=yp + 1)), rc(p=dict(u=up + 1, v=up + 3)), rc(p=dict(v=up + 1)), rc(p=dict(y_pitch=17)), rc(p=dict(c_pitch=17)),
            rc(p=dict(y_frame=2 * s.y_frame + 1)), rc(p=dict(c_frame=2 * s.c_frame + 1)), rc(p=dict(c_step=3))]
    bad += [rc(p=dict(sub_y=0)), rc(p=dict(sub_x=0, sub_y=0))]   # the 4:2:0 frame stride does not clear four chroma rows
    # its own: 8 bits, however well formed; the table; the descriptor's floats
    y8 = torch.zeros(T * H * 8 + T * 2 * 8, dtype=torch.uint8, device="cuda")
    bad += [rc(p=dict(y=y8.data_ptr(), u=y8.data_ptr() + T * H * 8, v=y8.data_ptr() + T * H * 8 + 1, bits=8, msb_aligned=0, c_step=2,
                      y_pitch=8, c_pitch=8, y_frame=H * 8, c_frame=2 * 8), c=dict(y_off=16)),
            rc(h=dict(lut=0)), rc(h=dict(lut=lut + 1)), rc(h=dict(lut=lut + 2))]
    for k in ("ootf_scale", "ootf_exp", "inv_p2"):
        bad += [rc(h={k: nan}), rc(h={k: inf}), rc(h={k: -inf})]
    for k, n in (("luma", 3), ("gamut", 9)):
        for i in (0, n - 1):
            for x in (nan, inf):
                vals = list(good_h[k])
                vals[i] = x
                bad.append(rc(h={k: vals}))
    bad += [rc(h=dict(inv_p2=0.0)), rc(h=dict(inv_p2=-0.25)), rc(h=dict(inv_p2=1.0000001)), rc(h=dict(inv_p2=2.0)),
            rc(h=dict(ootf_exp=-0.1)), rc(h=dict(ootf_exp=1.0)), rc(h=dict(ootf_exp=1.5)),
            rc(h=dict(ootf_scale=0.0)), rc(h=dict(ootf_scale=-1.0))]
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad      # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(T, dtype=torch.bool))
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_yuv_hdr_to_rgb")
    # the ends of the ranges are taken: inv_p2 = 1, no OOTF with any scale, the smallest strides that are enough
    assert rc(h=dict(inv_p2=1.0)) == 0 and rc(h=dict(ootf_exp=0.0, ootf_scale=0.0)) == 0 and rc(h=dict(ootf_exp=0.999)) == 0
    assert rc(p=dict(y_frame=3 * 16 + 12, c_frame=16 + 10)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the funnel
KINDS = {"p010_pq": (10, True, "420", "uv", "pq"), "yuv444p12le_hlg": (12, False, "444", "planar", "hlg")}


def frames_over(s, flats, transfer):
    from tdc_video_amd import preprocess as pp
    planes = s.planes(flats)
    if s.msb:
        return pp.YuvFrames.p010(*planes, width=s.W, matrix="bt2020", transfer=transfer)
    return pp.YuvFrames.i420(*planes, width=s.W, matrix="bt2020", bits=s.bits, subsampling=s.sub, transfer=transfer)


def sources(y, u, v, kind, transfer=None):
    """the same video as YuvFrames over device surfaces with pitches and gaps, and over dense pinned host planes"""
    bits, msb, sub, lay, tr = KINDS[kind]
    tr = transfer or tr
    a = aligned(y, u, v, bits, msb, sub, lay, fill=0xFF)
    c = hc.Surface(y, u, v, bits, msb, sub, lay, junk=6)
    return {"cuda": frames_over(a, a.tensors("cuda"), tr), "pinned": frames_over(c, c.tensors(pin=True), tr)}


def kernel_rgb(f):
    """the RGB frames ONE tdc_yuv_hdr_to_rgb launch writes for the device-resident YuvFrames f, through ops"""
    from tdc_video_amd import ops, preprocess as pp
    yv, uv, vv = f.kernel_views(list(f.planes()))
    hdr = dict(f.hdr, lut=pp.hdr_lut(f.transfer, f.bits, f.peak_nits, f.sdr_white, yv.device))
    return ops.yuv_hdr_to_rgb(yv, uv, vv, f.c_step, f.coef, f.shape[1], f.shape[2], f.bits, f.msb_aligned, f.subsampling, hdr)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("H,W", [(90, 160), (45, 81)])
def test_preprocess_selected_equals_process_images_of_the_kernels_rgb(H, W, kind):
    from tdc_video_amd import preprocess as pp
    bits, _, sub, _, _ = KINDS[kind]
    y, u, v = hc.random_planes(16, H, W, bits, sub)
    srcs = sources(y, u, v, kind)
    rgb = kernel_rgb(srcs["cuda"]).cpu()
    want = reference_pixels(rgb[IDX])
    want_all = reference_pixels(rgb)
    for name, src in srcs.items():
        for slab in (1, 7, 64):
            stats = {}
            got = pp.preprocess_selected(src, IDX, towers(), torch.float16, slab, stats=stats)
            assert len(got) == 2
            for g, w in zip(got, want):
                assert g.is_cuda and tuple(g.shape) == (10, 3, R, R) and memcheck.same_bits(g, w), (name, slab)
            assert stats["frames_in"] == 16 and stats["frames_resized"] == 10
        got = pp.preprocess_selected(src, None, towers(), torch.float16, 7)
        assert all(memcheck.same_bits(g, w) for g, w in zip(got, want_all)), name


@functools.lru_cache(maxsize=None)
def video(H=90, W=160, T0=40):
    """one P010 video of scenes of five frames -> its planes' samples"""
    y, u, v = hc.random_planes(T0, H, W, 10, "420", seed=4)
    for t in range(T0):                                           # scenes of five frames, so that the segmentation has cuts to find
        if t % 5:
            y[t] = np.clip(y[t - t % 5].astype(np.int32) + (y[t] % 29).astype(np.int32) - 14, 0, 1023)
            u[t], v[t] = u[t - t % 5], v[t - t % 5]
    return y, u, v


def test_encode_frames_a_cache_hit_and_the_transfer_is_not_ignored(fx):  # noqa: F811
    enc, pid = fx["enc"], fx["pid"]
    y, u, v = video()
    srcs = sources(y, u, v, "p010_pq")
    rgb = kernel_rgb(srcs["cuda"]).cpu()
    wi = {}
    want = enc.encode_frames(rgb, 9, 8, pid, frame_cap=30, info=wi)
    for name, src in srcs.items():
        c = enc.new_cache(1 << 30)
        gi, fi, hi = {}, {}, {}
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=gi), want), name
        assert gi == wi and gi["frames_resized"] == 30
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=fi, cache=c), want), name
        assert fi["cache"]["frames_encoded"] == 30
        assert torch.equal(enc.encode_frames(src, 9, 8, pid, frame_cap=30, info=hi, cache=c), want), name
        assert hi["cache"]["frames_encoded"] == 0 and hi["cache"]["frames_hit"] == hi["cache"]["frames"] == 30
    # the same planes declared SDR are other pixels, so other tokens: the transfer is not silently ignored
    sdr = sources(y, u, v, "p010_pq", transfer="sdr")["cuda"]
    assert sdr.transfer == "sdr" and not torch.equal(enc.encode_frames(sdr, 9, 8, pid, frame_cap=30), want)
    i1, i2 = {}, {}
    assert torch.equal(enc.encode_frames(srcs["cuda"][3:4], None, 8, None, image=True, info=i1),
                       enc.encode_frames(rgb[3:4], None, 8, None, image=True, info=i2)) and i1 == i2
