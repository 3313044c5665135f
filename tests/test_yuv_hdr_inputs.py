"""CPU: encode from HDR video - PQ / HLG surfaces tone-mapped to SDR.  The anchors of the two transfer
functions, stage A of the definition against the real-valued matrix, the shape of the whole definition along the grey axis,
the product's tables and coefficients against the helper's, the YuvFrames container's new arguments and the routing between
the three conversion entry points."""
import math

import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
import yuv_cases as yc
import yuv_hdr_cases as hd
import yuv_hibit_cases as hc
from tdc_video_amd import ops, preprocess

YuvFrames = preprocess.YuvFrames


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("signal,nits", [(0.5081, 100.02), (0.58069, 203.00), (0.7518, 999.75)])
def test_pq_anchors(signal, nits):
    assert abs(float(hd.pq_eotf(signal)) - nits) <= 0.005         # the printed digits
    assert float(hd.pq_eotf(0.0)) == 0.0 and abs(float(hd.pq_eotf(1.0)) - 10000.0) < 1e-6


def test_hlg_anchor_075_grey_at_peak_1000_is_203_nits_after_the_ootf():
    d = hd.descriptor("hlg", peak=1000.0, white=203.0)
    es = float(hd.hlg_inverse_oetf(0.75))
    ys = sum(d["luma"]) * es
    assert abs(sum(d["luma"]) - 1.0) < 1e-12 and abs(d["ootf_exp"] - 0.2) < 1e-12
    nits = 203.0 * d["ootf_scale"] * ys ** d["ootf_exp"] * es
    assert abs(nits - 203.15) <= 0.005
    assert float(hd.hlg_inverse_oetf(0.0)) == 0.0 and abs(float(hd.hlg_inverse_oetf(0.5)) - 1.0 / 12.0) < 1e-15
    assert abs(float(hd.hlg_inverse_oetf(1.0)) - 1.0) < 1e-7      # the constants are given to eight digits


@pytest.mark.parametrize("transfer", hd.TRANSFERS)
@pytest.mark.parametrize("bits", hd.BITS)
def test_hdr_table_is_the_helpers_table_and_its_scalars_the_descriptors(transfer, bits):
    for peak, white in ((1000.0, 203.0), (4000.0, 100.0)):
        tab, sc = preprocess.hdr_table(transfer, bits, peak, white)
        want = hd.table(transfer, bits, peak, white)
        assert tab.dtype == np.float32 and tab.shape == (1 << bits,) and tab[0] == 0.0 and np.all(np.diff(tab) > 0)
        assert np.allclose(tab, want, rtol=2.0 ** -22, atol=0.0)  # both round a double once: at most two float32 steps apart
        d = hd.descriptor(transfer, "bt2020", peak, white)
        assert set(sc) == {"ootf_scale", "ootf_exp", "luma", "inv_p2"}
        for k in ("ootf_scale", "ootf_exp", "inv_p2"):
            assert abs(sc[k] - d[k]) <= 1e-12 * max(1.0, abs(d[k])), k
        assert tuple(sc["luma"]) == hd.LUMA
        assert (sc["ootf_exp"] == 0.0) == (transfer == "pq")
    assert tuple(preprocess.GAMUT_2020_TO_709) == hd.GAMUT["bt2020"] and tuple(preprocess.GAMUT_IDENTITY) == hd.GAMUT["bt709"]
    for row in np.asarray(hd.GAMUT["bt2020"]).reshape(3, 3):
        assert abs(row.sum() - 1.0) < 1e-15


def test_hdr_table_refusals():
    for args, name in ((("gamma", 10), "transfer"), (("sdr", 10), "transfer"), (("pq", 8), "bits"), (("hlg", 11), "bits"),
                       (("pq", 10, 100.0, 203.0), "peak_nits"), (("pq", 10, 10001.0), "peak_nits"), (("pq", 10, 1000.0, 0.0), "sdr_white"),
                       (("pq", 10, 1000.0, -1.0), "sdr_white"), (("pq", 10, float("nan")), "peak_nits"),
                       (("pq", 10, 1000.0, float("inf")), "sdr_white"), (("pq", 10, "1000"), "peak_nits"),
                       (("hlg", 10, 300.0, 203.0), "peak_nits")):       # system gamma below 1: outside the stated OOTF
        with pytest.raises(ValueError, match=name):
            preprocess.hdr_table(*args)


# ------------------------------------------------------------------------------------------------ stage A
@pytest.mark.parametrize("matrix,full_range,bits", hd.SETTINGS)
def test_stage_a_against_the_real_valued_matrix(matrix, full_range, bits):
    coef = preprocess.yuv_code_coefficients(matrix, full_range, bits)
    assert coef == hd.code_coefficients(matrix, full_range, bits)
    if (matrix, full_range, bits) in hd.TABLE:
        assert coef == hd.TABLE[matrix, full_range, bits]
    s, N = bits - 8, (1 << bits) - 1
    y, u, v = (p[0].astype(np.int64) for p in hc.lattice(bits))
    E, acc = hd.codes(y, u, v, coef, bits)
    for e, r in zip(E, hd.real_codes(y, u, v, matrix, full_range, bits)):
        want = np.clip(np.floor(r + 0.5), 0, N).astype(np.int64)
        assert int(np.abs(e - want).max()) <= 1
    assert acc < 1 << 31
    # the refusal bound of the C entry is an upper bound of every accumulator, and inside int32
    y_off, ky, krv, kgu, kgv, kbu = coef
    assert acc <= (ky << bits) + (max(krv, kgu + kgv, kbu) << (bits - 1)) + (1 << (15 + s)) < 1 << 31
    assert all(0 <= c <= 1 << 18 for c in coef[1:])
    mid = np.array([1 << (bits - 1)])
    if not full_range:
        lo, _ = hd.codes(np.array([16 << s]), mid, mid, coef, bits)
        hi, _ = hd.codes(np.array([235 << s]), mid, mid, coef, bits)
        assert [int(e[0]) for e in lo] == [0, 0, 0] and [int(e[0]) for e in hi] == [N, N, N]
    else:
        assert coef[:2] == (0, 65536)                              # full range: the luma code is the luma sample


def test_yuv_code_coefficients_refusals():
    for args, name in ((("bt470", False, 10), "matrix"), (("bt2020", 1, 10), "full_range"), (("bt2020", False, 9), "bits"),
                       (("bt2020", False, True), "bits")):
        with pytest.raises(ValueError, match=name):
            preprocess.yuv_code_coefficients(*args)


# ------------------------------------------------------------------------------------------------ the definition's shape
@pytest.mark.parametrize("transfer", hd.TRANSFERS)
@pytest.mark.parametrize("bits", hd.BITS)
@pytest.mark.parametrize("matrix,full_range,primaries", [("bt2020", False, "bt2020"), ("bt709", True, "bt709")])
def test_the_definitions_grey_axis(transfer, bits, matrix, full_range, primaries):
    N, s = (1 << bits) - 1, bits - 8
    coef = hd.code_coefficients(matrix, full_range, bits)
    tab, desc = hd.table(transfer, bits), hd.descriptor(transfer, primaries)
    g = hd.grey_axis(coef, bits, tab, desc).astype(np.int64)
    assert np.all(np.diff(g, axis=0) >= 0)                        # non-decreasing in the luma code
    assert int((g.max(axis=1) - g.min(axis=1)).max()) <= 1        # the channels at most 1 apart
    assert g[0].tolist() == [0, 0, 0] and g[coef[0]].tolist() == [0, 0, 0]
    # a grey at peak_nits gives 255: the first code whose light reaches peak / white, HLG's is the top code
    p = 1000.0 / 203.0
    light = tab.astype(np.float64) if transfer == "pq" else desc["ootf_scale"] * tab.astype(np.float64) ** (1.0 + desc["ootf_exp"])
    code = int(np.argmax(light >= p * (1 - 1e-7)))
    assert light[code] >= p * (1 - 1e-7) and (transfer == "pq" or code == N)
    E = (np.array([code]),) * 3
    assert np.floor(hd.stage_b(E, tab, desc) + 0.5).reshape(3).tolist() == [255, 255, 255]
    if not full_range:
        assert g[235 << s].tolist() == [255, 255, 255] and g[N].tolist() == [255, 255, 255]


@pytest.mark.parametrize("transfer", hd.TRANSFERS)
@pytest.mark.parametrize("bits", hd.BITS)
def test_the_definition_is_finite_on_the_lattice_and_at_zero_light(transfer, bits):
    coef = hd.code_coefficients("bt2020", False, bits)
    tab, desc = hd.table(transfer, bits), hd.descriptor(transfer, "bt2020")
    y, u, v = (p[0].astype(np.int64) for p in hc.lattice(bits))
    E, _ = hd.codes(y, u, v, coef, bits)
    assert bool(((E[0] == 0) & (E[1] == 0) & (E[2] == 0)).any())  # Ys = 0 is among the cases
    out = hd.stage_b(E, tab, desc)
    assert np.all(np.isfinite(out)) and out.min() >= 0.0 and out.max() <= 255.0 + 1e-9
    zero = (np.zeros(1, np.int64),) * 3
    assert hd.stage_b(zero, tab, desc).reshape(3).tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ the container
def p010_planes(T=3, H=4, W=6, bits=10):
    y, u, v = hc.random_planes(T, H, W, bits)
    return y, np.stack([u, v], -1).reshape(T, (H + 1) // 2, 2 * ((W + 1) // 2))


def test_yuvframes_takes_the_transfer_on_every_constructor():
    y, uv = p010_planes()
    f = YuvFrames.p010(y, uv, matrix="bt2020", transfer="pq")     # a TypeError before this argument existed
    assert (f.transfer, f.peak_nits, f.sdr_white, f.primaries) == ("pq", 1000.0, 203.0, "bt2020")
    assert f.coef == hd.TABLE["bt2020", False, 10] and f.shape == (3, 4, 6, 3) and preprocess.is_yuv_frames(f)
    d = hd.descriptor("pq", "bt2020")
    assert set(f.hdr) == set(d) and all(f.hdr[k] == pytest.approx(d[k], rel=1e-12) for k in d)
    y12, uv12 = p010_planes(bits=12)
    g = YuvFrames.p016(y12, uv12, bits=12, matrix="bt2020", full_range=True, transfer="hlg", peak_nits=1500, sdr_white=250, primaries="bt709")
    assert (g.transfer, g.peak_nits, g.sdr_white, g.primaries) == ("hlg", 1500, 250, "bt709")
    assert g.coef == hd.code_coefficients("bt2020", True, 12) and tuple(g.hdr["gamut"]) == hd.GAMUT["bt709"]
    assert g.hdr["ootf_exp"] == pytest.approx(0.2 + 0.42 * math.log10(1.5)) and g.hdr["ootf_scale"] == pytest.approx(6.0)
    yy, u, v = hc.random_planes(2, 3, 5, 10, "444")
    for make in (lambda **kw: YuvFrames.i420(yy, u, v, bits=10, subsampling="444", **kw),
                 lambda **kw: YuvFrames.nv12(y, uv, bits=10, msb_aligned=True, **kw),
                 lambda **kw: YuvFrames(y, (uv,), 2, None, "bt709", False, 10, True, "420", **kw)):
        h = make(transfer="hlg")
        assert h.transfer == "hlg" and h.primaries == "bt709" and tuple(h.hdr["gamut"]) == hd.GAMUT["bt709"]
        assert make().transfer == "sdr" and make().hdr is None
    # the defaults of primaries follow the matrix; an SDR YuvFrames is what it was
    assert YuvFrames.p010(y, uv, matrix="bt2020").primaries == "bt2020" and YuvFrames.p010(y, uv, matrix="bt601").primaries == "bt709"
    assert YuvFrames.p010(y, uv, matrix="bt709", transfer="pq", primaries="bt2020").primaries == "bt2020"
    sdr = YuvFrames.p010(y, uv, matrix="bt2020")
    assert sdr.coef == hc.TABLE["bt2020", False, 10] and sdr.transfer == "sdr"
    y8, u8, v8 = yc.random_planes(2, 3, 5)
    assert YuvFrames.i420(y8, u8, v8).transfer == "sdr" and YuvFrames.i420(y8, u8, v8).coef == yc.TABLE["bt601", False]


def test_slicing_keeps_the_new_fields():
    y, uv = p010_planes(T=5)
    f = YuvFrames.p010(y, uv, matrix="bt2020", transfer="hlg", peak_nits=1200.0, sdr_white=180.0, primaries="bt709")
    g = f[1:4]
    assert isinstance(g, YuvFrames) and g.shape == (3, 4, 6, 3) and g.y.data_ptr() == f.y[1].data_ptr()
    assert (g.transfer, g.peak_nits, g.sdr_white, g.primaries, g.coef, g.hdr) == ("hlg", 1200.0, 180.0, "bt709", f.coef, f.hdr)
    assert [tuple(p.shape) for p in g.planes()] == [(3, 4, 6), (3, 2, 6)]
    s = YuvFrames.p010(y, uv)[0:2]
    assert s.transfer == "sdr" and s.hdr is None


def test_yuvframes_refusals_name_the_argument():
    y, uv = p010_planes()
    y8, u8, v8 = yc.random_planes(3, 4, 6)
    bad = [("transfer|bits", lambda: YuvFrames.i420(y8, u8, v8, transfer="pq")),            # HDR at 8 bits
           ("transfer|bits", lambda: YuvFrames.nv12(y8, np.stack([u8, v8], -1).reshape(3, 2, 6), transfer="hlg")),
           ("transfer", lambda: YuvFrames.p010(y, uv, transfer="gamma22")),
           ("transfer", lambda: YuvFrames.p010(y, uv, transfer=None)),
           ("primaries", lambda: YuvFrames.p010(y, uv, transfer="pq", primaries="p3")),
           ("primaries", lambda: YuvFrames.p010(y, uv, primaries="bt601")),
           ("sdr_white", lambda: YuvFrames.p010(y, uv, transfer="pq", sdr_white=0)),
           ("sdr_white", lambda: YuvFrames.p010(y, uv, transfer="pq", sdr_white=-203.0)),
           ("sdr_white", lambda: YuvFrames.p010(y, uv, transfer="pq", sdr_white=float("nan"))),
           ("peak_nits", lambda: YuvFrames.p010(y, uv, transfer="pq", peak_nits=100.0)),   # below sdr_white
           ("peak_nits", lambda: YuvFrames.p010(y, uv, transfer="pq", peak_nits=10000.5)),
           ("peak_nits", lambda: YuvFrames.p010(y, uv, transfer="hlg", peak_nits="1000")),
           ("peak_nits", lambda: YuvFrames.p010(y, uv, transfer="hlg", peak_nits=250.0)),  # HLG system gamma below 1
           ("peak_nits", lambda: YuvFrames.p010(y, uv, peak_nits=50.0))]                   # checked for sdr too
    for name, make in bad:
        with pytest.raises(ValueError, match=name):
            make()
    assert YuvFrames.p010(y, uv, transfer="pq", peak_nits=203.0).hdr["inv_p2"] == 1.0      # the ends of the range are taken
    assert YuvFrames.p010(y, uv, transfer="pq", peak_nits=10000).hdr["inv_p2"] == pytest.approx((203.0 / 10000) ** 2)


# ------------------------------------------------------------------------------------------------ routing
def record(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "yuv420_to_rgb", lambda y, u, v, c_step, coef, H, W, out=None: calls.append(("tdc_yuv420_to_rgb", c_step, coef, H, W)))
    monkeypatch.setattr(ops, "yuv_to_rgb", lambda y, u, v, c_step, coef, H, W, bits=8, msb_aligned=False, subsampling="420", out=None:
                        calls.append(("tdc_yuv_to_rgb", c_step, coef, H, W, bits, msb_aligned, subsampling)))
    monkeypatch.setattr(ops, "yuv_hdr_to_rgb", lambda y, u, v, c_step, coef, H, W, bits, msb_aligned, subsampling, hdr, out=None:
                        calls.append(("tdc_yuv_hdr_to_rgb", c_step, coef, H, W, bits, msb_aligned, subsampling, hdr)))
    return calls


def test_sdr_kinds_issue_what_they_issued(monkeypatch):
    calls = record(monkeypatch)
    y8, u8, v8 = yc.random_planes(2, 4, 6)
    f = YuvFrames.i420(y8, u8, v8)
    f.to_rgb(list(f.planes()), None)
    y, uv = p010_planes(T=2)
    f = YuvFrames.p010(y, uv, matrix="bt2020")
    f.to_rgb(list(f.planes()), None)
    assert calls == [("tdc_yuv420_to_rgb", 1, yc.TABLE["bt601", False], 4, 6),
                     ("tdc_yuv_to_rgb", 2, hc.TABLE["bt2020", False, 10], 4, 6, 10, True, "420")]


@pytest.mark.parametrize("transfer", hd.TRANSFERS)
@pytest.mark.parametrize("bits,msb,sub,layout", [(10, True, "420", "uv"), (12, False, "444", "planar"), (10, False, "422", "vu")])
def test_hdr_kinds_issue_one_hdr_launch_with_the_expected_descriptor(monkeypatch, transfer, bits, msb, sub, layout):
    calls = record(monkeypatch)
    y, u, v = hc.random_planes(2, 4, 6, bits, sub)
    s = hc.Surface(y, u, v, bits, msb, sub, layout)
    planes = s.planes(s.tensors())
    make = YuvFrames.i420 if layout == "planar" else YuvFrames.nv12
    f = make(*planes, width=6, matrix="bt2020", bits=bits, msb_aligned=msb, subsampling=sub, transfer=transfer, peak_nits=1500.0)
    f.to_rgb(list(f.planes()), None)
    f[0:1].to_rgb(list(f[0:1].planes()), None)
    assert len(calls) == 2 and calls[0][:8] == calls[1][:8]
    name, c_step, coef, H, W, b, m, sb, hdr = calls[0]
    assert (name, c_step, coef, H, W, b, m, sb) == ("tdc_yuv_hdr_to_rgb", 1 if layout == "planar" else 2,
                                                    hd.code_coefficients("bt2020", False, bits), 4, 6, bits, msb, sub)
    want = hd.descriptor(transfer, "bt2020", 1500.0, 203.0)
    assert set(hdr) == set(want) | {"lut"}
    for k in want:
        assert hdr[k] == pytest.approx(want[k], rel=1e-12), k
    lut = hdr["lut"]
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (1 << bits,) and lut.device == f.y.device
    assert np.array_equal(lut.numpy(), preprocess.hdr_table(transfer, bits, 1500.0, 203.0)[0])
    assert calls[1][8]["lut"] is lut                              # the device copy is made once per (settings, device), and kept


def test_the_c_abi_declares_the_entry_and_its_descriptor():
    from tdc_video_amd import lib as L
    assert {"tdc_yuv_hdr_to_rgb", "tdc_yuv_to_rgb", "tdc_yuv420_to_rgb"} <= set(L.SIGNATURES)
    assert [n for n, _ in L.HdrDesc._fields_] == ["lut", "ootf_scale", "ootf_exp", "luma", "inv_p2", "gamut"]
    import ctypes as C
    assert C.sizeof(L.HdrDesc) == 72 and L.HdrDesc.gamut.offset == 32 and L.HdrDesc.luma.offset == 16
