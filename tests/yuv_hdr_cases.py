"""Helper of the tests of HDR YUV input: the numpy statement of the conversion - stage A in int64, stage
B in float64 over a float32-rounded table -, the tables and descriptors it takes, and the case generators (the lattice and the
surfaces are those of yuv_hibit_cases).  The product is never imported here: the constants are the standards' and the
issue's, typed in."""
import math

import numpy as np

import yuv_hibit_cases as hc

TRANSFERS = ("pq", "hlg")
BITS = (10, 12)
# ST 2084
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
# BT.2100 HLG
A, B, C = 0.17883277, 0.28466892, 0.55991073
LUMA = (0.2627, 0.6780, 0.0593)
GAMUT = {"bt2020": (1.6604, -0.5876, -0.0728, -0.1246, 1.1329, -0.0083, -0.0182, -0.1006, 1.1188),
         "bt709": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)}
# (matrix, full_range, bits) -> (y_off, ky, krv, kgu, kgv, kbu): floor(real * 65536 + 0.5), luma scale N / (219 << s) and
# chroma scale N / (224 << s) at limited range, 1 at full range
TABLE = {("bt2020", False, 10): (64, 76533, 110337, 12313, 42752, 140776),
         ("bt2020", False, 12): (256, 76590, 110418, 12322, 42783, 140879),
         ("bt709", True, 10): (0, 65536, 103206, 12276, 30679, 121609),
         ("bt709", True, 12): (0, 65536, 103206, 12276, 30679, 121609)}
SETTINGS = [(m, fr, b) for b in BITS for m in ("bt709", "bt2020") for fr in (False, True)]


def code_coefficients(matrix, full_range, bits):
    """the issue's formula for the stage A coefficients, in double precision"""
    kr, kb = hc.KR_KB[matrix]
    kg = 1.0 - kr - kb
    s, N = bits - 8, (1 << bits) - 1
    ys, cs = (1.0, 1.0) if full_range else (N / float(219 << s), N / float(224 << s))
    real = (ys, 2 * (1 - kr) * cs, 2 * (1 - kb) * kb / kg * cs, 2 * (1 - kr) * kr / kg * cs, 2 * (1 - kb) * cs)
    return (0 if full_range else 16 << s,) + tuple(int(math.floor(r * 65536 + 0.5)) for r in real)


def pq_eotf(e):
    """ST 2084: signal in [0, 1] -> nits (float64)"""
    ep = np.asarray(e, np.float64) ** (1.0 / M2)
    return 10000.0 * (np.maximum(ep - C1, 0.0) / (C2 - C3 * ep)) ** (1.0 / M1)


def hlg_inverse_oetf(e):
    """BT.2100: signal in [0, 1] -> scene light in [0, 1] (float64)"""
    e = np.asarray(e, np.float64)
    return np.where(e <= 0.5, e * e / 3.0, (np.exp((e - C) / A) + B) / 12.0)


def table(transfer, bits, peak=1000.0, white=203.0):
    """code -> light, float32 [2^bits]: built in double precision and rounded once"""
    e = np.arange(1 << bits, dtype=np.float64) / ((1 << bits) - 1)
    return (pq_eotf(e) / white if transfer == "pq" else hlg_inverse_oetf(e)).astype(np.float32)


def descriptor(transfer, primaries="bt2020", peak=1000.0, white=203.0):
    """the scalars of stage B as the C descriptor names them (without the table)"""
    hlg = transfer == "hlg"
    return dict(ootf_scale=peak / white if hlg else 1.0, ootf_exp=0.2 + 0.42 * math.log10(peak / 1000.0) if hlg else 0.0,
                luma=LUMA, inv_p2=(white / peak) ** 2, gamut=GAMUT[primaries])


def codes(Y, U, V, coef, bits):
    """stage A on int arrays of samples of one shape, in int64: (E_R, E_G, E_B) in [0, N], and the largest |accumulator|"""
    y_off, ky, krv, kgu, kgv, kbu = coef
    N = (1 << bits) - 1
    yy = ky * (Y.astype(np.int64) - y_off)
    cb, cr = U.astype(np.int64) - (1 << (bits - 1)), V.astype(np.int64) - (1 << (bits - 1))
    acc = (yy + krv * cr + 32768, yy - kgu * cb - kgv * cr + 32768, yy + kbu * cb + 32768)
    return tuple(np.clip(a >> 16, 0, N) for a in acc), max(int(np.abs(a).max()) for a in acc)


def real_codes(Y, U, V, matrix, full_range, bits):
    """the real-valued conversion to codes in float64, unrounded and unclipped"""
    N = (1 << bits) - 1
    return tuple(c * (N / 255.0) for c in hc.real_channels(Y, U, V, matrix, full_range, bits))


def stage_b(E, tab, desc):
    """codes (E_R, E_G, E_B) -> the three channels on the 0 .. 255 scale before rounding, float64 [3, ...]"""
    lut = tab.astype(np.float64)
    l = np.stack([lut[e] for e in E])
    if desc["ootf_exp"] != 0.0:
        ys = sum(w * c for w, c in zip(desc["luma"], l))
        g = np.zeros_like(ys)
        pos = ys > 0
        g[pos] = desc["ootf_scale"] * ys[pos] ** desc["ootf_exp"]
        l = l * g
    m = l.max(axis=0)
    l = l * ((1.0 + m * desc["inv_p2"]) / (1.0 + m))
    M = np.asarray(desc["gamut"], np.float64).reshape(3, 3)
    x = np.clip(np.tensordot(M, l, axes=1), 0.0, 1.0)
    v = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.maximum(x, 1e-300) ** (1.0 / 2.4) - 0.055)
    return 255.0 * v


def channels(Y, U, V, coef, bits, tab, desc):
    """the definition on int arrays of samples of one shape -> uint8 [..., 3]"""
    E, _ = codes(Y, U, V, coef, bits)
    return np.moveaxis(np.floor(stage_b(E, tab, desc) + 0.5), 0, -1).astype(np.uint8)


def to_rgb(y, u, v, coef, bits, sub, tab, desc):
    """samples y [T, H, W], u / v [T, Hc, Wc] -> rgb [T, H, W, 3] uint8: pixel (y, x) takes chroma (y >> sub_y, x >> sub_x)"""
    T, H, W = y.shape
    sx, sy = hc.SUB[sub]
    assert u.shape == v.shape == (T,) + hc.chroma_shape(H, W, sub)
    up = lambda c: np.repeat(np.repeat(c, 1 << sy, axis=1), 1 << sx, axis=2)[:, :H, :W]
    return channels(y, up(u), up(v), coef, bits, tab, desc)


def grey_axis(coef, bits, tab, desc):
    """every luma code under neutral chroma -> uint8 [2^bits, 3]"""
    Y = np.arange(1 << bits)
    mid = np.full(1 << bits, 1 << (bits - 1))
    return channels(Y, mid, mid, coef, bits, tab, desc)
