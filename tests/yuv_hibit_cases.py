"""Helper of the tests of YUV input at 8, 10 and 12 bits, 4:2:0 / 4:2:2 / 4:4:4: the numpy statement of
the conversion, the real-valued conversion it approximates, and the designed inputs - the lattice of every luma value by the
chroma values where the arithmetic turns, every 10-bit (U, V) pair, and surfaces of bytes or 16-bit words with pitches, gaps
between frames and junk in the bits a sample does not use.  The product is never imported here: the coefficient table is the
one the issue states, typed in, not computed."""
import numpy as np

import yuv_cases as yc

MATRICES = ("bt601", "bt709", "bt2020")
BITS = (8, 10, 12)
SETTINGS = [(m, fr, b) for b in BITS for m in MATRICES for fr in (False, True)]       # all 18
SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}                                    # name -> (sub_x, sub_y)
KR_KB = dict(yc.KR_KB, bt2020=(0.2627, 0.0593))

#               cy     crv     cgu    cgv    cbu
_LIMITED = {"bt601": yc.TABLE["bt601", False][1:], "bt709": yc.TABLE["bt709", False][1:],
            "bt2020": (76309, 110014, 12277, 42626, 140363)}
_FULL = {("bt601", 8): yc.TABLE["bt601", True][1:], ("bt709", 8): yc.TABLE["bt709", True][1:],
         ("bt2020", 8): (65536, 96639, 10784, 37444, 123299),
         ("bt601", 10): (65344, 91612, 22487, 46664, 115789),
         ("bt709", 10): (65344, 102903, 12240, 30589, 121252),
         ("bt2020", 10): (65344, 96356, 10753, 37334, 122938),
         ("bt601", 12): (65296, 91545, 22471, 46630, 115704),
         ("bt709", 12): (65296, 102828, 12232, 30567, 121163),
         ("bt2020", 12): (65296, 96285, 10745, 37307, 122848)}
# (matrix, full_range, bits) -> (y_off, cy, crv, cgu, cgv, cbu): limited range has the 8-bit coefficients at every depth
TABLE = {(m, fr, b): ((0,) + _FULL[m, b]) if fr else ((16 << (b - 8),) + _LIMITED[m]) for (m, fr, b) in SETTINGS}


def channels(Y, U, V, coef, bits=8):
    """the definition on int arrays of samples of one shape: (R, G, B) uint8.  >> on int32 is numpy's arithmetic shift."""
    y_off, cy, crv, cgu, cgv, cbu = coef
    s = bits - 8
    mid, rnd, down = 1 << (bits - 1), 1 << (15 + s), 16 + s
    yy = np.int32(cy) * (Y.astype(np.int32) - np.int32(y_off))
    cb, cr = U.astype(np.int32) - np.int32(mid), V.astype(np.int32) - np.int32(mid)
    clip8 = lambda a: np.clip(a >> down, 0, 255).astype(np.uint8)
    return (clip8(yy + np.int32(crv) * cr + np.int32(rnd)), clip8(yy - np.int32(cgu) * cb - np.int32(cgv) * cr + np.int32(rnd)),
            clip8(yy + np.int32(cbu) * cb + np.int32(rnd)))


def accumulators(Y, U, V, coef, bits=8):
    """the three accumulators before the shift, in int64: what must fit an int32"""
    y_off, cy, crv, cgu, cgv, cbu = coef
    rnd = 1 << (7 + bits)
    yy = cy * (Y.astype(np.int64) - y_off)
    cb, cr = U.astype(np.int64) - (1 << (bits - 1)), V.astype(np.int64) - (1 << (bits - 1))
    return yy + crv * cr + rnd, yy - cgu * cb - cgv * cr + rnd, yy + cbu * cb + rnd


def chroma_shape(H, W, sub):
    sx, sy = SUB[sub]
    return (H + sy) >> sy, (W + sx) >> sx


def to_rgb(y, u, v, coef, bits=8, sub="420"):
    """samples y [T, H, W], u / v [T, Hc, Wc] -> rgb [T, H, W, 3] uint8: pixel (y, x) takes chroma (y >> sub_y, x >> sub_x)"""
    T, H, W = y.shape
    sx, sy = SUB[sub]
    assert u.shape == v.shape == (T,) + chroma_shape(H, W, sub)
    up = lambda c: np.repeat(np.repeat(c, 1 << sy, axis=1), 1 << sx, axis=2)[:, :H, :W]
    return np.stack(channels(y, up(u), up(v), coef, bits), axis=-1)


def real_channels(Y, U, V, matrix, full_range, bits=8):
    """the real-valued conversion to the 8-bit scale in float64, unrounded and unclipped: (R, G, B)"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    s = bits - 8
    if full_range:
        y_off, ys, cs = 0, 255.0 / ((1 << bits) - 1), 255.0 / ((1 << bits) - 1)
    else:
        y_off, ys, cs = 16 << s, 255.0 / (219 << s), 255.0 / (224 << s)
    yy = ys * (Y.astype(np.float64) - y_off)
    cb, cr = cs * (U.astype(np.float64) - (1 << (bits - 1))), cs * (V.astype(np.float64) - (1 << (bits - 1)))
    return yy + 2 * (1 - kr) * cr, yy - 2 * (1 - kb) * kb / kg * cb - 2 * (1 - kr) * kr / kg * cr, yy + 2 * (1 - kb) * cb


def edge_values(bits):
    """the chroma values where the arithmetic turns: 0, 1, mid - 1, mid, mid + 1, max - 1, max"""
    mid, top = 1 << (bits - 1), (1 << bits) - 1
    return np.array([0, 1, mid - 1, mid, mid + 1, top - 1, top])


def lattice(bits):
    """every luma value under each of the 49 pairs of edge_values as ONE 4:4:4 frame of 49 rows, a row per (U, V) pair and
    the luma value running along it -> samples (y, u, v), each [1, 49, 2^bits]"""
    e = edge_values(bits)
    n = 1 << bits
    dt = np.uint8 if bits == 8 else np.uint16
    y = np.broadcast_to(np.arange(n)[None, None, :], (1, 49, n)).astype(dt)
    u = np.broadcast_to(np.repeat(e, 7)[None, :, None], (1, 49, n)).astype(dt)
    v = np.broadcast_to(np.tile(e, 7)[None, :, None], (1, 49, n)).astype(dt)
    return y, u, v


def every_pair_10():
    """every (U, V) pair of 10 bits as ONE 4:2:0 frame of 2048 x 2048 (2^22 pixels): U along a chroma row, V down the rows,
    and under each pair a 2 x 2 luma block of four different values that between them run over every luma value"""
    yy, xx = np.arange(2048)[None, :, None], np.arange(2048)[None, None, :]
    y = ((37 * yy + 101 * xx + 512 * (yy & 1) + 256 * (xx & 1)) & 1023).astype(np.uint16)
    u = np.broadcast_to(np.arange(1024, dtype=np.uint16)[None, None, :], (1, 1024, 1024)).copy()
    v = np.broadcast_to(np.arange(1024, dtype=np.uint16)[None, :, None], (1, 1024, 1024)).copy()
    return y, u, v


def random_planes(T, H, W, bits=8, sub="420", seed=0):
    """seeded samples with the extremes present: (y [T, H, W], u, v [T, Hc, Wc])"""
    rng = np.random.RandomState(seed + 131 * H + 7 * W + T + 1009 * bits + 17 * len(sub) + int(sub))
    Hc, Wc = chroma_shape(H, W, sub)
    top = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    y, u, v = (rng.randint(0, top + 1, s).astype(dt) for s in ((T, H, W), (T, Hc, Wc), (T, Hc, Wc)))
    y.flat[0], u.flat[0], v.flat[0] = top, 0, top
    y.flat[-1], u.flat[-1], v.flat[-1] = 0, top, 0
    return y, u, v


class Surface:
    """samples laid out as a decoder would: bytes at 8 bits, else 16-bit words with the sample in the high (msb) or the low
    bits and - junk given - seeded random bits everywhere else in the word.  Rows of y_pitch / c_pitch SAMPLES, y_gap / c_gap
    samples between a plane's end and the next frame's, every byte outside the read set holding `fill`.  layout "planar" (two
    chroma buffers), "uv" (interleaved, u first) or "vu" (v first).  bufs: the flat numpy buffers [y, chroma ...]."""

    def __init__(self, y, u, v, bits=8, msb=False, sub="420", layout="uv", y_pitch=None, c_pitch=None, y_gap=0, c_gap=0,
                 fill=0, junk=None):
        self.T, self.H, self.W = T, H, W = y.shape
        self.Hc, self.Wc = Hc, Wc = chroma_shape(H, W, sub)
        assert u.shape == v.shape == (T, Hc, Wc) and not (msb and bits == 8)
        self.bits, self.msb, self.sub, self.layout = bits, msb, sub, layout
        self.c_step = 1 if layout == "planar" else 2
        self.dtype = np.uint8 if bits == 8 else np.uint16
        self.y_pitch = W if y_pitch is None else y_pitch
        self.c_pitch = self.c_step * Wc if c_pitch is None else c_pitch
        assert self.y_pitch >= W and self.c_pitch >= self.c_step * Wc
        self.y_frame, self.c_frame = H * self.y_pitch + y_gap, Hc * self.c_pitch + c_gap
        rng = np.random.RandomState(junk) if junk is not None else None
        y, u, v = (self.words(p, rng) for p in (y, u, v))
        ybuf = self._filled(T * self.y_frame, fill)
        self._strided(ybuf, (T, H, W), (self.y_frame, self.y_pitch, 1))[...] = y
        if layout == "planar":
            cbufs = [self._filled(T * self.c_frame, fill) for _ in range(2)]
            for b, c in zip(cbufs, (u, v)):
                self._strided(b, (T, Hc, Wc), (self.c_frame, self.c_pitch, 1))[...] = c
        else:
            cbufs = [self._filled(T * self.c_frame, fill)]
            pairs = self._strided(cbufs[0], (T, Hc, Wc, 2), (self.c_frame, self.c_pitch, 2, 1))
            pairs[..., 0], pairs[..., 1] = (u, v) if layout == "uv" else (v, u)
        self.bufs = [ybuf] + cbufs

    def words(self, samples, rng=None):
        """samples -> what the surface stores: the sample in its place and, rng given, random bits in the rest of the word"""
        if self.bits == 8:
            return samples.astype(np.uint8)
        shift = 16 - self.bits if self.msb else 0
        w = samples.astype(np.uint16) << shift
        if rng is not None:
            junk = rng.randint(0, 1 << 16, samples.shape).astype(np.uint16)
            w = w | (junk & np.uint16(0xffff ^ (((1 << self.bits) - 1) << shift)))
        return w.astype(np.uint16)

    def _filled(self, n, fill):
        return np.full(n * self.dtype().itemsize, fill, np.uint8).view(self.dtype)

    def _strided(self, buf, shape, strides):
        return np.lib.stride_tricks.as_strided(buf, shape, tuple(s * buf.itemsize for s in strides))

    def tensors(self, device=None, pin=False):
        """bufs as flat torch tensors over the same bits: uint8, or int16 (a bit pattern: every torch has it)"""
        import torch
        out = [torch.from_numpy(b if self.bits == 8 else b.view(np.int16)) for b in self.bufs]
        if pin:
            out = [t.pin_memory() for t in out]
        return [t.to(device) for t in out] if device is not None else out

    def planes(self, flats):
        """flat torch tensors holding bufs -> the whole-pitch planes a caller would wrap: y [T, H, y_pitch], then uv
        [T, Hc, c_pitch] or u, v [T, Hc, c_pitch]"""
        out = [flats[0].as_strided((self.T, self.H, self.y_pitch), (self.y_frame, self.y_pitch, 1), flats[0].storage_offset())]
        for f in flats[1:]:
            out.append(f.as_strided((self.T, self.Hc, self.c_pitch), (self.c_frame, self.c_pitch, 1), f.storage_offset()))
        return out

    def views(self, flats):
        """flat torch tensors holding bufs -> (y, u, v) covering exactly the read set, as ops.yuv_to_rgb takes them"""
        y = flats[0].as_strided((self.T, self.H, self.W), (self.y_frame, self.y_pitch, 1), flats[0].storage_offset())
        if self.layout == "planar":
            u, v = (f.as_strided((self.T, self.Hc, self.Wc), (self.c_frame, self.c_pitch, 1), f.storage_offset()) for f in flats[1:])
            return y, u, v
        n = 2 * (self.Wc - 1) + 1
        first, second = (flats[1].as_strided((self.T, self.Hc, n), (self.c_frame, self.c_pitch, 1), flats[1].storage_offset() + o)
                         for o in (0, 1))
        return (y, first, second) if self.layout == "uv" else (y, second, first)
