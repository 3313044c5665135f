"""Helper of the YUV 4:2:0 tests: the numpy statement of the conversion, the real-valued conversion it
approximates, and the designed inputs - the 2^24 cube and surfaces with pitch padding and gaps between frames.  The product
is never imported here: the coefficient table below is the one the issue states, typed in, not computed."""
import numpy as np

SETTINGS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
#                                   y_off  cy     crv     cgu    cgv    cbu
TABLE = {("bt601", False): (16, 76309, 104597, 25675, 53279, 132201),
         ("bt601", True): (0, 65536, 91881, 22553, 46802, 116130),
         ("bt709", False): (16, 76309, 117489, 13975, 34925, 138438),
         ("bt709", True): (0, 65536, 103206, 12276, 30679, 121609)}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def channels(Y, U, V, coef):
    """the definition on int arrays of one shape: (R, G, B) uint8.  >> on int32 is numpy's arithmetic shift."""
    y_off, cy, crv, cgu, cgv, cbu = coef
    yy = cy * (Y.astype(np.int32) - y_off)
    cb, cr = U.astype(np.int32) - 128, V.astype(np.int32) - 128
    clip8 = lambda a: np.clip(a >> 16, 0, 255).astype(np.uint8)
    return clip8(yy + crv * cr + 32768), clip8(yy - cgu * cb - cgv * cr + 32768), clip8(yy + cbu * cb + 32768)


def to_rgb(y, u, v, coef):
    """y [T, H, W], u / v [T, Hc, Wc] uint8 -> rgb [T, H, W, 3] uint8: pixel (y, x) takes chroma (y >> 1, x >> 1)"""
    T, H, W = y.shape
    assert u.shape == v.shape == (T, (H + 1) // 2, (W + 1) // 2)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)[:, :H, :W]
    return np.stack(channels(y, up(u), up(v), coef), axis=-1)


def real_channels(Y, U, V, matrix, full_range):
    """the real-valued conversion in float64, unrounded and unclipped: (R, G, B)"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y_off, ys, cs = (0, 1.0, 1.0) if full_range else (16, 255.0 / 219.0, 255.0 / 224.0)
    yy = ys * (Y.astype(np.float64) - y_off)
    cb, cr = cs * (U.astype(np.float64) - 128), cs * (V.astype(np.float64) - 128)
    return yy + 2 * (1 - kr) * cr, yy - 2 * (1 - kb) * kb / kg * cb - 2 * (1 - kr) * kr / kg * cr, yy + 2 * (1 - kb) * cb


def cube():
    """all 2^24 (Y, U, V) triples as 64 frames of 512 x 512: chroma runs over every (U, V) pair (U along a row, V down the
    rows), luma is 4*t + 2*(y&1) + (x&1) -> (y [64, 512, 512], u, v [64, 256, 256])"""
    t, yy, xx = np.arange(64)[:, None, None], np.arange(512)[None, :, None], np.arange(512)[None, None, :]
    y = (4 * t + 2 * (yy & 1) + (xx & 1)).astype(np.uint8)
    u = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :], (64, 256, 256)).copy()
    v = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (64, 256, 256)).copy()
    return y, u, v


def random_planes(T, H, W, seed=0):
    """seeded planes with the extremes present: (y [T, H, W], u, v [T, Hc, Wc])"""
    rng = np.random.RandomState(seed + 131 * H + 7 * W + T)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    y, u, v = (rng.randint(0, 256, s).astype(np.uint8) for s in ((T, H, W), (T, Hc, Wc), (T, Hc, Wc)))
    y.flat[0], u.flat[0], v.flat[0] = 255, 0, 255
    y.flat[-1], u.flat[-1], v.flat[-1] = 0, 255, 0
    return y, u, v


class Surface:
    """planes laid out as a decoder would: rows of y_pitch / c_pitch bytes, y_gap / c_gap bytes between a plane's end and the
    next frame's, everything outside the read set holding `fill`.  layout "i420" (two chroma buffers), "nv12" (u first) or
    "nv21" (v first).  bufs: the flat uint8 numpy buffers [y, chroma ...]; views(flat tensors) -> the strided torch views."""

    def __init__(self, y, u, v, layout="nv12", y_pitch=None, c_pitch=None, y_gap=0, c_gap=0, fill=0):
        self.T, self.H, self.W = T, H, W = y.shape
        self.Hc, self.Wc = Hc, Wc = u.shape[1:]
        self.layout, self.c_step = layout, 1 if layout == "i420" else 2
        self.y_pitch = W if y_pitch is None else y_pitch
        self.c_pitch = self.c_step * Wc if c_pitch is None else c_pitch
        assert self.y_pitch >= W and self.c_pitch >= self.c_step * Wc
        self.y_frame, self.c_frame = H * self.y_pitch + y_gap, Hc * self.c_pitch + c_gap
        ybuf = np.full(T * self.y_frame, fill, np.uint8)
        self._strided(ybuf, (T, H, W), (self.y_frame, self.y_pitch, 1))[...] = y
        if layout == "i420":
            cbufs = [np.full(T * self.c_frame, fill, np.uint8) for _ in range(2)]
            for b, c in zip(cbufs, (u, v)):
                self._strided(b, (T, Hc, Wc), (self.c_frame, self.c_pitch, 1))[...] = c
        else:
            cbufs = [np.full(T * self.c_frame, fill, np.uint8)]
            pairs = self._strided(cbufs[0], (T, Hc, Wc, 2), (self.c_frame, self.c_pitch, 2, 1))
            pairs[..., 0], pairs[..., 1] = (u, v) if layout == "nv12" else (v, u)
        self.bufs = [ybuf] + cbufs

    @staticmethod
    def _strided(buf, shape, strides):
        return np.lib.stride_tricks.as_strided(buf, shape, strides)

    def planes(self, flats):
        """flat torch tensors holding bufs -> the whole-pitch planes a caller would wrap: y [T, H, y_pitch], then uv
        [T, Hc, c_pitch] or u, v [T, Hc, c_pitch]"""
        out = [flats[0].as_strided((self.T, self.H, self.y_pitch), (self.y_frame, self.y_pitch, 1))]
        for f in flats[1:]:
            out.append(f.as_strided((self.T, self.Hc, self.c_pitch), (self.c_frame, self.c_pitch, 1)))
        return out

    def views(self, flats):
        """flat torch tensors holding bufs -> (y, u, v) covering exactly the read set, as ops.yuv420_to_rgb takes them"""
        y = flats[0].as_strided((self.T, self.H, self.W), (self.y_frame, self.y_pitch, 1))
        if self.layout == "i420":
            u, v = (f.as_strided((self.T, self.Hc, self.Wc), (self.c_frame, self.c_pitch, 1)) for f in flats[1:])
            return y, u, v
        n = 2 * (self.Wc - 1) + 1
        first, second = (flats[1].as_strided((self.T, self.Hc, n), (self.c_frame, self.c_pitch, 1), flats[1].storage_offset() + o)
                         for o in (0, 1))
        return (y, first, second) if self.layout == "nv12" else (y, second, first)
