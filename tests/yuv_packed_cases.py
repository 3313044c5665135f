"""Helper of the tests of packed YUV input: the memory layout of every packed format as the issue
states it - pack() puts planes into a packed surface with a pitch, a gap between frames, a fill pattern in every byte outside
the read set and random junk in every ignored bit and sample; unpack() is the inverse.  No arithmetic is restated: the
expected RGB is yuv_hibit_cases.to_rgb / yuv_hdr_cases.to_rgb on the unpacked planes.  The product is never imported here."""
from fractions import Fraction

import numpy as np

import yuv_hdr_cases as hd
import yuv_hibit_cases as hc

# name -> (word type of the surface, the order of the four samples of a group or None for a bit field, pixels per group)
FORMATS = {"yuyv": (np.uint8, "yuyv", 2), "yvyu": (np.uint8, "yvyu", 2), "uyvy": (np.uint8, "uyvy", 2), "vyuy": (np.uint8, "vyuy", 2),
           "y210": (np.uint16, "yuyv", 2), "vuya": (np.uint8, "vuya", 1), "ayuv": (np.uint8, "ayuv", 1),
           "y410": (np.uint32, None, 1), "y416": (np.uint16, "uyva", 1), "v210": (np.uint32, None, 6)}
# name -> the (bits, msb_aligned) it takes
DEPTHS = {f: [(8, False)] if t == np.uint8 else ([(10, False)] if t == np.uint32 else [(10, True), (10, False), (12, True), (12, False)])
          for f, (t, _, _) in FORMATS.items()}
# bytes per pixel of a surface whose width is a whole number of groups
BYTES_PER_PIXEL = {"yuyv": 2, "yvyu": 2, "uyvy": 2, "vyuy": 2, "y210": 4, "vuya": 4, "ayuv": 4, "y410": 4, "y416": 8, "v210": Fraction(8, 3)}


def geometry(fmt):
    """(words per group, pixels per group)"""
    return (1 if fmt == "y410" else 4), FORMATS[fmt][2]


def sub(fmt):
    """the chroma sub-sampling of the planes the format unpacks to"""
    return "444" if FORMATS[fmt][2] == 1 else "422"


def row_words(fmt, W):
    """the words of a row's read set: ceil(W / P) whole groups"""
    G, P = geometry(fmt)
    return -(-W // P) * G


def _sample_words(s, dt, bits, msb, rng):
    """samples -> words of the surface's type: 16-bit words hold the sample at either end and junk in the other bits"""
    if dt == np.uint8:
        return s.astype(np.uint8)
    shift = 16 - bits if msb else 0
    w = s.astype(np.uint16) << shift
    if rng is not None:
        w = w | (rng.randint(0, 1 << 16, s.shape).astype(np.uint16) & np.uint16(0xffff ^ (((1 << bits) - 1) << shift)))
    return w.astype(np.uint16)


def pack_rows(y, u, v, fmt, bits, msb=False, junk=None):
    """planes y [T, H, W], u / v [T, H, Wc] -> the rows of the surface [T, H, row_words]; junk (a seed): random samples in the
    unused tail of a last group, random alpha and random bits wherever a word holds none of a sample"""
    dt, order, P = FORMATS[fmt]
    T, H, W = y.shape
    G = geometry(fmt)[0]
    ng = -(-W // P)
    assert u.shape == v.shape == (T,) + hc.chroma_shape(H, W, sub(fmt)) and (bits, msb) in DEPTHS[fmt]
    rng = np.random.RandomState(junk) if junk is not None else None

    def padded(a, n):
        out = (rng.randint(0, 1 << bits, (T, H, n)) if rng is not None else np.zeros((T, H, n), np.int64)).astype(np.uint32)
        out[:, :, :a.shape[2]] = a
        return out

    Y = padded(y, ng * P)
    U, V = (padded(c, ng * P // 2 if P != 1 else ng) for c in (u, v))
    if order is not None:
        g = np.zeros((T, H, ng, 4), dt)
        word = lambda s: _sample_words(s, dt, bits, msb, rng)
        if P == 2:
            first, second = (i for i, ch in enumerate(order) if ch == "y")
            g[..., first], g[..., second] = word(Y[:, :, 0::2]), word(Y[:, :, 1::2])
        else:
            g[..., order.index("y")] = word(Y)
            if rng is not None:
                g[..., order.index("a")] = rng.randint(0, 1 << (8 * dt().itemsize), (T, H, ng)).astype(dt)
        g[..., order.index("u")], g[..., order.index("v")] = word(U), word(V)
        return g.reshape(T, H, ng * 4)
    top = (lambda shape: rng.randint(0, 4, shape).astype(np.uint32) << 30) if rng is not None else (lambda shape: np.uint32(0))
    if fmt == "y410":
        return (U | Y << 10 | V << 20 | top((T, H, ng))).astype(np.uint32)
    Yg, Ug, Vg = Y.reshape(T, H, ng, 6), U.reshape(T, H, ng, 3), V.reshape(T, H, ng, 3)
    g = np.zeros((T, H, ng, 4), np.uint32)
    g[..., 0] = Ug[..., 0] | Yg[..., 0] << 10 | Vg[..., 0] << 20
    g[..., 1] = Yg[..., 1] | Ug[..., 1] << 10 | Yg[..., 2] << 20
    g[..., 2] = Vg[..., 1] | Yg[..., 3] << 10 | Ug[..., 2] << 20
    g[..., 3] = Yg[..., 4] | Vg[..., 2] << 10 | Yg[..., 5] << 20
    return (g | top((T, H, ng, 4))).reshape(T, H, ng * 4).astype(np.uint32)


def unpack(rows, fmt, bits, msb, W):
    """the rows of a surface [T, H, >= row_words] -> the planes (y [T, H, W], u, v [T, H, Wc]); every ignored bit and sample
    is dropped"""
    dt, order, P = FORMATS[fmt]
    T, H = rows.shape[:2]
    ng = -(-W // P)
    assert rows.dtype == dt and rows.shape[2] >= row_words(fmt, W) and (bits, msb) in DEPTHS[fmt]
    mask = (1 << bits) - 1
    out = np.uint8 if bits == 8 else np.uint16
    if order is not None:
        g = rows[:, :, :ng * 4].reshape(T, H, ng, 4).astype(np.uint32)
        s = (g >> (16 - bits if msb else 0)) & mask if dt == np.uint16 else g
        if P == 2:
            first, second = (i for i, ch in enumerate(order) if ch == "y")
            Y = np.stack([s[..., first], s[..., second]], -1).reshape(T, H, ng * 2)
        else:
            Y = s[..., order.index("y")]
        U, V = s[..., order.index("u")], s[..., order.index("v")]
    elif fmt == "y410":
        w = rows[:, :, :ng]
        U, Y, V = w & 1023, w >> 10 & 1023, w >> 20 & 1023
    else:
        g = rows[:, :, :ng * 4].reshape(T, H, ng, 4)
        f = lambda k, i: g[..., k] >> (10 * i) & 1023
        Y = np.stack([f(0, 1), f(1, 0), f(1, 2), f(2, 1), f(3, 0), f(3, 2)], -1).reshape(T, H, ng * 6)
        U = np.stack([f(0, 0), f(1, 1), f(2, 2)], -1).reshape(T, H, ng * 3)
        V = np.stack([f(0, 2), f(2, 0), f(3, 1)], -1).reshape(T, H, ng * 3)
    Wc = hc.chroma_shape(H, W, sub(fmt))[1]
    return Y[:, :, :W].astype(out), U[:, :, :Wc].astype(out), V[:, :, :Wc].astype(out)


class pack:
    """planes into a packed buffer as a capture card or a decoder would lay it out: rows of `pitch` WORDS (default: the
    read set), `gap` words between a frame's end and the next frame's, every byte outside the read set holding `fill`, and -
    junk given - seeded random bits in everything the format ignores.  buf: the flat numpy buffer of the surface's words."""

    def __init__(self, y, u, v, fmt, bits, msb=False, pitch=None, gap=0, fill=0, junk=None):
        self.T, self.H, self.W = T, H, W = y.shape
        self.fmt, self.bits, self.msb = fmt, bits, msb
        self.dtype = FORMATS[fmt][0]
        self.row = row_words(fmt, W)
        self.pitch = self.row if pitch is None else pitch
        assert self.pitch >= self.row
        self.frame = H * self.pitch + gap
        self.buf = np.full(T * self.frame * self.dtype().itemsize, fill, np.uint8).view(self.dtype)
        self.rows()[...] = pack_rows(y, u, v, fmt, bits, msb, junk)

    def rows(self):
        """the read set [T, H, row] as a strided view of buf"""
        b = self.buf.itemsize
        return np.lib.stride_tricks.as_strided(self.buf, (self.T, self.H, self.row), (self.frame * b, self.pitch * b, b))

    def tensor(self, device=None, pin=False):
        """buf as a flat torch tensor over the same bits: uint8, int16 or int32 (bit patterns: every torch has them)"""
        import torch
        t = torch.from_numpy(self.buf.view({1: np.uint8, 2: np.int16, 4: np.int32}[self.buf.itemsize]))
        if pin:
            t = t.pin_memory()
        return t.to(device) if device is not None else t

    def view(self, flat):
        """a flat torch tensor holding buf -> the view [T, H, row] covering exactly the read set"""
        return flat.as_strided((self.T, self.H, self.row), (self.frame, self.pitch, 1), flat.storage_offset())

    def plane(self, flat):
        """a flat torch tensor holding buf -> the whole-pitch surface [T, H, pitch] a caller would wrap"""
        return flat.as_strided((self.T, self.H, self.pitch), (self.frame, self.pitch, 1), flat.storage_offset())


def random_planes(T, H, W, fmt, bits, seed=0):
    return hc.random_planes(T, H, W, bits, sub(fmt), seed)


def to_rgb(y, u, v, coef, fmt, bits):
    """the definition: yuv_hibit_cases.to_rgb on the planes the format unpacks to"""
    return hc.to_rgb(y, u, v, coef, bits, sub(fmt))


def hdr_to_rgb(y, u, v, coef, fmt, bits, tab, desc):
    """the HDR definition: yuv_hdr_cases.to_rgb on the planes the format unpacks to"""
    return hd.to_rgb(y, u, v, coef, bits, sub(fmt), tab, desc)
