"""Helper of the tests of interpolated chroma: the numpy statement of the sited upsampling of a chroma
plane - two taps per sub-sampled axis, weights in quarters, one rounding of the 2-D sum - with its real-valued twin, and the
designed inputs: impulses at every corner, edge and the interior, the 0 / max checkerboard, ramps, and three frames whose
chroma differs in every sample.  The expected RGB is yuv_hibit_cases.to_rgb(..., "444") on the upsampled planes: no colour
arithmetic is restated.  The product is never imported here."""
import numpy as np

import yuv_hibit_cases as hc

# ffmpeg's / H.273's chroma_sample_loc_type -> (sit_x, sit_y): 0 co-sited with the even luma sample, 1 centred between two
SITES = {"left": (0, 1), "center": (1, 1), "topleft": (0, 0), "top": (1, 0)}
SUBS = ("420", "422")


def taps(n_pix, n, sited, sub):
    """the two taps of every position of one axis: (index a, weight a, index b, weight b), weights in quarters"""
    p = np.arange(n_pix)
    if not sub:
        return p, np.full(n_pix, 4), p, np.zeros(n_pix, np.int64)
    k, odd = p >> 1, (p & 1).astype(bool)
    if sited == 0:                                                # sample k sits on position 2k
        return k, np.where(odd, 2, 4), np.minimum(k + 1, n - 1), np.where(odd, 2, 0)
    return k, np.full(n_pix, 3), np.where(odd, np.minimum(k + 1, n - 1), np.maximum(k - 1, 0)), np.full(n_pix, 1)


def weighted(c, H, W, sub, site):
    """the 2-D sum in sixteenths, before the rounding: int64 [T, H, W]"""
    sx, sy = hc.SUB[sub]
    T, Hc, Wc = c.shape
    assert (Hc, Wc) == hc.chroma_shape(H, W, sub)
    ya, wya, yb, wyb = taps(H, Hc, site[1], sy)
    xa, wxa, xb, wxb = taps(W, Wc, site[0], sx)
    c = c.astype(np.int64)
    acc = np.zeros((T, H, W), np.int64)
    for yi, wy in ((ya, wya), (yb, wyb)):
        for xi, wx in ((xa, wxa), (xb, wxb)):
            acc += (wy[:, None] * wx[None, :])[None] * c[:, yi][:, :, xi]
    return acc


def upsample(c, H, W, sub, site):
    """the definition: chroma samples [T, Hc, Wc] -> the interpolated samples [T, H, W], (sum + 8) >> 4 in integers"""
    return ((weighted(c, H, W, sub, site) + 8) >> 4).astype(c.dtype)


def upsample_real(c, H, W, sub, site):
    """the real-valued twin: the same taps, not rounded"""
    return weighted(c, H, W, sub, site) / 16.0


def to_rgb(y, u, v, coef, bits, sub, site):
    """the oracle: the replicate definition on 4:4:4 planes holding the interpolated samples"""
    T, H, W = y.shape
    return hc.to_rgb(y, upsample(u, H, W, sub, site), upsample(v, H, W, sub, site), coef, bits, "444")


# ---------------------------------------------------------------------------------------------------- designed inputs
def _dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def impulses(Hc, Wc, bits):
    """one frame per position of interest - the corners, the middle of each edge, the interior: that sample at max, the rest 0"""
    top = (1 << bits) - 1
    at = sorted({(r, c) for r in (0, Hc // 2, Hc - 1) for c in (0, Wc // 2, Wc - 1)})
    out = np.zeros((len(at), Hc, Wc), _dtype(bits))
    for t, (r, c) in enumerate(at):
        out[t, r, c] = top
    return out


def checkerboard(Hc, Wc, bits):
    """two frames of 0 / max, the second inverted: every rounding of (w * max + 8) >> 4, w = 0 .. 16"""
    top = (1 << bits) - 1
    a = ((np.arange(Hc)[:, None] + np.arange(Wc)[None, :]) & 1) * top
    return np.stack([a, top - a]).astype(_dtype(bits))


def ramps(Hc, Wc, bits):
    """a horizontal and a vertical ramp over the whole range"""
    top = (1 << bits) - 1
    h = np.broadcast_to(np.round(np.linspace(0, top, Wc))[None, :], (Hc, Wc))
    v = np.broadcast_to(np.round(np.linspace(top, 0, Hc))[:, None], (Hc, Wc))
    return np.stack([h, v]).astype(_dtype(bits))


def three_frames(Hc, Wc, bits):
    """three frames whose chroma differs in every sample: a halo taken from the wrong frame shows"""
    top = (1 << bits) - 1
    base = (np.arange(Hc)[:, None] * 37 + np.arange(Wc)[None, :] * 11) % (top // 4)
    return np.stack([base + t * (top // 3) for t in range(3)]).astype(_dtype(bits))


def designed(H, W, bits, sub):
    """name -> (y, u, v): the designed chroma in u, its reverse over the frames in v, seeded luma"""
    Hc, Wc = hc.chroma_shape(H, W, sub)
    out = {}
    for name, c in (("impulses", impulses(Hc, Wc, bits)), ("checkerboard", checkerboard(Hc, Wc, bits)), ("ramps", ramps(Hc, Wc, bits)),
                    ("three_frames", three_frames(Hc, Wc, bits))):
        y = hc.random_planes(c.shape[0], H, W, bits, sub, seed=5)[0]
        out[name] = (y, c, c[::-1].copy())
    return out
