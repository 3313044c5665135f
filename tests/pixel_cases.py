"""The pixel layouts of DESIGN.md section 24 restated in numpy from the index formula - what tdc_pack_rgb and
preprocess.RgbFrames are held to.  `data` is [T, H, W, C] ("hwc") or [T, C, H, W] ("chw"), a 3-D [T, H, W] one gray channel;
`order` names the stored channels, one letter each: r, g, b once each or l (gray) once, every other letter an ignored a / x.
    O[t, y, x, c] = data[t, y, x, i_c]  (hwc)        O[t, y, x, c] = data[t, i_c, y, x]  (chw)        c = 0, 1, 2 (R, G, B)
with i_c the position of "rgb"[c] in order, or of l for all three.  Written with explicit per-channel index arrays, on
purpose not with fancy channel lists, reversed slices, transposes or Pillow: the tests compare it against those."""
import numpy as np

COLOUR_ORDERS = ["rgb", "rbg", "grb", "gbr", "brg", "bgr",
                 "rgba", "bgra", "argb", "abgr", "rgbx", "bgrx", "xrgb", "xbgr", "grab"]
GRAY_ORDERS = ["l", "la", "al", "lx", "xl"]
ORDERS = COLOUR_ORDERS + GRAY_ORDERS
LAYOUTS = ("hwc", "chw")


def channel_index(order):
    """(iR, iG, iB): where each output channel is stored"""
    o = order.lower()
    if "l" in o:
        return (o.index("l"),) * 3
    return tuple(o.index(ch) for ch in "rgb")


def to_rgb(data, layout, order):
    """numpy uint8 in the given layout -> contiguous [T, H, W, 3]"""
    data = np.asarray(data)
    if data.ndim == 3:
        data = data[:, :, :, None] if layout == "hwc" else data[:, None]
    T, H, W = (data.shape[0],) + (data.shape[1:3] if layout == "hwc" else data.shape[2:4])
    out = np.empty((T, H, W, 3), np.uint8)
    t, y, x = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    for c, i in enumerate(channel_index(order)):
        out[t, y, x, c] = data[t, y, x, i] if layout == "hwc" else data[t, i, y, x]
    return out


def random_source(T, H, W, layout, order, pitch=0, crop=None, seed=0, junk=None):
    """-> (buffer, view): a flat uint8 numpy buffer and a view [T, H, W, C] / [T, C, H, W] into it, C = len(order).  Rows are
    W * ps + pitch bytes apart (ps = C for hwc, 1 for chw); crop = (top, left, bottom, right) pixels of a larger picture that the
    view leaves out.  The view's own bytes are random; every other byte of the buffer - pitch padding, cropped-away pixels -
    and, with `junk` given, every ignored channel of the view holds `junk` (default: random too)."""
    C = len(order)
    top, left, bottom, right = crop or (0, 0, 0, 0)
    Hf, Wf = H + top + bottom, W + left + right
    rng = np.random.RandomState(seed + 1000 * T + 131 * H + W + 7 * C)
    if layout == "hwc":
        full_shape, rowb = (T, Hf, Wf * C + pitch), Wf * C + pitch
    else:
        full_shape, rowb = (T, C, Hf, Wf + pitch), Wf + pitch
    n = int(np.prod(full_shape))
    buf = rng.randint(0, 256, n).astype(np.uint8) if junk is None else np.full(n, junk, np.uint8)
    full = buf.reshape(full_shape)
    if layout == "hwc":
        view = np.lib.stride_tricks.as_strided(full[:, top:, left * C:], (T, H, W, C), (Hf * rowb, rowb, C, 1))
    else:
        view = full[:, :, top:top + H, left:left + W]
    used = sorted(set(channel_index(order)))
    for i in range(C):
        if junk is None or i in used:
            sub = view[..., i] if layout == "hwc" else view[:, i]
            sub[...] = rng.randint(0, 256, sub.shape).astype(np.uint8)
    return buf, view
