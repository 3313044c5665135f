"""The rebuild of a full-height frame from one field of interlaced video restated in numpy from its
formula - what tdc_field_to_frame and preprocess.Interlaced are held to - with the field views of each layout and the random
and designed field pictures the tests share.  F is [..., Hf, W, C], the kept field's rows; p = 0 (top) or 1 (bottom);
cl(i) = min(max(i, 0), Hf - 1); per byte
    O[2k + p]     = F[k]
    O[2k + 1 - p],  m = k - p:
        linear   (F[cl(m)] + F[cl(m+1)] + 1) >> 1
        cubic    clip_0_255((9 (F[cl(m)] + F[cl(m+1)]) - F[cl(m-1)] - F[cl(m+2)] + 8) >> 4)
Written with index arrays and int64 sums (numpy's >> on a negative int64 is an arithmetic shift, and every negative sum clips to
0 whichever way it rounds); test_interlaced_inputs.py checks it against exact rational arithmetic."""
import numpy as np

FIELDS = ("top", "bottom")
FILLS = ("linear", "cubic")
LAYOUTS = ("interleaved", "sequential_tb", "sequential_bt")
RUN = 16                      # csrc/deinterlace.hip: the field rows a thread walks
THREADS, WIDEST = 256, 16     # its workgroup, and the bytes of a thread's column in the widest form


def rebuild(F, parity, fill):
    """numpy uint8 [..., Hf, W, C] -> contiguous uint8 [..., 2 Hf, W, C]"""
    F = np.asarray(F)
    assert F.dtype == np.uint8 and parity in (0, 1) and fill in FILLS
    Hf = F.shape[-3]
    k = np.arange(Hf)
    m = k - parity

    def rows(i):
        return F[..., np.clip(i, 0, Hf - 1), :, :].astype(np.int64)

    if fill == "linear":
        made = (rows(m) + rows(m + 1) + 1) >> 1
    else:
        made = np.clip((9 * (rows(m) + rows(m + 1)) - rows(m - 1) - rows(m + 2) + 8) >> 4, 0, 255)
    O = np.empty(F.shape[:-3] + (2 * Hf,) + F.shape[-2:], np.uint8)
    O[..., 2 * k + parity, :, :] = F
    O[..., 2 * k + 1 - parity, :, :] = made.astype(np.uint8)
    return O


def field_index(n, parity, layout):
    """the rows of field `parity` among the n rows of one plane, as an index array"""
    assert n % 2 == 0 and layout in LAYOUTS
    if layout == "interleaved":
        return np.arange(parity, n, 2)
    first = parity == (0 if layout == "sequential_tb" else 1)
    return np.arange(0, n // 2) if first else np.arange(n // 2, n)


def field_of(plane, parity, layout, axis=1):
    """one plane [T0, rows, ...] (rows on `axis`) -> a dense copy of its rows of field `parity`"""
    return np.ascontiguousarray(np.take(np.asarray(plane), field_index(plane.shape[axis], parity, layout), axis=axis))


def weave(top, bottom, layout):
    """two fields [T0, Hf, ...] -> the frames [T0, 2 Hf, ...] that hold them in `layout`"""
    out = np.empty((top.shape[0], 2 * top.shape[1]) + top.shape[2:], top.dtype)
    out[:, field_index(out.shape[1], 0, layout)] = top
    out[:, field_index(out.shape[1], 1, layout)] = bottom
    return out


def random_fields(T, Hf, W, seed=0):
    return np.random.RandomState(seed + 131 * Hf + W).randint(0, 256, (T, Hf, W, 3)).astype(np.uint8)


# ---- designed field pictures --------------------------------------------------------------------------------------------
def alternating(Hf=12, W=8):
    """[6, Hf, W, 3]: rows alternating 0 / 255 in both phases, and rows 0, 255, 255, 0 in all four phases - the cubic window
    (0, 255, 255, 0) sums to 4598 and clips to 255, (255, 0, 0, 255) to -502 and clips to 0"""
    k = np.arange(Hf)
    cols = [255 * ((k + ph) & 1) for ph in (0, 1)] + [255 * np.isin((k + ph) & 3, (1, 2)) for ph in range(4)]
    F = np.stack([np.broadcast_to(np.asarray(c, np.uint8)[:, None, None], (Hf, W, 3)) for c in cols])
    return np.ascontiguousarray(F)


def constant(value, T=2, Hf=5, W=7):
    return np.full((T, Hf, W, 3), value, np.uint8)


def linear_pairs():
    """[1, 2, 21846, 3]: byte j < 65536 of row 0 holds j >> 8 and of row 1 holds j & 255 - with parity 0 row 1 of the rebuilt
    frame is the mean of every (a, b) pair"""
    j = np.arange(3 * 21846)
    F = np.stack([np.where(j < 65536, j >> 8, 0), np.where(j < 65536, j & 255, 0)]).astype(np.uint8)
    return F.reshape(1, 2, 21846, 3)


CUBIC_FRAMES, CUBIC_W = 4, 21761          # 4 frames of 65283 bytes per row: 261132 >= 511 * 511 columns


def cubic_sums():
    """(s1, s2) of column j of cubic_pairs(): every pair of [0, 510] x [0, 510], then zeros"""
    j = np.arange(CUBIC_FRAMES * 3 * CUBIC_W)
    ok = j < 511 * 511
    return np.where(ok, j // 511, 0), np.where(ok, j % 511, 0)


def cubic_pairs():
    """[4, 4, 21761, 3]: the four rows of column j hold (a, b, c, d) with b + c = s1 and a + d = s2 - with parity 0 row 3 of
    the rebuilt frame (k = 1, m = 1) is the cubic fill of every pair of sums"""
    s1, s2 = cubic_sums()
    b, a = np.minimum(s1, 255), np.minimum(s2, 255)
    F = np.stack([a, b, s1 - b, s2 - a]).astype(np.uint8)                  # [4 rows, frames * bytes]
    return np.ascontiguousarray(F.reshape(4, CUBIC_FRAMES, CUBIC_W, 3).transpose(1, 0, 2, 3))
