"""The display orientation of DESIGN.md section 23 restated in numpy from its index formulas - what tdc_orient_frames and
preprocess.Oriented are held to.  S is [..., H, W, C]; `rotate` is the clockwise turn that makes the stored frame upright,
`hflip` a left-right mirror after it:
    rotate   0: O[y, x] = S[y, x]                    (H', W') = (H, W)
    rotate  90: O[y, x] = S[H-1-x, y]                (H', W') = (W, H)
    rotate 180: O[y, x] = S[H-1-y, W-1-x]            (H', W') = (H, W)
    rotate 270: O[y, x] = S[x, W-1-y]                (H', W') = (W, H)
    hflip:      O'[y, x] = O[y, W'-1-x]
Written with index arrays, on purpose not with np.rot90 or reversed slices: the tests compare it against those."""
import numpy as np

ROTATIONS = (0, 90, 180, 270)
ALL = [(r, f) for r in ROTATIONS for f in (False, True)]           # the eight elements of the dihedral group
NON_IDENTITY = ALL[1:]
# EXIF orientation -> (rotate, hflip), as DESIGN.md section 23 states it (checked against Pillow in test_orient_inputs.py)
EXIF = {1: (0, False), 2: (0, True), 3: (180, False), 4: (180, True), 5: (90, True), 6: (90, False), 7: (270, True), 8: (270, False)}


def out_hw(H, W, rotate):
    return (W, H) if rotate in (90, 270) else (H, W)


def source_index(H, W, rotate, hflip):
    """(sy, sx): integer arrays [H', W'] with O[y, x] = S[sy[y, x], sx[y, x]]"""
    Ho, Wo = out_hw(H, W, rotate)
    y, x = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    if hflip:                                   # O'[y, x] = O[y, W'-1-x]
        x = Wo - 1 - x
    if rotate == 0:
        return y, x
    if rotate == 90:
        return H - 1 - x, y
    if rotate == 180:
        return H - 1 - y, W - 1 - x
    if rotate == 270:
        return x, W - 1 - y
    raise ValueError(rotate)


def orient(S, rotate, hflip=False):
    """numpy [..., H, W, C] -> contiguous [..., H', W', C]"""
    S = np.asarray(S)
    sy, sx = source_index(S.shape[-3], S.shape[-2], rotate, hflip)
    return np.ascontiguousarray(S[..., sy, sx, :])


def random_frames(T, H, W, seed=0):
    return np.random.RandomState(seed + 131 * H + W).randint(0, 256, (T, H, W, 3)).astype(np.uint8)
