"""Frame pre-processing on the device: drop-in for the reference's `process_images` (tdc/mm_datautils.py:286-314) on
video frames - uint8 HWC frames in, one fp16/bf16 [T,3,R,R] tensor per tower out (SigLIP 384 / mean 0.5, DINOv2 378 /
ImageNet mean).  The host only builds the small resampling tables (Pillow's Resample.c precompute_coeffs, done in
double precision exactly like the C code) and the 3x256 normalisation table; the pixels never leave the GPU."""
import math

import numpy as np
import torch

from . import lib as L
from . import ops

PRECISION_BITS = 32 - 8 - 2

SIGLIP = dict(R=384, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
DINOV2 = dict(R=378, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_tables(in_size, out_size, support=2.0):
    """Pillow src/libImaging/Resample.c: precompute_coeffs (box = whole axis) + normalize_coeffs_8bpc."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    sup = support * filterscale
    ksize = int(math.ceil(sup)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)
        xmax = min(int(center + sup + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def norm_table(mean, std):
    """lut[c, v] = ((v * 1/255 in float64 -> float32) - mean32[c]) / std32[c]   (HF rescale + normalize)."""
    v = (np.arange(256, dtype=np.float64) * (1.0 / 255.0)).astype(np.float32)
    m = np.array(mean, dtype=np.float32)
    s = np.array(std, dtype=np.float32)
    return ((v[None, :] - m[:, None]) / s[:, None]).astype(np.float32)


_cache = {}


def _tables(S, R, mean, std, device):
    """the resampling tables S -> R and the normalisation table of one tower on `device` (made once per geometry)"""
    key = (S, R, tuple(mean), tuple(std), device)
    if key not in _cache:
        b, k = resize_tables(S, R) if S != R else (np.zeros((1, 2), np.int32), np.zeros((1, 1), np.int32))
        _cache[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device).contiguous(),
                       torch.from_numpy(norm_table(mean, std)).to(device).contiguous())
    return _cache[key]


def preprocess_frames(frames, R, mean, std, dtype=torch.float16, out_f32=False):
    """frames: uint8 tensor [T, H, W, 3] (cpu or cuda) -> [T, 3, R, R] on the GPU."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    frames = frames.cuda().contiguous() if not frames.is_cuda else frames.contiguous()
    T, H, W, _ = frames.shape
    bounds, coeffs, lut = _tables(max(H, W), R, mean, std, frames.device)
    lib = L.load()
    out = torch.empty(T, 3, R, R, device=frames.device, dtype=torch.float32 if out_f32 else dtype)
    nscr = lib.tdc_preprocess_scratch_bytes(T, H, W, R)
    scratch = torch.empty(max(nscr, 1), dtype=torch.uint8, device=frames.device)
    _resize(frames, T, H, W, dict(R=R, mean=mean), (bounds, coeffs, lut), out, dtype, scratch, out_f32)
    return out


def _resize(frames, n, H, W, tower, tables, out, dtype, scratch, out_f32=False):
    """ONE tdc_preprocess_frames launch: n contiguous uint8 [H, W, 3] frames on the GPU -> out [n, 3, R, R] of one tower
    (`tables`: its _tables for max(H, W); `scratch`: tdc_preprocess_scratch_bytes(>= n, H, W, R) bytes)"""
    bounds, coeffs, lut = tables
    pad = [int(x * 255) for x in tower["mean"]]        # expand2square background (tdc/mm_datautils.py:302-304)
    L.check(L.load().tdc_preprocess_frames(ops._ptr(frames), n, H, W, tower["R"], ops._ptr(bounds), ops._ptr(coeffs), coeffs.shape[1],
                                           pad[0], pad[1], pad[2], ops._ptr(lut), ops._ptr(out), int(out_f32),
                                           ops._dtcode(dtype), ops._ptr(scratch), ops._stream()), "tdc_preprocess_frames")


def process_images(frames, dtype=torch.float16, towers=(SIGLIP, DINOV2)):
    """Mirror of tdc/mm_datautils.py process_images for a list / array of video frames: returns one tensor per tower."""
    if not torch.is_tensor(frames):
        frames = torch.from_numpy(np.ascontiguousarray(np.stack(list(frames))))
    return [preprocess_frames(frames, t["R"], t["mean"], t["std"], dtype) for t in towers]


def check_frames(frames):
    """decoded frames as a decoder hands them over -> a uint8 torch tensor [T0, H, W, 3] over the same memory (numpy arrays
    and lists of arrays included); anything else raises ValueError"""
    if not torch.is_tensor(frames):
        a = frames if isinstance(frames, np.ndarray) else np.stack(list(frames))
        if a.dtype != np.uint8:
            raise ValueError("frames must be uint8, got %s" % (a.dtype,))
        if any(s < 0 for s in a.strides):      # a flipped view: torch takes no negative strides
            a = np.ascontiguousarray(a)
        frames = torch.from_numpy(a)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or 0 in frames.shape:
        raise ValueError("frames must be uint8 [T0, H, W, 3] with T0, H, W >= 1, got %s %s" % (frames.dtype, tuple(frames.shape)))
    return frames


def check_indices(idx, T0):
    """the host list of frames to keep out of T0 -> that list as ints, or None when it keeps every frame; anything but
    ascending frame numbers in [0, T0) raises ValueError (the kernels and the gathers behind this trust their indices)"""
    if idx is None:
        return None
    idx = [int(i) for i in idx]
    if not idx:
        raise ValueError("idx keeps no frame")
    if min(idx) < 0 or max(idx) >= T0 or any(b <= a for a, b in zip(idx, idx[1:])):
        raise ValueError("idx must be ascending frame numbers in [0, %d), got %d entries from %d to %d"
                         % (T0, len(idx), min(idx), max(idx)))
    return None if len(idx) == T0 else idx


def selected_frames(frames, idx, device):
    """the frames idx (check_indices) of `frames` (check_frames) as one contiguous uint8 tensor on `device`.  Frames that live
    on the host: the kept ones are gathered into one pinned staging tensor and only they are uploaded - a dropped frame is
    never read or copied; frames on the device are indexed there.  -> (tensor [T, H, W, 3], bytes uploaded)"""
    T0 = frames.shape[0]
    if frames.is_cuda:
        if idx is not None:
            frames = frames[torch.tensor(idx, device=frames.device)]
        return frames.to(device).contiguous(), 0
    if idx is not None or not (frames.is_pinned() and frames.is_contiguous()):
        stage = torch.empty((T0 if idx is None else len(idx),) + tuple(frames.shape[1:]), dtype=torch.uint8, pin_memory=True)
        if idx is None:
            stage.copy_(frames)
        else:
            torch.index_select(frames, 0, torch.tensor(idx), out=stage)
        frames = stage
    return frames.to(device, non_blocking=True), frames.numel()


# ---- YUV frames (DESIGN.md sections 19 and 20) ----------------------------------------------------------------------------
YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}      # (Kr, Kb); bt2020: non-constant luminance
YUV_BITS = (8, 10, 12)


def yuv_coefficients(matrix="bt601", full_range=False, bits=8):
    """(y_off, cy, crv, cgu, cgv, cbu) of tdc_yuv420_to_rgb (bits = 8) and tdc_yuv_to_rgb: floor(real * 65536 + 0.5) of the
    matrix's real coefficients, in double precision.  Limited range: luma 16 .. 235 and chroma 16 .. 240, times 2^(bits - 8) -
    the scales 255/219 and 255/224 and so the coefficients are those of 8 bits at every depth, y_off is 16 << (bits - 8).
    Full range: 0 .. 2^bits - 1 both, one scale 255 * 2^(bits - 8) / (2^bits - 1), which is 1 at 8 bits."""
    _check_matrix_range_bits(matrix, full_range, bits)
    s = bits - 8
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    full =255.0 * (1 << s) / ((1 << bits) - 1)
    ys, cs = (full, full) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    real = (ys, 2 * (1 - kr) * cs, 2 * (1 - kb) * kb / kg * cs, 2 * (1 - kr) * kr / kg * cs, 2 * (1 - kb) * cs)
    return (0 if full_range else 16 << s,) + tuple(int(math.floor(r * 65536 + 0.5)) for r in real)


def _check_matrix_range_bits(matrix, full_range, bits):
    if matrix not in YUV_MATRICES:
        raise ValueError("matrix must be one of %s, got %r" % (sorted(YUV_MATRICES), matrix))
    if not isinstance(full_range, bool):
        raise ValueError("full_range must be True / False, got %r" % (full_range,))
    if isinstance(bits, bool) or bits not in YUV_BITS:
        raise ValueError("bits must be one of %s, got %r" % (YUV_BITS, bits))


def yuv_code_coefficients(matrix="bt2020", full_range=False, bits=10):
    """(y_off, ky, krv, kgu, kgv, kbu) of tdc_yuv_hdr_to_rgb's stage A: YCbCr to non-linear R'G'B' CODES
    at the samples' depth, [0, N] with N = 2^bits - 1, instead of bytes.  floor(real * 65536 + 0.5) in double precision of the
    matrix factors of yuv_coefficients times the luma scale N / (219 << s) and the chroma scale N / (224 << s) (limited range;
    both 1 at full range), s = bits - 8."""
    _check_matrix_range_bits(matrix, full_range, bits)
    s, N = bits - 8, (1 << bits) - 1
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (N / float(219 << s), N / float(224 << s))
    real = (ys, 2 * (1 - kr) * cs, 2 * (1 - kb) * kb / kg * cs, 2 * (1 - kr) * kr / kg * cs, 2 * (1 - kb) * cs)
    return (0 if full_range else 16 << s,) + tuple(int(math.floor(r * 65536 + 0.5)) for r in real)


# ---- HDR transfer functions to SDR -----------------------------------------------------------------
HDR_TRANSFERS = ("pq", "hlg")
YUV_PRIMARIES = ("bt709", "bt2020")
PQ_M1, PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0                              # SMPTE ST 2084
PQ_C1, PQ_C2, PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073                              # BT.2100
BT2020_LUMA = (0.2627, 0.6780, 0.0593)
# BT.2087 BT.2020 -> BT.709 primaries at four digits, each diagonal set so that its row sums to exactly 1 (grey stays grey)
GAMUT_2020_TO_709 = (1.6604, -0.5876, -0.0728, -0.1246, 1.1329, -0.0083, -0.0182, -0.1006, 1.1188)
GAMUT_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def _check_hdr(transfer, bits, peak_nits, sdr_white):
    if transfer not in HDR_TRANSFERS:
        raise ValueError("transfer must be 'sdr' or one of %s, got %r" % (HDR_TRANSFERS, transfer))
    if isinstance(bits, bool) or bits not in (10, 12):
        raise ValueError("transfer %r is taken at bits 10 and 12, got bits %r" % (transfer, bits))
    _check_nits(peak_nits, sdr_white)
    if transfer == "hlg" and not 0.0 < 0.2 + 0.42 * math.log10(peak_nits / 1000.0) < 1.0:
        raise ValueError("peak_nits %r gives the HLG system gamma %.3f: hlg takes a peak whose gamma 1.2 + 0.42 log10(peak / 1000) "
                         "is inside (1, 2), above 334.1 nits" % (peak_nits, 1.2 + 0.42 * math.log10(peak_nits / 1000.0)))


def _check_nits(peak_nits, sdr_white):
    for name, v in (("sdr_white", sdr_white), ("peak_nits", peak_nits)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError("%s must be a finite number of nits, got %r" % (name, v))
    if not 0 < sdr_white:
        raise ValueError("sdr_white must be above 0 nits, got %r" % (sdr_white,))
    if not sdr_white <= peak_nits <= 10000:
        raise ValueError("peak_nits must be in [sdr_white, 10000] = [%r, 10000] nits, got %r" % (sdr_white, peak_nits))


def hdr_table(transfer, bits, peak_nits=1000.0, sdr_white=203.0):
    """(table, scalars) of tdc_yuv_hdr_to_rgb's stage B.  table: numpy float32 [2^bits], code -> light, built in double
    precision and rounded once - pq: 10000 * PQ_EOTF(i / N) / sdr_white, linear light in units of SDR white; hlg: the BT.2100
    inverse OETF of i / N, scene light in [0, 1].  scalars: ootf_scale, ootf_exp (hlg: peak / white and gamma - 1 of the
    BT.2100 OOTF with gamma = 1.2 + 0.42 log10(peak / 1000); pq: 1 and 0, no OOTF), luma, inv_p2 = (white / peak)^2."""
    scalars = _hdr_scalars(transfer, bits, peak_nits, sdr_white)
    e = np.arange(1 << bits, dtype=np.float64) / ((1 << bits) - 1)
    if transfer == "pq":
        ep = e ** (1.0 / PQ_M2)
        table = 10000.0 * (np.maximum(ep - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * ep)) ** (1.0 / PQ_M1) / sdr_white
    else:
        table = np.where(e <= 0.5, e * e / 3.0, (np.exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0)
    return table.astype(np.float32), scalars


def _hdr_scalars(transfer, bits, peak_nits, sdr_white):
    _check_hdr(transfer, bits, peak_nits, sdr_white)
    hlg = transfer == "hlg"
    return dict(ootf_scale=peak_nits / sdr_white if hlg else 1.0, ootf_exp=0.2 + 0.42 * math.log10(peak_nits / 1000.0) if hlg else 0.0,
                luma=BT2020_LUMA, inv_p2=(sdr_white / peak_nits) ** 2)


_HDR_LUTS = {}      # (transfer, bits, peak_nits, sdr_white, device) -> the table on that device: made once, kept


def hdr_lut(transfer, bits, peak_nits, sdr_white, device):
    """hdr_table's table as a float32 tensor on `device`"""
    key = (transfer, bits, float(peak_nits), float(sdr_white), str(torch.device(device)))
    if key not in _HDR_LUTS:
        _HDR_LUTS[key] = torch.from_numpy(hdr_table(transfer, bits, peak_nits, sdr_white)[0]).to(device)
    return _HDR_LUTS[key]


def _plane(p, name, bits=8):
    """one plane as a torch tensor [T0, rows, samples] over the same memory, the last dimension dense: uint8 at bits = 8;
    16-bit words (numpy uint16, torch.uint16 or torch.int16) as torch.int16, a bit pattern the kernel masks its sample out of"""
    kind = "uint8" if bits == 8 else "uint16 (or torch.int16 as a bit pattern)"
    if isinstance(p, np.ndarray):
        if p.dtype != (np.uint8 if bits == 8 else np.uint16):
            raise ValueError("%s must be %s at %d bits, got %s" % (name, kind, bits, p.dtype))
        if any(s < 0 for s in p.strides):
            raise ValueError("%s has a negative stride" % name)
        p = torch.from_numpy(p if bits == 8 else p.view(np.int16))
    if not torch.is_tensor(p):
        raise ValueError("%s must be a %s torch tensor or numpy array, got %s" % (name, kind, type(p).__name__))
    if bits != 8 and p.dtype == getattr(torch, "uint16", None):
        p = p.view(torch.int16)
    if p.dtype != (torch.uint8 if bits == 8 else torch.int16) or p.dim() != 3 or 0 in p.shape:
        raise ValueError("%s must be %s [T0, rows, samples] with no empty dimension at %d bits, got %s %s"
                         % (name, kind, bits, p.dtype, tuple(p.shape)))
    if p.stride(2) != 1 and p.shape[2] > 1:
        raise ValueError("%s: the last dimension must be dense, got stride %d" % (name, p.stride(2)))
    return p


# interpolated chroma: ffmpeg's / H.273's chroma_sample_loc_type -> (sit_x, sit_y), 0 co-sited, 1 centred
CHROMA_UPSAMPLE = ("replicate", "linear")
CHROMA_SITES = {"left": (0, 1), "center": (1, 1), "topleft": (0, 0), "top": (1, 0)}


def _check_chroma(upsample, siting):
    if upsample not in CHROMA_UPSAMPLE:
        raise ValueError("upsample must be one of %s, got %r" % (CHROMA_UPSAMPLE, upsample))
    if siting not in CHROMA_SITES:
        raise ValueError("siting must be one of %s, got %r" % (sorted(CHROMA_SITES), siting))
    return upsample, siting


class YuvFrames:
    """T0 frames of YUV of one size, described and not copied: what a decoder hands over before any colour conversion.
    y is [T0, H, >= W]; the chroma planes have Hc = (H + 1) // 2 rows of Wc = (W + 1) // 2 samples -
    interleaved uv [T0, Hc, >= 2 * Wc] samples (nv12) or planar u, v [T0, Hc, >= Wc] with equal strides (i420).  Planes are
    uint8 torch tensors, all on the host or all on one device, or numpy arrays; row and frame strides may exceed the plane
    (a decoder surface with a pitch and an aligned height, taken as a view) and rows may be longer than `width` (default: the
    luma row length).  matrix "bt601" / "bt709" / "bt2020" and full_range choose the coefficients of the conversion
    (yuv_coefficients), which is the stated formula of include/tdc_hip.h and no decoder library's.  transfer "sdr" (the
    default) leaves the transfer function alone; "pq" or "hlg" (HDR: 10 or 12 bits) converts to SDR sRGB bytes by the stated
    tone mapping of DESIGN.md section 21 (tdc_yuv_hdr_to_rgb) - peak_nits is the mastering peak or MaxCLL (pq) or the nominal
    display peak Lw (hlg, above 334.1 nits), sdr_white the luminance that maps to SDR's diffuse white (203 nits: BT.2408),
    0 < sdr_white <= peak_nits <= 10000; primaries "bt2020" / "bt709" are the source's (None: bt2020 under the bt2020 matrix,
    else bt709) and are converted to BT.709's.  .shape is (T0, H, W, 3), that of the RGB frames the planes convert to;
    yuv[a:b] is a YuvFrames over the same memory.
    Beyond 8-bit 4:2:0: bits 10 or 12 - the planes are 16-bit words (numpy uint16, torch.uint16 where
    torch has it, or torch.int16 as a bit pattern; kept as torch.int16 views), the sample in their high bits (msb_aligned: P010,
    P012, P016) or their low bits (yuv420p10le and its kin); whatever the other bits hold is ignored.  subsampling "422":
    Hc = H, "444": Hc = H and Wc = W.  bt2020 is taken at 10 and 12 bits, the depths it is defined for.
    Packed surfaces - luma and chroma in one row: YUY2, UYVY, Y210, AYUV, Y410, Y416, v210 - are built by
    YuvFrames.packed and its named forms and are PackedYuvFrames, which every consumer of a YuvFrames takes.
    upsample "replicate" (the default) gives pixel (y, x) the chroma sample (y >> sub_y, x >> sub_x); "linear" interpolates the
    chroma samples per axis by where they sit: siting "left" (MPEG-2 / H.264 / HEVC 4:2:0, the default),
    "center" (JPEG, MPEG-1), "topleft" (BT.2020 UHD / HDR10) or "top"; for 4:2:2 only the horizontal half of it matters, and
    on a 4:4:4 surface there is nothing to interpolate.  The siting describes the stored picture and is ignored by "replicate"."""

    def __init__(self, y, chroma, c_step, width=None, matrix="bt601", full_range=False, bits=8, msb_aligned=False,
                 subsampling="420", transfer="sdr", peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        if c_step not in (1, 2):
            raise ValueError("c_step is 1 (planar u, v) or 2 (interleaved uv), got %r" % (c_step,))
        names = ("uv",) if c_step == 2 else ("u", "v")
        if len(chroma) != len(names):
            raise ValueError("c_step %r takes %d chroma plane(s), got %d" % (c_step, len(names), len(chroma)))
        if isinstance(bits, bool) or bits not in YUV_BITS:
            raise ValueError("bits must be one of %s, got %r" % (YUV_BITS, bits))
        if not isinstance(msb_aligned, bool) or (msb_aligned and bits == 8):
            raise ValueError("msb_aligned must be True / False, and False at 8 bits, got %r at %d bits" % (msb_aligned, bits))
        if subsampling not in ops.YUV_SUBSAMPLING:
            raise ValueError("subsampling must be one of %s, got %r" % (sorted(ops.YUV_SUBSAMPLING), subsampling))
        self._colour("planes", matrix=matrix, full_range=full_range, bits=bits, msb_aligned=msb_aligned, transfer=transfer,
                     peak_nits=peak_nits, sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)
        self.y = _plane(y, "y", bits)
        self.chroma = tuple(_plane(c, n, bits) for c, n in zip(chroma, names))
        self.c_step, self.subsampling = c_step, subsampling
        self.sub_x, self.sub_y = ops.YUV_SUBSAMPLING[subsampling]
        T0, H, pitch = self.y.shape
        W = pitch if width is None else int(width)
        if not 1 <= W <= pitch:
            raise ValueError("width must be in [1, %d] (the y rows), got %r" % (pitch, width))
        if T0 > 65535 or H > 65535 or W > 65535:
            raise ValueError("y %s: at most 65535 frames, rows and pixels per row" % (tuple(self.y.shape),))
        Hc, Wc = (H + self.sub_y) >> self.sub_y, (W + self.sub_x) >> self.sub_x
        for c, n in zip(self.chroma, names):
            if c.shape[0] != T0 or c.shape[1] != Hc or c.shape[2] < c_step * Wc:
                raise ValueError("%s must be [%d, %d, >= %d] for y %s and width %d, got %s"
                                 % (n, T0, Hc, c_step * Wc, tuple(self.y.shape), W, tuple(c.shape)))
            if c.device != self.y.device:
                raise ValueError("%s is on %s, y on %s: the planes must share one device" % (n, c.device, self.y.device))
        if len(self.chroma) == 2 and self.chroma[0].stride() != self.chroma[1].stride():
            raise ValueError("u and v must have equal strides, got %s and %s" % (self.chroma[0].stride(), self.chroma[1].stride()))
        self.shape = (T0, H, W, 3)

    def _colour(self, what, matrix, full_range, bits, msb_aligned, transfer, peak_nits, sdr_white, primaries, upsample, siting):
        """the colour half of a constructor, the same for planar and packed surfaces (`what`: "planes" or "surfaces"; bits and
        msb_aligned as the constructor settled them): checks the ten colour parameters, keeps them, and makes .coef and .hdr"""
        self.upsample, self.siting = _check_chroma(upsample, siting)
        if matrix == "bt2020" and bits == 8:
            raise ValueError("matrix bt2020 is taken at 10 and 12 bits, the depths it is defined for; 8-bit %s take %s"
                             % (what, sorted(m for m in YUV_MATRICES if m != "bt2020")))
        if primaries is None:
            primaries = "bt2020" if matrix == "bt2020" else "bt709"
        if primaries not in YUV_PRIMARIES:
            raise ValueError("primaries must be None or one of %s, got %r" % (YUV_PRIMARIES, primaries))
        self.matrix, self.full_range, self.bits, self.msb_aligned = matrix, full_range, bits, msb_aligned
        self.transfer, self.peak_nits, self.sdr_white, self.primaries = transfer, peak_nits, sdr_white, primaries
        if transfer == "sdr":
            _check_nits(peak_nits, sdr_white)
            self.coef, self.hdr = yuv_coefficients(matrix, full_range, bits), None
        else:       # the descriptor of tdc_yuv_hdr_to_rgb but its table, which hdr_on takes from the planes' device
            self.coef = yuv_code_coefficients(matrix, full_range, bits)
            self.hdr = dict(_hdr_scalars(transfer, bits, peak_nits, sdr_white),
                            gamut=GAMUT_2020_TO_709 if primaries == "bt2020" else GAMUT_IDENTITY)

    def colour(self):
        """the ten colour parameters by name, as every constructor takes them"""
        return dict(matrix=self.matrix, full_range=self.full_range, bits=self.bits, msb_aligned=self.msb_aligned,
                    transfer=self.transfer, peak_nits=self.peak_nits, sdr_white=self.sdr_white, primaries=self.primaries,
                    upsample=self.upsample, siting=self.siting)

    def hdr_on(self, device):
        """.hdr with the table of `device` (made once for it) attached, as ops takes the descriptor; None under transfer "sdr" """
        return self.hdr and dict(self.hdr, lut=hdr_lut(self.transfer, self.bits, self.peak_nits, self.sdr_white, device))

    @classmethod
    def nv12(cls, y, uv, width=None, matrix="bt601", full_range=False, bits=8, msb_aligned=False, subsampling="420",
             transfer="sdr", peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """a luma plane and one plane of interleaved (u, v) samples: NV12, and NV16 / NV24 with subsampling "422" / "444" """
        return cls(y, (uv,), 2, width, matrix=matrix, full_range=full_range, bits=bits, msb_aligned=msb_aligned, subsampling=subsampling,
                   transfer=transfer, peak_nits=peak_nits, sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def i420(cls, y, u, v, width=None, matrix="bt601", full_range=False, bits=8, msb_aligned=False, subsampling="420",
             transfer="sdr", peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """three planes: yuv420p, yuv422p, yuv444p and - bits 10 / 12 - their 10le / 12le forms"""
        return cls(y, (u, v), 1, width, matrix=matrix, full_range=full_range, bits=bits, msb_aligned=msb_aligned, subsampling=subsampling,
                   transfer=transfer, peak_nits=peak_nits, sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def p010(cls, y, uv, width=None, matrix="bt601", full_range=False, transfer="sdr", peak_nits=1000.0, sdr_white=203.0,
             primaries=None, upsample="replicate", siting="left"):
        """P010 as a hardware decoder writes it: 4:2:0, 16-bit words, the 10-bit sample in the high bits"""
        return cls(y, (uv,), 2, width, matrix=matrix, full_range=full_range, bits=10, msb_aligned=True, subsampling="420",
                   transfer=transfer, peak_nits=peak_nits, sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def p016(cls, y, uv, bits, width=None, matrix="bt601", full_range=False, transfer="sdr", peak_nits=1000.0, sdr_white=203.0,
             primaries=None, upsample="replicate", siting="left"):
        """a P016 surface holding `bits` (10 or 12) significant bits, MSB-aligned; the low bits are ignored"""
        if isinstance(bits, bool) or bits not in (10, 12):
            raise ValueError("bits of a P016 surface must be 10 or 12, got %r" % (bits,))
        return cls(y, (uv,), 2, width, matrix=matrix, full_range=full_range, bits=bits, msb_aligned=True, subsampling="420",
                   transfer=transfer, peak_nits=peak_nits, sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def packed(cls, data, fmt, width=None, matrix="bt601", full_range=False, bits=None, msb_aligned=None, transfer="sdr",
               peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """a packed surface, luma and chroma in one row: a PackedYuvFrames, which every consumer of a
        YuvFrames takes.  fmt: one of YUV_PACKED_NAMES."""
        return PackedYuvFrames(data, fmt, width, matrix=matrix, full_range=full_range, bits=bits, msb_aligned=msb_aligned, transfer=transfer,
                               peak_nits=peak_nits, sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def yuy2(cls, data, width=None, matrix="bt601", full_range=False, transfer="sdr", peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """YUY2 / YUYV / ffmpeg yuyv422: bytes Y0 U Y1 V"""
        return cls.packed(data, "yuyv", width, matrix=matrix, full_range=full_range, transfer=transfer, peak_nits=peak_nits,
                          sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def uyvy(cls, data, width=None, matrix="bt601", full_range=False, transfer="sdr", peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """UYVY / ffmpeg uyvy422: bytes U Y0 V Y1"""
        return cls.packed(data, "uyvy", width, matrix=matrix, full_range=full_range, transfer=transfer, peak_nits=peak_nits,
                          sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def y210(cls, data, width=None, matrix="bt601", full_range=False, bits=10, msb_aligned=True, transfer="sdr", peak_nits=1000.0,
             sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """Y210 / Y212 / a Y216 container (ffmpeg y210le, y212le): 16-bit words Y0 U Y1 V holding `bits` (10 or 12) bits"""
        return cls.packed(data, "y210", width, matrix=matrix, full_range=full_range, bits=bits, msb_aligned=msb_aligned, transfer=transfer,
                          peak_nits=peak_nits, sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def ayuv(cls, data, width=None, matrix="bt601", full_range=False, transfer="sdr", peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """Microsoft AYUV / VUYX / ffmpeg vuya, vuyx: bytes V U Y A (ffmpeg's `ayuv`, bytes A Y U V, is packed(data, "ayuv"))"""
        return cls.packed(data, "vuya", width, matrix=matrix, full_range=full_range, transfer=transfer, peak_nits=peak_nits,
                          sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def y410(cls, data, width=None, matrix="bt601", full_range=False, transfer="sdr", peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """Y410 / ffmpeg xv30le: one 32-bit word per pixel, U = bits 0-9, Y = 10-19, V = 20-29"""
        return cls.packed(data, "y410", width, matrix=matrix, full_range=full_range, transfer=transfer, peak_nits=peak_nits,
                          sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @classmethod
    def v210(cls, data, width, matrix="bt601", full_range=False, transfer="sdr", peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        """v210: six pixels in four 32-bit words; `width` is required (a row holds whole blocks, often padded to 128 bytes)"""
        return cls.packed(data, "v210", width, matrix=matrix, full_range=full_range, transfer=transfer, peak_nits=peak_nits,
                          sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)

    @property
    def sample_size(self):
        """bytes per sample: 1 at 8 bits, 2 above"""
        return self.y.element_size()

    @property
    def is_420_8bit(self):
        """the kind tdc_yuv420_to_rgb takes (section 19); every other kind goes to tdc_yuv_to_rgb (section 20)"""
        return self.bits == 8 and self.subsampling == "420"

    @property
    def is_cuda(self):
        return self.y.is_cuda

    @property
    def device(self):
        return self.y.device

    @property
    def interpolates(self):
        """upsample "linear" on a surface whose chroma is sub-sampled: on 4:4:4 there is nothing to interpolate"""
        return self.upsample == "linear" and self.sub_x == 1

    def _over(self, cut):
        """a YuvFrames of this kind over cut(plane) of every plane, every other parameter kept: rebuilt through the constructor,
        which checks the view as it checks any planes"""
        return YuvFrames(cut(self.y), tuple(cut(c) for c in self.chroma), self.c_step, self.shape[2], subsampling=self.subsampling,
                         **self.colour())

    def __getitem__(self, s):
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError("YuvFrames takes a slice of frames a:b, got %r" % (s,))
        return self._over(lambda p: p[s])

    def field(self, parity, layout="interleaved"):
        """one field of interlaced frames: a YuvFrames (packed: a PackedYuvFrames) over the same memory
        whose planes hold every plane's rows of field `parity` (field_rows), every other parameter kept - a half-height picture
        of the same kind"""
        return self._over(lambda p: p[:, field_rows(p.shape[1], parity, layout)])

    def planes(self):
        """the read set as views: (y [T0, H, W], one or two chroma planes [T0, Hc, c_step * Wc]) - the pitch padding cut off"""
        W = self.shape[2]
        return (self.y[:, :, :W],) + tuple(c[:, :, :self.c_step * ((W + self.sub_x) >> self.sub_x)] for c in self.chroma)

    def kernel_views(self, planes):
        """(y, u, v) as ops.yuv420_to_rgb and ops.yuv_to_rgb take them, from `planes` laid out like planes()"""
        return (planes[0], planes[1], planes[1][:, :, 1:]) if self.c_step == 2 else tuple(planes)

    def to_rgb(self, planes, out):
        """ONE conversion launch: the frames of `planes` (device planes laid out like planes()) -> out uint8 [T, H, W, 3].
        8-bit 4:2:0 issues tdc_yuv420_to_rgb as it always did; every other SDR kind issues tdc_yuv_to_rgb; transfer "pq" / "hlg"
        issues tdc_yuv_hdr_to_rgb, its table taken from (and made once for) the planes' device.  upsample "linear" on a 4:2:0 or
        4:2:2 surface issues tdc_yuv_linear_to_rgb in their place."""
        y, u, v = self.kernel_views(planes)
        H, W = self.shape[1:3]
        hdr = self.hdr_on(y.device)
        if self.interpolates:
            return ops.yuv_linear_to_rgb(y, u, v, self.c_step, self.coef, H, W, self.bits, self.msb_aligned, self.subsampling,
                                         CHROMA_SITES[self.siting], hdr=hdr, out=out)
        if hdr is not None:
            return ops.yuv_hdr_to_rgb(y, u, v, self.c_step, self.coef, H, W, self.bits, self.msb_aligned, self.subsampling, hdr, out=out)
        if self.is_420_8bit:
            return ops.yuv420_to_rgb(y, u, v, self.c_step, self.coef, H, W, out=out)
        return ops.yuv_to_rgb(y, u, v, self.c_step, self.coef, H, W, self.bits, self.msb_aligned, self.subsampling, out=out)


# ---- packed YUV surfaces ----------------------------------------------------------------------------
# name -> (the kernel's format, default bits, the depths the name takes)
YUV_PACKED_NAMES = {"yuyv": ("yuyv", 8, (8,)), "yuy2": ("yuyv", 8, (8,)), "yvyu": ("yvyu", 8, (8,)), "uyvy": ("uyvy", 8, (8,)),
                    "vyuy": ("vyuy", 8, (8,)), "y210": ("y210", 10, (10, 12)), "y212": ("y210", 12, (12,)), "y216": ("y210", None, (10, 12)),
                    "vuya": ("vuya", 8, (8,)), "vuyx": ("vuya", 8, (8,)), "ayuv": ("ayuv", 8, (8,)), "y410": ("y410", 10, (10,)),
                    "y412": ("y416", 12, (12,)), "y416": ("y416", None, (10, 12)), "v210": ("v210", 10, (10,))}


def _packed_words(p, fmt, ws):
    """a packed surface as a torch tensor [T0, H, words] over the same memory, the last dimension dense: uint8 for the byte
    formats, 16-bit words as _plane keeps them (torch.int16), 32-bit words (numpy uint32, torch.uint32 or torch.int32) as
    torch.int32 - bit patterns the kernel takes its samples out of"""
    np_dt, t_dt, kind = {1: (np.uint8, torch.uint8, "uint8"), 2: (np.uint16, torch.int16, "uint16 (or torch.int16 as a bit pattern)"),
                         4: (np.uint32, torch.int32, "uint32 (or torch.int32 as a bit pattern)")}[ws]
    if isinstance(p, np.ndarray):
        if p.dtype != np_dt:
            raise ValueError("data must be %s for fmt %r, got %s" % (kind, fmt, p.dtype))
        if any(s < 0 for s in p.strides):
            raise ValueError("data has a negative stride")
        p = torch.from_numpy(p if ws == 1 else p.view({2: np.int16, 4: np.int32}[ws]))
    if not torch.is_tensor(p):
        raise ValueError("data must be a %s torch tensor or numpy array for fmt %r, got %s" % (kind, fmt, type(p).__name__))
    if ws != 1 and p.dtype == getattr(torch, "uint%d" % (8 * ws), None):
        p = p.view(t_dt)
    if p.dtype != t_dt or p.dim() != 3 or 0 in p.shape:
        raise ValueError("data must be %s [T0, H, row] with no empty dimension for fmt %r, got %s %s" % (kind, fmt, p.dtype, tuple(p.shape)))
    if p.stride(2) != 1 and p.shape[2] > 1:
        raise ValueError("data: the last dimension must be dense, got stride %d" % p.stride(2))
    return p


class PackedYuvFrames(YuvFrames):
    """T0 frames of packed YUV of one size, described and not copied (YuvFrames.packed and its named forms): ONE surface
    `data` [T0, H, row] whose rows hold luma and chroma together - uint8 for the byte formats (yuyv / yuy2, yvyu, uyvy, vyuy:
    4:2:2; vuya / vuyx, ayuv: 4:4:4), 16-bit words for y210 / y212 / y216 (4:2:2) and y412 / y416 (4:4:4), 32-bit words for
    y410 and v210 - on the host or the device, with any row and frame stride.  A row holds ceil(width / P) whole groups of P
    pixels; width defaults to the row's whole groups times P and is required for v210.  bits defaults to the name's (y216 and
    y416 are containers: give 10 or 12), msb_aligned to True for the 16-bit-word formats.  Everything else is YuvFrames': the
    matrix, the range, the transfer (pq / hlg at 10 and 12 bits), .shape, slicing, and the members its consumers use - .y is
    the surface, planes() one view of it cut to the read set, to_rgb ONE tdc_yuv_packed_to_rgb launch."""

    def __init__(self, data, fmt, width=None, matrix="bt601", full_range=False, bits=None, msb_aligned=None, transfer="sdr",
                 peak_nits=1000.0, sdr_white=203.0, primaries=None, upsample="replicate", siting="left"):
        if fmt not in YUV_PACKED_NAMES:
            raise ValueError("fmt must be one of %s, got %r" % (sorted(YUV_PACKED_NAMES), fmt))
        self.name = fmt
        self.fmt, default_bits, depths = YUV_PACKED_NAMES[fmt]
        ws, per_group, P, _ = ops.YUV_PACKED[self.fmt]
        if bits is None:
            bits = default_bits
        if isinstance(bits, bool) or bits not in depths:
            raise ValueError("bits of fmt %r must be %s, got %r" % (fmt, " or ".join(str(b) for b in depths), bits))
        if msb_aligned is None:
            msb_aligned = ws == 2
        if not isinstance(msb_aligned, bool) or (msb_aligned and ws != 2):
            raise ValueError("msb_aligned must be True / False, and False for fmt %r (it places a sample in a 16-bit word), got %r"
                             % (fmt, msb_aligned))
        self._colour("surfaces", matrix=matrix, full_range=full_range, bits=bits, msb_aligned=msb_aligned, transfer=transfer,
                     peak_nits=peak_nits, sdr_white=sdr_white, primaries=primaries, upsample=upsample, siting=siting)
        self.y = _packed_words(data, fmt, ws)
        self.chroma, self.c_step = (), 0
        self.subsampling = "422" if P != 1 else "444"
        self.sub_x, self.sub_y = ops.YUV_SUBSAMPLING[self.subsampling]
        T0, H, row = self.y.shape
        if width is None:
            if self.fmt == "v210":
                raise ValueError("width is required for fmt 'v210': a row holds whole blocks of six pixels")
            width = row // per_group * P
        W = int(width)
        if W < 1 or ops.yuv_packed_words(self.fmt, W) > row:
            raise ValueError("width %r needs rows of %d words of %d byte(s) for fmt %r, data has %d"
                             % (width, ops.yuv_packed_words(self.fmt, max(W, 1)), ws, fmt, row))
        if T0 > 65535 or H > 65535 or W > 65535:
            raise ValueError("data %s: at most 65535 frames, rows and pixels per row" % (tuple(self.y.shape),))
        self.shape = (T0, H, W, 3)

    def _over(self, cut):
        return PackedYuvFrames(cut(self.y), self.name, self.shape[2], **self.colour())

    def planes(self):
        """the read set as ONE view: data [T0, H, the words of ceil(W / P) groups] - the pitch padding cut off"""
        return (self.y[:, :, :ops.yuv_packed_words(self.fmt, self.shape[2])],)

    def kernel_views(self, planes):
        return tuple(planes)

    def to_rgb(self, planes, out):
        """ONE tdc_yuv_packed_to_rgb launch: the frames of `planes` (the device surface laid out like planes()) -> out uint8
        [T, H, W, 3]; transfer "pq" / "hlg" passes the descriptor, its table taken from (and made once for) the surface's device"""
        H, W = self.shape[1:3]
        hdr = self.hdr_on(planes[0].device)
        if self.interpolates:       # ONE tdc_yuv_packed_linear_to_rgb launch in its place
            return ops.yuv_packed_linear_to_rgb(planes[0], self.fmt, self.coef, H, W, self.bits, self.msb_aligned,
                                                CHROMA_SITES[self.siting], hdr=hdr, out=out)
        return ops.yuv_packed_to_rgb(planes[0], self.fmt, self.coef, H, W, self.bits, self.msb_aligned, hdr=hdr, out=out)


def is_yuv_frames(x):
    """a YuvFrames, recognised by its members (the package can be imported under two names: not by isinstance)"""
    return all(hasattr(x, k) for k in ("y", "chroma", "c_step", "coef", "shape")) and not torch.is_tensor(x)


def gather_planes(yuv, idx, pin=True):
    """the frames idx (check_indices; not None) of host planes, gathered plane by plane with the pitch padding removed into
    ONE staging tensor (pinned when `pin`) -> (the staged planes as views of it laid out like yuv.planes(), the staging
    tensor).  Frames outside idx and bytes outside planes() are never read.  The staging holds T * (H*W + 2*Hc*Wc) samples
    of the planes' type: that many bytes at 8 bits, twice as many at 10 and 12."""
    sel = torch.tensor(idx)
    src = yuv.planes()
    sizes = [len(idx) * p.shape[1] * p.shape[2] for p in src]
    stage = torch.empty(sum(sizes), dtype=src[0].dtype, pin_memory=pin)
    out, at = [], 0
    for p, n in zip(src, sizes):
        dst = stage[at:at + n].view(len(idx), p.shape[1], p.shape[2])
        torch.index_select(p, 0, sel, out=dst)
        out.append(dst)
        at += n
    return out, stage


def selected_planes(yuv, idx, device):
    """the frames idx (check_indices) of a YuvFrames as planes on `device`, laid out like yuv.planes() -> (planes, bytes
    uploaded).  Host planes: the kept frames go through gather_planes and one upload of exactly their bytes (dense pinned
    planes with every frame kept are uploaded from where they lie).  Device planes: used in place through their strides when
    every frame is kept, gathered on the device otherwise."""
    src = yuv.planes()
    if yuv.is_cuda:
        if idx is not None:
            sel = torch.tensor(idx, device=yuv.y.device)
            src = [torch.index_select(p, 0, sel) for p in src]
        return [p.to(device) for p in src], 0
    if idx is None and all(p.is_pinned() and p.is_contiguous() for p in src):
        return [p.to(device, non_blocking=True) for p in src], sum(p.numel() * p.element_size() for p in src)
    staged, stage = gather_planes(yuv, list(range(yuv.shape[0])) if idx is None else idx)
    dev = stage.to(device, non_blocking=True)
    out, at = [], 0
    for p in staged:
        out.append(dev[at:at + p.numel()].view(p.shape))
        at += p.numel()
    return out, stage.numel() * stage.element_size()


# ---- channel-first, BGR, RGBA and gray frames -------------------------------------------------------
RGB_LAYOUTS = ("hwc", "chw")


def channel_order(order, C):
    """the stored channels (iR, iG, iB) an `order` string names among C stored channels: one letter per stored channel,
    case-insensitive - each of r, g, b exactly once, or l (gray) exactly once and then iR = iG = iB, every other letter an
    ignored a or x; anything else, or a length other than C, raises ValueError"""
    if not isinstance(order, str):
        raise ValueError("order must be a string with one letter per stored channel, got %r" % (order,))
    o = order.lower()
    if len(o) != C or not 1 <= C <= 4:
        raise ValueError("order %r names %d channel(s), the data stores %d (1 to 4 are taken)" % (order, len(o), C))
    if any(ch not in "rgblax" for ch in o):
        raise ValueError("order %r: the letters are r, g, b, l (gray) and the ignored a, x" % (order,))
    if "l" in o:
        if o.count("l") != 1 or any(ch in o for ch in "rgb"):
            raise ValueError("order %r: a gray order holds l exactly once beside ignored a / x" % (order,))
        return (o.index("l"),) * 3
    if any(o.count(ch) != 1 for ch in "rgb"):
        raise ValueError("order %r: a colour order holds each of r, g, b exactly once beside ignored a / x" % (order,))
    return tuple(o.index(ch) for ch in "rgb")


class RgbFrames:
    """T0 decoded pictures of one size in the layout their source writes, described and not copied: `data` is a uint8 torch
    tensor or numpy array, on the host or the device, taken through its strides as it is - a row pitch, a crop or a slice of
    frames is a valid source (a negative numpy stride raises ValueError).  layout "hwc": [T0, H, W, C], what OpenCV, Pillow
    and hardware RGB surfaces write; "chw": [T0, C, H, W], what torchcodec and torchvision.io return; a 3-D [T0, H, W] is one
    gray channel (order "l") under either.  `order` names the C stored channels, 1 to 4 of them, one letter each,
    case-insensitive: r, g, b once each plus ignored a / x ("rgb", "bgr", "rgba", "bgra", "argb", "abgr", "rgbx", ...), or
    l once plus ignored a / x ("l", "la", "al").  The RGB frames it stands for are what Pillow's .convert("RGB") gives:
    alpha is dropped and not composited, gray is replicated into R, G and B.  .shape is (T0, H, W, 3), theirs; r[a:b] is an
    RgbFrames over the same memory.  The kept frames are packed on the device, in front of the resize (tdc_pack_rgb);
    layout "hwc" with order "rgb" is the frames entry's own form and issues no launch."""

    def __init__(self, data, layout="hwc", order="rgb"):
        if layout not in RGB_LAYOUTS:
            raise ValueError("layout must be one of %s, got %r" % (RGB_LAYOUTS, layout))
        if is_rgb_frames(data) or is_oriented(data) or is_yuv_frames(data):
            raise ValueError("data must be a uint8 torch tensor or numpy array, got a %s: an RgbFrames describes memory (an "
                             "Oriented goes around it, not inside)" % type(data).__name__)
        if isinstance(data, np.ndarray):
            if data.dtype != np.uint8:
                raise ValueError("data must be uint8, got %s" % (data.dtype,))
            if any(s < 0 for s in data.strides):
                raise ValueError("data has a negative stride: a flipped view is not described here (preprocess.Oriented mirrors)")
            data = torch.from_numpy(data)
        if not torch.is_tensor(data):
            raise ValueError("data must be a uint8 torch tensor or numpy array, got %s" % type(data).__name__)
        if data.dtype != torch.uint8 or data.dim() not in (3, 4) or 0 in data.shape:
            raise ValueError("data must be uint8 [T0, H, W, C], [T0, C, H, W] or [T0, H, W] with no empty dimension, got %s %s"
                             % (data.dtype, tuple(data.shape)))
        if data.dim() == 3:
            data = data.unsqueeze(3 if layout == "hwc" else 1)
        T0, H, W, C = (data.shape[i] for i in ((0, 1, 2, 3) if layout == "hwc" else (0, 2, 3, 1)))
        self.index = channel_order(order, int(C))
        if T0 > 65535 or H > 65535 or W > 65535:
            raise ValueError("data %s: at most 65535 frames, rows and pixels per row" % (tuple(data.shape),))
        self.data, self.layout, self.order = data, layout, order.lower()
        self.shape = (int(T0), int(H), int(W), 3)

    @classmethod
    def chw(cls, data, order="rgb"):
        """channel-first frames [T0, C, H, W]: a torchcodec / torchvision.io decoder's default"""
        return cls(data, "chw", order)

    @classmethod
    def gray(cls, data):
        """one gray plane per frame [T0, H, W], replicated into R, G and B"""
        if not hasattr(data, "ndim") or data.ndim != 3:
            raise ValueError("RgbFrames.gray takes [T0, H, W], got %s" % (tuple(getattr(data, "shape", ())),))
        return cls(data, "hwc", "l")

    @property
    def is_identity(self):
        """[T0, H, W, 3] in R, G, B order: what the frames entries take as it is"""
        return self.layout == "hwc" and self.index == (0, 1, 2) and self.data.shape[3] == 3

    @property
    def is_cuda(self):
        return self.data.is_cuda

    @property
    def device(self):
        return self.data.device

    @property
    def is_gray(self):
        return self.index[0] == self.index[1] == self.index[2]

    def __getitem__(self, s):
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError("RgbFrames takes a slice of frames a:b, got %r" % (s,))
        return RgbFrames(self.data[s], self.layout, self.order)

    def field(self, parity, layout="interleaved"):
        """one field of interlaced frames: an RgbFrames over the same memory holding the pictures'
        rows of field `parity` (field_rows), layout and order kept"""
        rows = field_rows(self.shape[1], parity, layout)
        return RgbFrames(self.data[:, rows] if self.layout == "hwc" else self.data[:, :, rows], self.layout, self.order)

    def descriptor(self):
        """(byte offset of the base inside data's storage, frame_stride, row_stride, pixel_stride, chan) as Python ints, from
        the strides alone: the R, G, B sample of pixel (t, y, x) is the byte base + t * frame_stride + y * row_stride +
        x * pixel_stride + chan[c] of the storage.  What tdc_pack_rgb takes, with data's first element as the base."""
        st = self.data.stride()
        fs, rs, ps, cs = (st[i] for i in ((0, 1, 2, 3) if self.layout == "hwc" else (0, 2, 3, 1)))
        return int(self.data.storage_offset()), int(fs), int(rs), int(ps), tuple(int(i * cs) for i in self.index)

    def pack(self, out):
        """ONE tdc_pack_rgb launch: these frames (on the device) -> out uint8 [T, H, W, 3]"""
        _, fs, rs, ps, chan = self.descriptor()
        T, H, W, _ = self.shape
        return ops.pack_rgb(self.data, fs, rs, ps, chan, T, H, W, out=out)

    def dense_like(self, T, make):
        """(staging tensor, RgbFrames over it) for T frames in this source's own layout, made dense: "hwc" [T, H, W, C], every
        stored channel; "chw" only the planes that are used, in R, G, B order (gray: the one), each plane's T frames
        together.  make(shape) allocates the uint8 staging tensor."""
        _, H, W, _ = self.shape
        if self.layout == "hwc":
            stage = make((T, H, W, self.data.shape[3]))
            return stage, RgbFrames(stage, "hwc", self.order)
        stage = make((1 if self.is_gray else 3, T, H, W))
        return stage, RgbFrames(stage.permute(1, 0, 2, 3), "chw", "l" if self.is_gray else "rgb")

    def gather_into(self, staged, sel):
        """the frames `sel` (an index tensor on data's device) -> the frames of `staged` (dense_like), by index_select on views:
        only the kept frames' used bytes are read - no pitch padding, and of "chw" no plane that is ignored"""
        if self.layout == "hwc":
            torch.index_select(self.data, 0, sel, out=staged.data)
        else:
            for k, i in enumerate(self.index[:1] if self.is_gray else self.index):
                torch.index_select(self.data[:, i], 0, sel, out=staged.data[:, k])
        return staged

    @property
    def is_dense(self):
        """contiguous, and every stored byte a used one or an interleaved neighbour of one: uploaded as it lies"""
        return self.data.is_contiguous() and (self.layout == "hwc" or self.data.shape[1] == (1 if self.is_gray else 3))


def is_rgb_frames(x):
    """an RgbFrames, recognised by its members (the package can be imported under two names: not by isinstance)"""
    return all(hasattr(x, k) for k in ("data", "layout", "order", "index", "descriptor", "shape")) and not torch.is_tensor(x)


def gather_pixels(rgb, idx, pin=True):
    """the frames idx (check_indices; not None) of a host RgbFrames, gathered into ONE dense staging tensor (pinned when
    `pin`) in the source's own layout -> (an RgbFrames over the staging tensor, the staging tensor).  Frames outside idx,
    pitch padding and ignored planes of a "chw" source are never read.  The staging holds T * H * W * C bytes for "hwc",
    T * H * W * 3 for "chw" colour and T * H * W for gray."""
    stage, staged = rgb.dense_like(len(idx), lambda shape: torch.empty(shape, dtype=torch.uint8, pin_memory=pin))
    return rgb.gather_into(staged, torch.tensor(idx)), stage


def selected_pixels(rgb, idx, device):
    """the frames idx (check_indices) of an RgbFrames as an RgbFrames on `device` -> (it, bytes uploaded).  Host data: the kept
    frames go through gather_pixels and one upload of exactly their bytes (dense pinned data with every frame kept is
    uploaded from where it lies).  Device data: read in place through its strides when every frame is kept, gathered on the
    device in its own layout otherwise."""
    if rgb.is_cuda:
        if idx is None:
            return RgbFrames(rgb.data.to(device), rgb.layout, rgb.order), 0
        _, staged = rgb.dense_like(len(idx), lambda shape: torch.empty(shape, dtype=torch.uint8, device=rgb.device))
        rgb.gather_into(staged, torch.tensor(idx, device=rgb.device))
        return RgbFrames(staged.data.to(device), staged.layout, staged.order), 0
    if idx is None and rgb.data.is_pinned() and rgb.is_dense:
        return RgbFrames(rgb.data.to(device, non_blocking=True), rgb.layout, rgb.order), rgb.data.numel()
    staged, stage = gather_pixels(rgb, list(range(rgb.shape[0])) if idx is None else idx)
    dev = stage.to(device, non_blocking=True)
    return RgbFrames(dev if rgb.layout == "hwc" else dev.permute(1, 0, 2, 3), staged.layout, staged.order), stage.numel()


# ---- display orientation ---------------------------------------------------------------------------
ROTATIONS = (0, 90, 180, 270)
# EXIF orientation -> (rotate, hflip): the clockwise turn that makes the stored picture upright, then a left-right mirror
EXIF_ORIENTATIONS = {1: (0, False), 2: (0, True), 3: (180, False), 4: (180, True),
                     5: (90, True), 6: (90, False), 7: (270, True), 8: (270, False)}


class Oriented:
    """T0 stored frames and the display orientation that travels beside them, described and not copied: `frames` is what the
    frames entries take - uint8 [T0, H, W, 3] (torch tensor or numpy array, host or device), a YuvFrames of any kind or an
    RgbFrames - as the decoder wrote it, `rotate` in {0, 90, 180, 270} the clockwise turn that makes a stored frame upright (the `rotate`
    tag of MP4 / MOV), `hflip` a left-right mirror applied after the turn.  With S a stored frame [H, W, 3], the upright
    frame O is
        rotate   0: O[y, x] = S[y, x]                 rotate 180: O[y, x] = S[H-1-y, W-1-x]          both [H, W, 3]
        rotate  90: O[y, x] = S[H-1-x, y]             rotate 270: O[y, x] = S[x, W-1-y]              both [W, H, 3]
        hflip:      O'[y, x] = O[y, W'-1-x]
    (np.rot90(S, -1) is rotate 90; a vertical flip is rotate 180 with hflip).  .shape is (T0, H', W', 3), that of the upright
    frames; o[a:b] is an Oriented over the same memory.  The kept frames are turned on the device, in front of the resize
    (tdc_orient_frames); everything behind sees the upright frames.  `frames` may also be an Interlaced over any of these
    kinds: the field is rebuilt to the stored frame first, then the frame is turned."""

    def __init__(self, frames, rotate=0, hflip=False):
        if isinstance(rotate, bool) or rotate not in ROTATIONS:
            raise ValueError("rotate must be one of %s (clockwise degrees), got %r" % (ROTATIONS, rotate))
        if not isinstance(hflip, bool):
            raise ValueError("hflip must be True / False, got %r" % (hflip,))
        if is_oriented(frames):
            raise ValueError("frames is an Oriented already: compose the two orientations into one")
        self.frames = frames if is_yuv_frames(frames) or is_rgb_frames(frames) or is_interlaced(frames) else check_frames(frames)
        self.rotate, self.hflip, self.quarters = int(rotate), hflip, int(rotate) // 90
        T0, H, W, _ = self.frames.shape
        self.shape = (int(T0), int(W), int(H), 3) if self.quarters & 1 else (int(T0), int(H), int(W), 3)

    @classmethod
    def exif(cls, frames, orientation):
        """from an EXIF orientation 1 .. 8 (EXIF_ORIENTATIONS)"""
        if isinstance(orientation, bool) or orientation not in EXIF_ORIENTATIONS:
            raise ValueError("an EXIF orientation is 1 .. 8, got %r" % (orientation,))
        return cls(frames, *EXIF_ORIENTATIONS[orientation])

    @property
    def is_identity(self):
        return self.quarters == 0 and not self.hflip

    @property
    def is_cuda(self):
        return self.frames.is_cuda

    def __getitem__(self, s):
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError("Oriented takes a slice of frames a:b, got %r" % (s,))
        return Oriented(self.frames[s], self.rotate, self.hflip)


def is_oriented(x):
    """an Oriented, recognised by its members (the package can be imported under two names: not by isinstance)"""
    return all(hasattr(x, k) for k in ("frames", "rotate", "hflip", "quarters", "shape")) and not torch.is_tensor(x)


# ---- interlaced video: one field rebuilt to full height ---------------------------------------------
FIELDS = ("top", "bottom")
FIELD_LAYOUTS = ("interleaved", "sequential_tb", "sequential_bt")


def field_rows(n, parity, layout="interleaved"):
    """the rows of field `parity` (0 top, 1 bottom) among the n rows (n even) of one plane, as a slice: every second row from
    row `parity` on ("interleaved"), or one half of the rows - the top field first ("sequential_tb", V4L2 FIELD_SEQ_TB) or the
    bottom field first ("sequential_bt")"""
    if layout == "interleaved":
        return slice(parity, None, 2)
    first = parity == (0 if layout == "sequential_tb" else 1)
    return slice(0, n // 2) if first else slice(n // 2, n)


class Interlaced:
    """T0 interlaced frames and the field to keep of them, described and not copied: `frames` is what the frames entries take
    except an Oriented or an Interlaced - uint8 [T0, H, W, 3] (torch tensor or numpy array, host or device), an RgbFrames, or a
    YuvFrames, planar or packed, SDR or HDR - holding two fields per frame: layout "interleaved", field f (0 top, 1 bottom)
    is rows f, f + 2, ... of every plane; "sequential_tb", the top field is rows [0, H / 2) of every plane and the bottom
    field the rest (V4L2 FIELD_SEQ_TB); "sequential_bt", the reverse.  The chroma planes of a vertically sub-sampled surface
    split the same way, plane by plane, so a field of a 4:2:0 surface is a half-height 4:2:0 picture with its own chroma rows.
    `field` "top" / "bottom" is the field that is kept: it alone is uploaded, converted or packed, and its Hf = H / 2 rows
    F[k] become the rows 2k + p of the frame (p = 0 top, 1 bottom).  `fill` makes the other rows, per byte of the RGB picture,
    with m = k - p and cl(i) = min(max(i, 0), Hf - 1):
        "linear":  O[2k + 1 - p] = (F[cl(m)] + F[cl(m+1)] + 1) >> 1
        "cubic":   O[2k + 1 - p] = clip_0_255((9 * (F[cl(m)] + F[cl(m+1)]) - F[cl(m-1)] - F[cl(m+2)] + 8) >> 4)
    (tdc_field_to_frame: a stated formula, no library's deinterlacer).  .shape is (T0, H, W, 3), that of the rebuilt frames;
    x[a:b] is an Interlaced over the same memory.  An Oriented goes around an Interlaced, not inside: fields belong to the
    coded picture, so the field is rebuilt first and the frame turned after.  ValueError: a bad field / fill / layout; H odd;
    H % 4 != 0 on a surface with vertically sub-sampled chroma (its two chroma fields would differ in height); upsample
    "linear" on such a surface (a field's chroma sits a quarter of a field row off the sitings of section 26)."""

    def __init__(self, frames, field="top", fill="linear", layout="interleaved"):
        if field not in FIELDS:
            raise ValueError("field must be one of %s, got %r" % (FIELDS, field))
        if fill not in ops.FIELD_FILLS:
            raise ValueError("fill must be one of %s, got %r" % (sorted(ops.FIELD_FILLS), fill))
        if layout not in FIELD_LAYOUTS:
            raise ValueError("layout must be one of %s, got %r" % (FIELD_LAYOUTS, layout))
        if is_oriented(frames):
            raise ValueError("frames is an Oriented: fields belong to the coded picture, so the Oriented goes around the "
                             "Interlaced - Oriented(Interlaced(frames, ...), rotate, hflip)")
        if is_interlaced(frames):
            raise ValueError("frames is an Interlaced already")
        self.frames = frames if is_yuv_frames(frames) or is_rgb_frames(frames) else check_frames(frames)
        self.field, self.fill, self.layout, self.parity = field, fill, layout, FIELDS.index(field)
        T0, H, W, _ = self.frames.shape
        if H % 2:
            raise ValueError("interlaced frames hold two fields of equal height: H must be even, got %d" % H)
        if is_yuv_frames(self.frames) and self.frames.sub_y:
            if H % 4:
                raise ValueError("a %s surface splits into fields whose chroma planes have H / 4 rows: H must be a multiple of 4, "
                                 "got %d" % (self.frames.subsampling, H))
            if self.frames.upsample == "linear":
                raise ValueError("upsample 'linear' on a %s surface is not taken inside an Interlaced: a field's chroma rows sit a "
                                 "quarter of a field row off the sitings that are interpolated; use 'replicate'" % self.frames.subsampling)
        self.shape = (int(T0), int(H), int(W), 3)

    @property
    def is_cuda(self):
        return self.frames.is_cuda

    def __getitem__(self, s):
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError("Interlaced takes a slice of frames a:b, got %r" % (s,))
        return Interlaced(self.frames[s], self.field, self.fill, self.layout)

    def field_frames(self):
        """the kept field as a view of the wrapped kind: a uint8 [T0, H / 2, W, 3] tensor, an RgbFrames or a YuvFrames over the
        same memory"""
        if torch.is_tensor(self.frames):
            return self.frames[:, field_rows(self.shape[1], self.parity, self.layout)]
        return self.frames.field(self.parity, self.layout)


def is_interlaced(x):
    """an Interlaced, recognised by its members (the package can be imported under two names: not by isinstance)"""
    return all(hasattr(x, k) for k in ("frames", "field", "fill", "layout", "parity", "shape")) and not torch.is_tensor(x)


def selected_field(field, idx, device):
    """the frames idx (check_indices) of a field view (uint8 [T0, Hf, W, 3], strided: Interlaced.field_frames) on `device` ->
    (a [T, Hf, W, 3] tensor whose pixels are dense, bytes uploaded).  On the host the kept frames' field rows are gathered into
    one pinned staging tensor and uploaded - a dropped frame and the other field are never read or copied; on the device the
    view is read where it lies when every frame is kept and its pixels are dense (three adjacent bytes, W of them adjacent in a
    row: what tdc_field_to_frame addresses), and the kept frames' field rows are gathered dense there otherwise - under a
    selection, or for a view such as a permuted channel-first tensor or rgba[..., :3], which check_frames takes."""
    if field.is_cuda:
        if idx is not None:
            field = torch.index_select(field, 0, torch.tensor(idx, device=field.device))
        elif not ops.field_pixels_dense(field):
            field = field.contiguous()
        return field.to(device), 0
    stage = torch.empty((field.shape[0] if idx is None else len(idx),) + tuple(field.shape[1:]), dtype=torch.uint8, pin_memory=True)
    if idx is None:
        stage.copy_(field)
    else:
        torch.index_select(field, 0, torch.tensor(idx), out=stage)
    return stage.to(device, non_blocking=True), stage.numel()


def _check_dtype_slab(dtype, slab):
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("preprocess_selected writes float16 or bfloat16 pixels, got %s" % (dtype,))
    if isinstance(slab, bool) or not isinstance(slab, int) or not 1 <= slab <= 65535:
        raise ValueError("slab must be a frame count in [1, 65535], got %r" % (slab,))


def _outputs(out, towers, T, dtype, device):
    """one [T, 3, R, R] tensor per tower: new ones, or the caller's `out` checked against the towers"""
    if out is None:
        return [torch.empty(T, 3, t["R"], t["R"], device=device, dtype=dtype) for t in towers]
    out = list(out)
    if len(out) != len(towers):
        raise ValueError("out holds %d tensors for %d towers" % (len(out), len(towers)))
    for o, t in zip(out, towers):
        if not (torch.is_tensor(o) and o.device == device and o.dtype == dtype and o.is_contiguous() and o.dim() == 4
                and o.shape[0] >= T and tuple(o.shape[1:]) == (3, t["R"], t["R"])):
            raise ValueError("out must be contiguous %s [>= %d, 3, %d, %d] tensors on %s" % (dtype, T, t["R"], t["R"], device))
    return out


def preprocess_selected(frames, idx, towers=(SIGLIP, DINOV2), dtype=torch.float16, slab=64, device=None, out=None, stats=None):
    """process_images(frames[idx], dtype, towers) for a caller that holds a whole decoded video: frames uint8 [T0, H, W, 3]
    (a torch tensor - pageable, pinned or on the device - or a numpy array), idx the ascending host list of the frames to
    keep (encode.frame_indices; None: all) -> one [T, 3, R, R] tensor per tower on `device` (default: the frames' device, or
    the current one), bit for bit what process_images gives for the kept frames.
    frames may also be a YuvFrames (a decoder's planes, DESIGN.md sections 19 and 20): its kept frames are converted to RGB on the device,
    slab by slab, in front of the same resize - the result is what the RGB frames the planes convert to give.
    The kept frames are resized in slabs of at most `slab` frames: one tdc_preprocess_frames call per slab and tower writes its
    slice of the output, and ONE scratch of tdc_preprocess_scratch_bytes(slab, H, W, R) bytes serves every slab and tower, so the
    scratch does not grow with the video.  Frames are resized independently: the result does not depend on `slab`.
    out: one preallocated contiguous [>= T, 3, R, R] tensor of `dtype` per tower - rows [0, T) are written, nothing else, and
    the views out[j][:T] are returned.  stats: a dict that receives frames_in, frames_resized and bytes_uploaded.
    frames may be an Oriented over either kind: the kept frames are turned upright on the device, one
    launch per slab, in front of the same resize - the result is what the upright frames give.
    frames may be an RgbFrames (an Oriented may hold one): channel-first, B G R, 4-byte-pixel or gray
    pictures, pitched or cropped, packed to R G B on the device, one launch per slab, in front of the same resize - the result
    is what the [T0, H, W, 3] frames Pillow's .convert("RGB") makes of them give.
    frames may be an Interlaced over any of these kinds (an Oriented may hold one): only the kept field
    is uploaded, converted or packed, and the full-height frames are rebuilt from it on the device, one tdc_field_to_frame
    launch per slab, in front of the same resize - the result is what the frames a host rebuilds by the stated formula give.
    The launches, for every kind (_plan): the kept frames - of an Interlaced only their kept field, half the bytes - are uploaded
    as their innermost kind is, and per slab of kept frames the stages that apply run in the order
        convert or pack -> rebuild -> turn -> resize
    each ONE launch into a slab-sized uint8 [slab, H, W, 3] scratch of its own that serves the whole video: YuvFrames.to_rgb
    (tdc_yuv420_to_rgb for 8-bit 4:2:0, tdc_yuv_to_rgb for every other planar kind, tdc_yuv_hdr_to_rgb under pq / hlg,
    tdc_yuv_packed_to_rgb for a packed surface; with upsample "linear" tdc_yuv_linear_to_rgb / tdc_yuv_packed_linear_to_rgb in
    their place) or RgbFrames.pack (tdc_pack_rgb) at the stored size, of a field at H / 2; tdc_field_to_frame to [H, W];
    tdc_orient_frames to the upright [H', W']; then tdc_preprocess_frames per tower on the last scratch - the RGB path's
    launches on the frames the source stands for.  A slab is made once and every tower reads it.  Plain uint8 frames, an RgbFrames
    that is [T0, H, W, 3] in R, G, B order and an identity Oriented over either have no stage and issue exactly the launches of
    the tensor; the kept field of such frames is read where it lies by tdc_field_to_frame."""
    source, upload, stages = _plan(frames)
    T0 = source.shape[0]                            # a wrapper keeps every frame of what it wraps
    idx = check_indices(idx, T0)                    # on the host, before anything is uploaded or launched
    _check_dtype_slab(dtype, slab)
    if device is None:
        device = source.device if source.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    kept, uploaded = upload(source, idx, device)
    planar = isinstance(kept, list)                 # selected_planes: the planes of the kept frames, each [T, rows, samples]
    T = (kept[0] if planar else kept).shape[0]
    if stats is not None:
        stats.update(frames_in=T0, frames_resized=T, bytes_uploaded=uploaded)
    out = _outputs(out, towers, T, dtype, device)
    lib = L.load()
    n0 = min(slab, T)
    Ho, Wo = stages[-1][0] if stages else source.shape[1:3]
    nscr = max(lib.tdc_preprocess_scratch_bytes(n0, Ho, Wo, t["R"]) for t in towers)
    scratch = torch.empty(max(nscr, 1), dtype=torch.uint8, device=device)
    made = [torch.empty((n0, H, W, 3), dtype=torch.uint8, device=device) for (H, W), _ in stages]
    tables = [_tables(max(Ho, Wo), t["R"], t["mean"], t["std"], device) for t in towers]
    slabs = [(s, min(slab, T - s)) for s in range(0, T, slab)]
    with torch.cuda.device(device):
        if not stages:
            # nothing to make per slab, so the frames are resized where the upload left them, tower by tower: all slabs of the
            # first tower, then all of the next.  With stages a slab is made once and every tower reads it before the next slab
            # overwrites the scratches, so the loop is slab by slab (tests/test_hip_orient_inputs.py holds both orders).
            for t, o, tab in zip(towers, out, tables):
                for s, n in slabs:
                    _resize(kept[s:s + n], n, Ho, Wo, t, tab, o[s:s + n], dtype, scratch)
        else:
            for s, n in slabs:
                x = [p[s:s + n] for p in kept] if planar else kept[s:s + n]
                for (_, run), buf in zip(stages, made):
                    run(x, buf[:n])
                    x = buf[:n]
                for t, o, tab in zip(towers, out, tables):
                    _resize(x, n, Ho, Wo, t, tab, o[s:s + n], dtype, scratch)
    return [o[:T] for o in out]


def _plan(frames):
    """what preprocess_selected does for `frames`, found once -> (source, upload, stages).  The wrappers are peeled in their one
    nesting order, Oriented(Interlaced(kind)): an Oriented that turns or mirrors gives the turn stage (the identity gives
    none), an Interlaced replaces the kind by the view of its kept field and gives the rebuild stage, and an RgbFrames that is
    [T0, H, W, 3] in R, G, B order already stands for its tensor.  `source` is the innermost kind and upload(source, idx,
    device) its kept frames on the device: selected_frames for a tensor (selected_field for the kept field of one),
    selected_planes for a YuvFrames, planar or packed, whose front stage is its to_rgb, selected_pixels for any other
    RgbFrames, whose front stage is its pack.  A stage is ((H, W), run): run(x, made) issues ONE launch from x, the slab the
    stage before it made or the slab of the upload, into made, a uint8 [n, H, W, 3] scratch."""
    turn = rebuild = None
    if is_oriented(frames):
        turn, frames = (None if frames.is_identity else frames), frames.frames
    if is_interlaced(frames):
        rebuild, frames = frames, frames.field_frames()
    if is_rgb_frames(frames) and frames.is_identity:
        frames = frames.data
    stages = []
    if is_yuv_frames(frames):
        upload = selected_planes
        stages.append((frames.shape[1:3], frames.to_rgb))
    elif is_rgb_frames(frames):
        upload = selected_pixels
        stages.append((frames.shape[1:3], lambda kept, made: kept.pack(made)))
    else:
        frames = check_frames(frames)
        upload = selected_frames if rebuild is None else selected_field
    if rebuild is not None:
        stages.append((rebuild.shape[1:3], lambda x, made: ops.field_to_frame(x, rebuild.parity, rebuild.fill, out=made)))
    if turn is not None:
        stages.append((turn.shape[1:3], lambda x, made: ops.orient_frames(x, turn.quarters, turn.hflip, out=made)))
    return frames, upload, stages
