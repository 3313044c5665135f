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
    pad = [int(x * 255) for x in mean]        # expand2square background (tdc/mm_datautils.py:302-304)
    L.check(lib.tdc_preprocess_frames(ops._ptr(frames), T, H, W, R, ops._ptr(bounds), ops._ptr(coeffs), coeffs.shape[1],
                                      pad[0], pad[1], pad[2], ops._ptr(lut), ops._ptr(out), int(out_f32),
                                      ops._dtcode(dtype), ops._ptr(scratch), ops._stream()), "tdc_preprocess_frames")
    return out


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


def preprocess_selected(frames, idx, towers=(SIGLIP, DINOV2), dtype=torch.float16, slab=64, device=None, out=None, stats=None):
    """process_images(frames[idx], dtype, towers) for a caller that holds a whole decoded video: frames uint8 [T0, H, W, 3]
    (a torch tensor - pageable, pinned or on the device - or a numpy array), idx the ascending host list of the frames to
    keep (encode.frame_indices; None: all) -> one [T, 3, R, R] tensor per tower on `device` (default: the frames' device, or
    the current one), bit for bit what process_images gives for the kept frames.
    The kept frames are resized in slabs of at most `slab` frames: one tdc_preprocess_frames call per slab and tower writes its
    slice of the output, and ONE scratch of tdc_preprocess_scratch_bytes(slab, H, W, R) bytes serves every slab and tower, so the
    scratch does not grow with the video.  Frames are resized independently: the result does not depend on `slab`.
    out: one preallocated contiguous [>= T, 3, R, R] tensor of `dtype` per tower - rows [0, T) are written, nothing else, and
    the views out[j][:T] are returned.  stats: a dict that receives frames_in, frames_resized and bytes_uploaded."""
    frames = check_frames(frames)
    idx = check_indices(idx, frames.shape[0])       # on the host, before anything is launched
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("preprocess_selected writes float16 or bfloat16 pixels, got %s" % (dtype,))
    if isinstance(slab, bool) or not isinstance(slab, int) or not 1 <= slab <= 65535:
        raise ValueError("slab must be a frame count in [1, 65535], got %r" % (slab,))
    if device is None:
        device = frames.device if frames.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    T0, H, W, _ = frames.shape
    kept, uploaded = selected_frames(frames, idx, device)
    T = kept.shape[0]
    if stats is not None:
        stats.update(frames_in=T0, frames_resized=T, bytes_uploaded=uploaded)
    if out is None:
        out = [torch.empty(T, 3, t["R"], t["R"], device=device, dtype=dtype) for t in towers]
    else:
        out = list(out)
        if len(out) != len(towers):
            raise ValueError("out holds %d tensors for %d towers" % (len(out), len(towers)))
        for o, t in zip(out, towers):
            if not (torch.is_tensor(o) and o.device == device and o.dtype == dtype and o.is_contiguous() and o.dim() == 4
                    and o.shape[0] >= T and tuple(o.shape[1:]) == (3, t["R"], t["R"])):
                raise ValueError("out must be contiguous %s [>= %d, 3, %d, %d] tensors on %s" % (dtype, T, t["R"], t["R"], device))
    lib = L.load()
    n0 = min(slab, T)
    nscr = max(lib.tdc_preprocess_scratch_bytes(n0, H, W, t["R"]) for t in towers)
    scratch = torch.empty(max(nscr, 1), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        for t, o in zip(towers, out):
            R = t["R"]
            bounds, coeffs, lut = _tables(max(H, W), R, t["mean"], t["std"], device)
            pad = [int(x * 255) for x in t["mean"]]   # expand2square background (tdc/mm_datautils.py:302-304)
            for s in range(0, T, slab):
                n = min(slab, T - s)
                L.check(lib.tdc_preprocess_frames(ops._ptr(kept[s:s + n]), n, H, W, R, ops._ptr(bounds), ops._ptr(coeffs),
                                                  coeffs.shape[1], pad[0], pad[1], pad[2], ops._ptr(lut), ops._ptr(o[s:s + n]), 0,
                                                  ops._dtcode(dtype), ops._ptr(scratch), ops._stream()), "tdc_preprocess_frames")
    return [o[:T] for o in out]
