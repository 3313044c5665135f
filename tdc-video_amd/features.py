"""Stored tower features: run the frozen towers once per video, start every later encode behind them.

A FeatureSet is one video (or one image) after a3 / a4: the SigLIP and DINOv2 rows of EVERY input frame, exactly as
VideoEncoder.tower hands them on (padding columns dropped), with the source image size and a signature of the towers that
made them.  Everything downstream - a1, a5, the connector, the Q-Former, the emission - reads only these rows, so a set
survives a change of connector / Q-Former checkpoint, of `context_token_num`, of the frame cap and of the prompts, across
processes and days (save / load).  It does not survive anything that changes a tower output bit: that is what the signature
holds, and encode.check_features refuses a set whose signature is not the engine's.
"""
import torch

from .cache import fingerprint_rows_host

FORMAT = 1


class FeatureSet:
    """siglip [T0, P, Ds], dino [T0, P, Dd] (16-bit, the type the towers emit; P = 576 at full size), image_size (the source
    image size the connector un-pads by), signature (tower_signature of the exporting engine; None: unknown)."""

    def __init__(self, siglip, dino, image_size, signature=None):
        if not (torch.is_tensor(siglip) and torch.is_tensor(dino) and siglip.dim() == 3 and dino.dim() == 3):
            raise ValueError("a FeatureSet holds two [frames, tokens, width] tensors")
        if siglip.shape[:2] != dino.shape[:2] or siglip.shape[0] < 1:
            raise ValueError("SigLIP features %s and DINOv2 features %s do not describe the same frames"
                             % (tuple(siglip.shape), tuple(dino.shape)))
        # fp32: the CPU engine doubles of the tests; VideoEncoder.feature_rows takes the engine's own 16-bit type only
        if siglip.dtype != dino.dtype or siglip.dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise ValueError("feature types %s / %s: both towers emit one type, fp16 or bf16" % (siglip.dtype, dino.dtype))
        self.siglip, self.dino = siglip, dino
        self.image_size = tuple(int(v) for v in image_size)
        self.signature = None if signature is None else str(signature)

    @property
    def frames(self):
        return int(self.siglip.shape[0])

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.siglip, self.dino))

    def to(self, device):
        """the set with both tensors on `device` (itself when they already are)"""
        device = torch.device(device)
        if self.siglip.device == device and self.dino.device == device:
            return self
        return FeatureSet(self.siglip.to(device), self.dino.to(device), self.image_size, self.signature)

    def cpu(self):
        """the set in host memory - pinned when CUDA is available, so .to(device) is one DMA per tensor"""
        def host(t):
            if t.device.type == "cpu" and (t.is_pinned() or not torch.cuda.is_available()):
                return t
            out = torch.empty(t.shape, dtype=t.dtype, pin_memory=torch.cuda.is_available())
            return out.copy_(t)
        return FeatureSet(host(self.siglip), host(self.dino), self.image_size, self.signature)

    def save(self, path):
        """a plain dict of tensors, ints and strings through torch.save: no pickled class, loads with weights_only=True"""
        def compact(t):                         # a copy that owns exactly its bytes (a view would drag its whole storage along)
            return t.detach().to("cpu").clone(memory_format=torch.contiguous_format)
        torch.save(dict(format=FORMAT, siglip=compact(self.siglip), dino=compact(self.dino),
                        image_size=[int(v) for v in self.image_size], signature=self.signature or ""), path)

    @classmethod
    def load(cls, path, map_location="cpu"):
        d = torch.load(path, map_location=map_location, weights_only=True)
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise ValueError("%s is not a FeatureSet file of format %d" % (path, FORMAT))
        return cls(d["siglip"], d["dino"], d["image_size"], d["signature"] or None)


def is_feature_set(x):
    """a FeatureSet by what it holds (the package is importable under two names, so its class is not compared)"""
    return all(hasattr(x, k) for k in ("siglip", "dino", "image_size", "signature", "frames")) and not torch.is_tensor(x)


def _walk(e, v, out):
    """the content of a prepared tower, depth first in a fixed order: tensors as fingerprints of their bytes"""
    if torch.is_tensor(v):
        out.append(("tensor", str(v.dtype), tuple(v.shape), _tensor_fp(e, v)))
    elif isinstance(v, dict):
        for k in sorted(v):
            if not str(k).startswith("_"):      # "_..." entries are caches derived from the rest (position tables, structs)
                out.append(("key", str(k)))
                _walk(e, v[k], out)
    elif isinstance(v, (list, tuple)):
        out.append(("list", len(v)))
        for x in v:
            _walk(e, x, out)
    elif hasattr(v, "__slots__"):               # weights.Lin
        for k in v.__slots__:
            out.append(("key", k))
            _walk(e, getattr(v, k), out)
    else:
        out.append(("value", repr(v)))


def _tensor_fp(e, v):
    if v.numel() == 0:
        return (0, 0)
    if v.is_cuda and hasattr(e, "fingerprint"):                     # tdc_fingerprint_rows, where the weights lie
        d = v.detach().contiguous().view(-1)
        return tuple(int(x) for x in e.fingerprint(d, [0], d.numel() * d.element_size(), 0)[0])
    b = v.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy()
    return tuple(int(x) for x in fingerprint_rows_host(b)[0])


def weights_fingerprint(e, tower):
    """128-bit fingerprint (hex) of everything a prepared tower holds: every tensor's bytes, shapes, types and scalars"""
    import numpy as np
    out = []
    _walk(e, tower, out)
    a, b = fingerprint_rows_host(np.frombuffer(repr(out).encode(), dtype=np.uint8))[0]
    return "%016x%016x" % (int(a), int(b))


def tower_signature(e):
    """Everything that changes a tower output bit, as one string: per tower a fingerprint of its prepared weights, its operand
    type, fp8 level and LayerNorm fold; the residual-stream type, the type the rows are emitted in and the output grid.
    Nothing of the connector, the Q-Former or the config keys read behind the towers.  Cached by engine.feature_signature."""
    if hasattr(e, "feature_signature"):
        return e.feature_signature()
    return compute_tower_signature(e)


def compute_tower_signature(e):
    towers = getattr(e, "towers", None) or {}
    if "siglip" not in towers or "dino" not in towers:
        raise ValueError("this engine holds no tower weights to take a signature of (check_signature=False encodes a feature "
                         "set without the comparison)")
    parts = ["tdc-features-%d" % FORMAT, "out=%s" % getattr(e, "dtype", None), "res=%s" % getattr(e, "tower_res_dtype", None),
             "grid=%s" % (list(getattr(e, "out_grid", None) or []),)]
    for name in ("siglip", "dino"):
        t = towers[name]
        get = t.get if hasattr(t, "get") else (lambda k, d=None: d)
        parts.append("%s{dtype=%s,fp8=%d,ln_fuse=%d,w=%s}" % (name, get("dtype"), int(get("fp8") or 0), int(bool(get("fused"))),
                                                              weights_fingerprint(e, t)))
    return "|".join(parts)
