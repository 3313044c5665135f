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

FORMAT = 1                  # lossless sets: the 16-bit rows
FORMAT_COMPACT = 2          # compact sets: e4m3 bytes, one fp32 scale per token row, the exact a5 similarities (section 14)
FORMAT_GAPS = 3             # format 2 plus gap_sims, the similarities across gaps 1 .. G (section 16); written only with a table
ROWS_DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


class FeatureSet:
    """siglip [T0, P, Ds], dino [T0, P, Dd] (16-bit, the type the towers emit; P = 576 at full size), image_size (the source
    image size the connector un-pads by), signature (tower_signature of the exporting engine; None: unknown).  store = "f16".

    The compact form (store = "e4m3"; VideoEncoder.export_features(store="e4m3") / compact_features):
    siglip / dino are uint8 [T0, P, D] - OCP e4m3 bytes, plain uint8 so that loading depends on no torch float8 type -,
    siglip_scale / dino_scale fp32 [T0, P] (row = float(byte) * scale), sims fp32 [T0 - 1] - the a5 similarities of the ORIGINAL
    16-bit DINOv2 rows of all T0 frames (None for one frame), so that a lossy store never moves the frame selection - and
    rows_dtype, the 16-bit type the rows decode to.  The signature stays the towers': the store form is a property of the set.
    gap_sims (compact sets only): fp32 [G, T0 - 1], row g - 1, entry i = cos(f_i, f_{i+g}) of the ORIGINAL
    rows for i + g < T0, every other entry 0.0; row 0 is sims (taken from it when sims is not given).  With it a call whose a1
    sub-samples still selects on the original rows' similarities (stored_sims)."""

    def __init__(self, siglip, dino, image_size, signature=None, siglip_scale=None, dino_scale=None, sims=None, rows_dtype=None,
                 gap_sims=None):
        if not (torch.is_tensor(siglip) and torch.is_tensor(dino) and siglip.dim() == 3 and dino.dim() == 3):
            raise ValueError("a FeatureSet holds two [frames, tokens, width] tensors")
        if siglip.shape[:2] != dino.shape[:2] or siglip.shape[0] < 1:
            raise ValueError("SigLIP features %s and DINOv2 features %s do not describe the same frames"
                             % (tuple(siglip.shape), tuple(dino.shape)))
        compact = siglip_scale is not None or dino_scale is not None or siglip.dtype == torch.uint8 or dino.dtype == torch.uint8
        if compact:
            if siglip.dtype != torch.uint8 or dino.dtype != torch.uint8:
                raise ValueError("feature types %s / %s: a compact set holds e4m3 bytes as uint8 in both towers"
                                 % (siglip.dtype, dino.dtype))
            for name, sc in (("siglip_scale", siglip_scale), ("dino_scale", dino_scale)):
                if not (torch.is_tensor(sc) and sc.dtype == torch.float32 and tuple(sc.shape) == tuple(siglip.shape[:2])):
                    raise ValueError("%s: a compact set holds one fp32 scale per token row, %s; got %s"
                                     % (name, tuple(siglip.shape[:2]), "%s %s" % (sc.dtype, tuple(sc.shape))
                                        if torch.is_tensor(sc) else type(sc).__name__))
            if sims is not None and not (torch.is_tensor(sims) and sims.dtype == torch.float32
                                         and tuple(sims.shape) == (siglip.shape[0] - 1,)):
                raise ValueError("sims: the %d fp32 adjacent-frame similarities of %d frames" % (siglip.shape[0] - 1, siglip.shape[0]))
            if sims is not None and sims.numel() == 0:
                sims = None
            if gap_sims is not None:
                if not (torch.is_tensor(gap_sims) and gap_sims.dtype == torch.float32 and gap_sims.dim() == 2
                        and gap_sims.shape[0] >= 1 and siglip.shape[0] > 1 and gap_sims.shape[1] == siglip.shape[0] - 1):
                    raise ValueError("gap_sims: an fp32 [G, %d] table of the similarities across gaps 1 .. G of %d frames, "
                                     "G >= 1" % (siglip.shape[0] - 1, siglip.shape[0]))
                if sims is None:
                    sims = gap_sims[0]
                elif not torch.equal(gap_sims[0].to(sims.device), sims):
                    raise ValueError("gap_sims: row 0 holds the adjacent-frame similarities and must equal sims")
            if isinstance(rows_dtype, str):
                rows_dtype = ROWS_DTYPES.get(rows_dtype)
            if rows_dtype not in ROWS_DTYPES.values():
                raise ValueError("rows_dtype %r: the type the rows of a compact set decode to, fp16 or bf16" % (rows_dtype,))
        else:
            # fp32: the CPU engine doubles of the tests; VideoEncoder.feature_rows takes the engine's own 16-bit type only
            if siglip.dtype != dino.dtype or siglip.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                raise ValueError("feature types %s / %s: both towers emit one type, fp16 or bf16" % (siglip.dtype, dino.dtype))
            if sims is not None or gap_sims is not None or rows_dtype not in (None, siglip.dtype):
                raise ValueError("a lossless set holds neither similarities nor a rows_dtype of its own")
            rows_dtype = siglip.dtype
        self.siglip, self.dino = siglip, dino
        self.siglip_scale, self.dino_scale, self.sims, self.rows_dtype = siglip_scale, dino_scale, sims, rows_dtype
        self.gap_sims = gap_sims
        self.store = "e4m3" if compact else "f16"
        self.image_size = tuple(int(v) for v in image_size)
        self.signature = None if signature is None else str(signature)

    @property
    def frames(self):
        return int(self.siglip.shape[0])

    @property
    def gaps(self):
        """the largest frame gap whose similarities the set holds: G with a table, 1 with sims alone, else 0"""
        if self.gap_sims is not None:
            return int(self.gap_sims.shape[0])
        return 1 if self.sims is not None else 0

    def tensors(self):
        """every tensor the set holds, by attribute name"""
        names = ("siglip", "dino", "siglip_scale", "dino_scale", "sims", "gap_sims")
        return {k: getattr(self, k) for k in names if getattr(self, k) is not None}

    def _with(self, f):
        t = {k: f(v) for k, v in self.tensors().items()}
        if self.store == "f16":
            return FeatureSet(t["siglip"], t["dino"], self.image_size, self.signature)
        return FeatureSet(t["siglip"], t["dino"], self.image_size, self.signature, t["siglip_scale"], t["dino_scale"],
                          t.get("sims"), self.rows_dtype, t.get("gap_sims"))

    def clip(self, lo, hi):
        """the set of the frames [lo, hi) (views, both stores): the rows, the scales, sims[lo:hi - 1] and the table cut to
        G' = min(G, hi - lo - 1) gaps with the entries that reach past hi set to 0 - what an export of those frames alone holds.
        image_size and the signature are kept."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= self.frames:
            raise ValueError("clip: frames [%d, %d) of a %d-frame set" % (lo, hi, self.frames))
        if self.store == "f16":
            return FeatureSet(self.siglip[lo:hi], self.dino[lo:hi], self.image_size, self.signature)
        n = hi - lo
        sims = self.sims[lo:hi - 1] if self.sims is not None and n > 1 else None
        table = None
        if self.gap_sims is not None and n > 1:
            table = self.gap_sims[:min(self.gaps, n - 1), lo:hi - 1].clone()
            for g in range(2, table.shape[0] + 1):          # row g - 1: entries i + g >= n look past the last kept frame
                table[g - 1, n - g:] = 0.0
        return FeatureSet(self.siglip[lo:hi], self.dino[lo:hi], self.image_size, self.signature, self.siglip_scale[lo:hi],
                          self.dino_scale[lo:hi], sims, self.rows_dtype, table)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.tensors().values())

    def to(self, device):
        """the set with its tensors on `device` (itself when they already are)"""
        device = torch.device(device)
        if all(t.device == device for t in self.tensors().values()):
            return self
        return self._with(lambda t: t.to(device))

    def cpu(self):
        """the set in host memory - pinned when CUDA is available, so .to(device) is one DMA per tensor"""
        def host(t):
            if t.device.type == "cpu" and (t.is_pinned() or not torch.cuda.is_available()):
                return t
            out = torch.empty(t.shape, dtype=t.dtype, pin_memory=torch.cuda.is_available())
            return out.copy_(t)
        return self._with(host)

    def save(self, path):
        """a plain dict of tensors, ints and strings through torch.save: no pickled class, loads with weights_only=True.
        Lossless sets are format 1, as they always were; compact sets are format 2, format 3 when they hold a gap table."""
        def compact(t):                         # a copy that owns exactly its bytes (a view would drag its whole storage along)
            return t.detach().to("cpu").clone(memory_format=torch.contiguous_format)
        d = dict(format=FORMAT, siglip=compact(self.siglip), dino=compact(self.dino),
                 image_size=[int(v) for v in self.image_size], signature=self.signature or "")
        if self.store == "e4m3":
            d.update(format=FORMAT_COMPACT, store="e4m3", siglip_scale=compact(self.siglip_scale),
                     dino_scale=compact(self.dino_scale), rows_dtype=str(self.rows_dtype).replace("torch.", ""),
                     sims=compact(self.sims) if self.sims is not None else torch.empty(0, dtype=torch.float32))
            if self.gap_sims is not None:
                d.update(format=FORMAT_GAPS, gap_sims=compact(self.gap_sims))
        torch.save(d, path)

    @classmethod
    def load(cls, path, map_location="cpu"):
        d = torch.load(path, map_location=map_location, weights_only=True)
        if isinstance(d, dict) and d.get("format") in (FORMAT_COMPACT, FORMAT_GAPS) and d.get("store") == "e4m3":
            return cls(d["siglip"], d["dino"], d["image_size"], d["signature"] or None, d["siglip_scale"], d["dino_scale"],
                       d["sims"] if d["sims"].numel() else None, d["rows_dtype"],
                       d["gap_sims"] if d["format"] == FORMAT_GAPS else None)
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise ValueError("%s is not a FeatureSet file of format %d, %d or %d" % (path, FORMAT, FORMAT_COMPACT, FORMAT_GAPS))
        return cls(d["siglip"], d["dino"], d["image_size"], d["signature"] or None)


def is_feature_set(x):
    """a FeatureSet by what it holds (the package is importable under two names, so its class is not compared); both stores"""
    return all(hasattr(x, k) for k in ("siglip", "dino", "image_size", "signature", "frames")) and not torch.is_tensor(x)


def is_compact(fs):
    return getattr(fs, "store", "f16") == "e4m3"


def stored_sims(fs, idx):
    """the a5 similarities of the kept frames idx (ascending) from what the set stores: the host list of cos(idx[k], idx[k + 1])
    of the ORIGINAL 16-bit rows, or None when some gap is wider than the set holds (fs.gaps) - then a5 has to launch.  Gap 1
    reads sims, wider gaps the table."""
    G = getattr(fs, "gaps", 0)
    if len(idx) < 2 or G < 1:
        return None
    gap = [b - a for a, b in zip(idx[:-1], idx[1:])]
    if min(gap) < 1 or max(gap) > G:
        return None
    if max(gap) == 1:
        return fs.sims[idx[0]:idx[-1]].tolist()
    dev = fs.gap_sims.device                    # a table on the device: only the T - 1 entries cross
    g = torch.tensor(gap, dtype=torch.long).to(dev)
    i = torch.tensor(list(idx[:-1]), dtype=torch.long).to(dev)
    return fs.gap_sims[g - 1, i].tolist()


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
