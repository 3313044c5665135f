"""Deterministic synthetic video used by the golden fixtures AND by the tests that replay them.

A video is `coef [T, NB] @ basis [NB, 3*px*px]` (fp32): only the small fp16 basis and the coefficient matrix are
stored in the fixture, the frames are rebuilt with the same formula on both sides.
"""
import re

import numpy as np


def make_basis_and_coef(T, px, nb=8, seed=0, scene_len=3):
    rng = np.random.RandomState(seed)
    basis = (rng.rand(nb, 3, px, px).astype(np.float32) * 2 - 1).astype(np.float16)
    coef = np.zeros((T, nb), dtype=np.float32)
    scene = 0
    for t in range(T):
        if t > 0 and t % scene_len == 0:
            scene = (scene + 1 + rng.randint(0, nb - 1)) % nb
        coef[t, scene] = 1.0
        coef[t] += (0.02 * (t % scene_len + 1)) * rng.randn(nb).astype(np.float32)
    return basis, coef


def video_from_basis(basis, coef):
    nb = basis.shape[0]
    flat = basis.astype(np.float32).reshape(nb, -1)
    vid = coef.astype(np.float32) @ flat
    return vid.reshape((coef.shape[0],) + basis.shape[1:]).astype(np.float32)


class FakeBeats:
    """Stand-in for BEATs.extract_features (tdc/audio_models/beats/BEATs.py:131-178; needs torchaudio, absent in the
    build container): deterministic [1, n, 768] features with n = floor(seconds * 49.6) - a full 10-s window gives 496
    frames, so its last second has 46 tokens and takes the reference's adaptive_avg_pool2d branch
    (tdc/cambrian_arch.py:1567-1568).  Used by make_golden.py (plugged into the reference) and by the tests."""

    def extract_features(self, wav, padding_mask=None, feature_only=True):
        import torch
        n = int(wav.shape[1] / 16000.0 * 49.6)
        seg = wav[0, : n * 320].reshape(n, 320)
        base = seg.mean(1, keepdim=True) * 50.0 + seg.std(1, keepdim=True)
        emb = torch.sin(base * torch.arange(1, 769).float()[None] * 0.37) + base
        return emb[None], None


def beats_windows(wav, dist=10, sr=16000):
    """BEATs features of the consecutive 10-s windows of wav [1, n] (tdc/cambrian_arch.py:1552-1560)."""
    out = []
    for k in range(0, int(wav.shape[1] / sr), dist):
        out.append(FakeBeats().extract_features(wav[:, sr * k: sr * (k + dist)])[0])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Hash-filled weights and inputs of the full-dimension fixtures (make_golden_fulldim.py, test_oracle_golden.py
# test_fulldim_*, test_hip_fulldim.py).  Integer arithmetic only: element i of the tensor `name` comes from
# splitmix64(fnv1a64(name) + (i + 1) * 0x9E3779B97F4A7C15), whose top 24 bits are an exact fp32 in [-1, 1); a rule per
# kind of parameter scales it.  No RNG state of numpy or torch is involved, so every machine with numpy gets the same bits.
_M64 = (1 << 64) - 1
_CHUNK = 1 << 22


def name_hash(name):
    """FNV-1a 64 of the UTF-8 bytes of `name`."""
    h = 0xCBF29CE484222325
    for b in name.encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) & _M64
    return h


def _unit_into(out, seed, lo):
    with np.errstate(over="ignore"):
        z = np.arange(lo + 1, lo + len(out) + 1, dtype=np.uint64)
        z *= np.uint64(0x9E3779B97F4A7C15)
        z += seed
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        z >>= np.uint64(40)
    out[:] = z
    out *= np.float32(2.0 ** -23)
    out -= np.float32(1.0)


def unit(name, n, pool=None):
    """n fp32 values in [-1, 1) of the stream `name` (chunks on `pool`, a thread pool, when given)."""
    seed = np.uint64(name_hash(name))
    out = np.empty(n, dtype=np.float32)
    parts = [(out[lo:lo + _CHUNK], seed, lo) for lo in range(0, n, _CHUNK)]
    if pool is None or len(parts) == 1:
        for a in parts:
            _unit_into(*a)
    else:
        list(pool.map(lambda a: _unit_into(*a), parts))
    return out


# kind -> (scale, offset): value = offset + scale * u.  "linear" scales by sqrt(3 / fan_in), so that a block fed unit-RMS
# rows writes unit-RMS rows: every attention and MLP block adds about as much to the residual stream as it already holds,
# and a wrong head, row tile or mask moves the output by a sizeable fraction of max|ref| (HF's init, std 0.02, leaves
# the blocks a small correction to a dominant residual).
KIND_RULES = {
    "bias": (0.1, 0.0), "ln_weight": (0.2, 1.0), "ln_bias": (0.1, 0.0), "layerscale": (0.3, 1.0),
    "pos_embed": (0.5, 0.0), "cls_token": (1.0, 0.0), "vision_query": (1.0, 0.0), "image_newline": (1.0, 0.0),
    "frame_seg": (1.0, 0.0), "word_embed": (1.0, 0.0), "pixels": (1.0, 0.0), "features": (1.0, 0.0),
}


def kind_of(name, shape):
    """The scale rule of a reference-named parameter."""
    leaf = name.rsplit(".", 1)[-1]
    if name.endswith("lambda1"):
        return "layerscale"
    if "position_embedding" in name or "pos_embed_" in name:
        return "pos_embed"
    if name.endswith("cls_token"):
        return "cls_token"
    if name in ("vision_query", "image_newline", "frame_seg"):
        return name
    if "word_embeddings" in name:
        return "word_embed"
    if len(shape) == 1:     # LayerNorm (ln_* / norm* / LayerNorm / layernorm / *_proj_*.0 / mm_projector_aux_*.3) or bias
        if ("norm" in name.lower() or re.search(r"_proj(_\d+)?\.0\.(weight|bias)$", name)
                or re.match(r"mm_projector_aux_\d+\.3\.", name)):
            return "ln_weight" if leaf == "weight" else "ln_bias"
        return "bias"
    return "linear"


def fill(name, shape, kind=None, pool=None):
    """Deterministic fp32 tensor (numpy) of `shape` for the parameter / input `name`, scaled by its kind's rule."""
    shape = tuple(int(s) for s in shape)
    kind = kind or kind_of(name, shape)
    n = int(np.prod(shape)) if shape else 1
    u = unit(name, n, pool)
    if kind == "linear":
        fan_in = int(np.prod(shape[1:]))
        u *= np.float32((3.0 / fan_in) ** 0.5)
    else:
        scale, offset = KIND_RULES[kind]
        u *= np.float32(scale)
        if offset:
            u += np.float32(offset)
    return u.reshape(shape)


def fulldim_shapes(layers_siglip, layers_dino, H=3584, K=144):
    """key -> shape of the model bench.py runs (bench.random_state_dict on the meta device), towers cut to their first
    layers_siglip / layers_dino layers."""
    import os
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    sd = bench.random_state_dict(H, K, torch.device("meta"), None)
    out = {}
    for k, v in sd.items():
        for pre, n in (("vision_tower_aux_list.0.vision_tower.encoder.layers.", layers_siglip),
                       ("vision_tower_aux_list.1.vision_tower.encoder.layer.", layers_dino)):
            if k.startswith(pre) and int(k[len(pre):].split(".")[0]) >= n:
                break
        else:
            out[k] = tuple(v.shape)
    return out


def synth_state_dict(layers_siglip, layers_dino, prefixes=None, H=3584, K=144):
    """Reference-named fp32 state dict (torch tensors) of the full-dimension model with hash-filled weights; `prefixes`
    restricts it to the keys starting with one of them (the weights of one stage are cheaper to make than all 0.4 G)."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    shapes = fulldim_shapes(layers_siglip, layers_dino, H, K)
    if prefixes is not None:
        shapes = {k: s for k, s in shapes.items() if k.startswith(tuple(prefixes))}
    with ThreadPoolExecutor(8) as pool:
        return {k: torch.from_numpy(fill(k, s, pool=pool)) for k, s in shapes.items()}


def synth_input(name, shape):
    """Pixels ([-1, 1)) or synthetic features (kind "features") from the same hash as the weights."""
    return torch_from(fill(name, shape, "pixels" if name.startswith("pixels") else "features"))


def torch_from(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------------------------
# Digests: what the full-dimension fixtures store of an output x, viewed as rows [R, D] (D = last dimension).  They see
# every row (its L2 norm) and every column (its sum), plus a few full rows where row tiles of 64 / 128 / 256 begin, end or
# run ragged, and a strided sample of the elements.
def digest_rows(R):
    """Row indices kept in full: first, last, 63 / 64, 127 / 128, 255 / 256 and the first and last rows of the ragged last
    64- and 256-row tiles."""
    idx = {0, R - 1, 63, 64, 127, 128, 255, 256}
    for tile in (64, 256):
        if R % tile:
            idx.update((R // tile * tile, R - 1))
    return np.array(sorted(i for i in idx if 0 <= i < R), dtype=np.int64)


def digest(x, n_sample=4096):
    x = np.asarray(x, dtype=np.float64)
    x2 = x.reshape(-1, x.shape[-1])
    R = x2.shape[0]
    flat = x2.reshape(-1)
    stride = max(1, len(flat) // n_sample)
    sidx = (np.arange(min(n_sample, len(flat)), dtype=np.int64) * stride + stride // 2) % len(flat)
    ridx = digest_rows(R)
    return dict(shape=np.array(x.shape, dtype=np.int64), sumsq=np.array((x2 * x2).sum()),
                maxabs=np.array(np.abs(x2).max()), row_norm=np.sqrt((x2 * x2).sum(1)), col_sum=x2.sum(0),
                row_idx=ridx, rows=x2[ridx].astype(np.float32), sample_idx=sidx, sample=flat[sidx].astype(np.float32))


def save_digest(arrs, key, x):
    for k, v in digest(x).items():
        arrs[key + "/" + k] = v


def load_digest(z, key):
    return {k[len(key) + 1:]: z[k] for k in z.files if k.startswith(key + "/")}


def digest_errors(d, x):
    """Errors of x against the digest d, each normalised by the scale of its field:
       sumsq, maxabs   relative;
       row_norm        per row, relative to that row's reference norm;
       col_sum         per column, relative to R * max|ref|: the error of each column's mean, of max|ref| (16-bit
                       weights and biases err alike in every row of a column, so column errors add up linearly in R);
       rows, sample    abs, relative to max|ref|."""
    x = np.asarray(x, dtype=np.float64)
    assert tuple(x.shape) == tuple(int(s) for s in d["shape"]), (x.shape, d["shape"])
    x2 = x.reshape(-1, x.shape[-1])
    R, D = x2.shape
    mx = float(d["maxabs"])
    rn = np.sqrt((x2 * x2).sum(1))
    return dict(
        sumsq=abs(float((x2 * x2).sum()) - float(d["sumsq"])) / float(d["sumsq"]),
        maxabs=abs(float(np.abs(x2).max()) - mx) / mx,
        row_norm=float((np.abs(rn - d["row_norm"]) / np.maximum(d["row_norm"], 1e-30)).max()),
        col_sum=float(np.abs(x2.sum(0) - d["col_sum"]).max()) / (R * mx),
        rows=float(np.abs(x2[d["row_idx"]] - d["rows"]).max()) / mx,
        sample=float(np.abs(x2.reshape(-1)[d["sample_idx"]] - d["sample"]).max()) / mx)
