"""GPU: the HIP path directly against digests of the REFERENCE's outputs at the model's real dimensions
(tests/golden/fulldim_*.npz, written by tests/golden/make_golden_fulldim.py; run with -m gpu).

test_hip_fullsize.py compares the HIP path with the fp32 oracle, and test_oracle_golden.py pins the oracle to the reference
at toy sizes and, through the same digests as here, at these sizes.  This file closes the loop without the oracle: the same
hash-filled weights and inputs (synth.synth_state_dict, towers cut to 4 layers) go through VideoEncoder and every digest
field is compared - every row's L2 norm and every column's sum, full rows where 64 / 128 / 256-row tiles begin, end and run
ragged, a strided sample - so a wrong row tile, last head or mask cannot hide below a tolerance relative to max|ref|.
Errors are synth.digest_errors' normalised ones (rows / sample / maxabs: of max|ref|; row_norm: of each row's own norm;
col_sum: each column's mean, of max|ref|; sumsq: relative)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, GOLDEN):
    if p not in sys.path:
        sys.path.insert(0, p)
import synth  # noqa: E402

H = 3584


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(4, 4)


def digest(name, key):
    z = np.load(os.path.join(GOLDEN, name))
    return synth.load_digest(z, key), z


def check(label, d, x, tol, bad):
    """every digest field within tol[field] (a float: the same bound for all fields); misses are added to `bad`"""
    e = synth.digest_errors(d, x.double().cpu().numpy())
    tol = tol if isinstance(tol, dict) else {k: tol for k in e}
    print("%s: %s" % (label, " ".join("%s %.2e" % kv for kv in e.items())))
    bad.update({(label, k): (v, tol[k]) for k, v in e.items() if not v <= tol[k]})
    return e


def encoder(sd, dtype, K=144, **kw):
    import bench
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd.pipeline import VideoEncoder
    cfg = dict(bench.model_cfg(H, K, 8), context_token_num=K)
    return VideoEncoder(sd, cfg, dtype=dtype, device="cuda:0", selection_refine=False, **kw)


# about 2x the errors measured on an MI355X (max over both towers and ln_fuse off / on), all below test_hip_fullsize's tower bound
# (fp16 4e-3, bf16 3e-2 of max|ref|).  Measured fp16: sumsq 1.0e-5, maxabs 5.1e-5, row_norm 6.7e-5, col_sum 2.6e-4,
# rows 7.9e-4, sample 8.6e-4; bf16: sumsq 3.6e-4, maxabs 3.3e-3, row_norm 5.9e-4, col_sum 2.4e-3, rows 6.6e-3, sample 4.9e-3.
TOWER_TOL = {torch.float16: dict(sumsq=2.5e-5, maxabs=1.2e-4, row_norm=1.5e-4, col_sum=6e-4, rows=1.8e-3, sample=1.8e-3),
             torch.bfloat16: dict(sumsq=8e-4, maxabs=7e-3, row_norm=1.2e-3, col_sum=5e-3, rows=1.4e-2, sample=1.4e-2)}


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fulldim_towers(sd, dtype, fuse):
    """SigLIP-so400m and DINOv2-giant widths (4 layers), 2 frames each, with the LayerNorm-kernel and the folded-LayerNorm
    (ln_fuse) towers."""
    enc = encoder(sd, dtype, tower_batch=2, ln_fuse=fuse)
    assert all(bool(t.fused) == fuse for t in enc.towers.values())
    bad = {}
    for name, fixture, px, D in (("siglip", "fulldim_siglip.npz", (2, 3, 384, 384), 1152),
                                 ("dino", "fulldim_dino.npz", (2, 3, 378, 378), 1536)):
        x = synth.synth_input("pixels/" + name, px).cuda()
        got = enc.tower(name, x)[:, :D].float().reshape(2, 576, D)
        check("%s %s ln_fuse=%d" % (name, dtype, fuse), digest(fixture, "out")[0], got, TOWER_TOL[dtype], bad)
    assert not bad, bad


# about 2x the errors measured on an MI355X (max over square / 16:9), all below test_hip_ops.py::test_sva_attention's bound
# (2 x tol(dtype): fp16 4e-3, bf16 3.2e-2 of max|ref|).  Measured fp16: sumsq 2.2e-5, maxabs 2.1e-4, row_norm 1.0e-4,
# col_sum 2.3e-4, rows 7.4e-4, sample 8.1e-4; bf16: sumsq 9.4e-6, maxabs 1.2e-3, row_norm 9.4e-4, col_sum 1.7e-3, rows 5.7e-3,
# sample 5.4e-3.
SVA_TOL = {torch.float16: dict(sumsq=5e-5, maxabs=5e-4, row_norm=2.5e-4, col_sum=5e-4, rows=1.6e-3, sample=1.6e-3),
           torch.bfloat16: dict(sumsq=3e-5, maxabs=2.5e-3, row_norm=2e-3, col_sum=3.5e-3, rows=1.2e-2, sample=1.2e-2)}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fulldim_sva(sd, dtype):
    """The SVA (3 layers, C = 1024, 12 x 12 windows of 2 x 2 keys per tower) on 3 frames of synthetic aux features, square and
    16:9 (360, 640): the window masks (bit for bit) and the queries it writes."""
    from tdc_video_amd.weights import pad64
    enc = encoder({k: v for k, v in sd.items() if not k.startswith("vision_tower_aux_list.")}, dtype)
    T, C = 3, 1024
    aux, bad = [], {}
    for i in range(2):
        a = torch.zeros(T * 576, pad64(C), dtype=dtype, device="cuda:0")
        a[:, :C] = synth.synth_input("features/sva_aux%d" % i, (T, 576, C)).reshape(T * 576, C).to(dtype).cuda()
        aux.append(a)
    for tag, size in (("square", (384, 384)), ("wide", (360, 640))):
        d, z = digest("fulldim_sva.npz", "out_" + tag)
        mask, r = enc._window_mask(T, 576, [size] * T)
        assert r == 2
        want = np.concatenate([z["mask0_" + tag], z["mask1_" + tag]], -1)
        assert np.array_equal(mask.cpu().numpy().astype(bool), want)
        got = enc.sva(aux, T, [size] * T)[:, :C].float().reshape(T, 144, C)
        check("sva %s %s" % (tag, dtype), d, got, SVA_TOL[dtype], bad)
    assert not bad, bad


# compressed tokens (unit-norm rows, max|ref| 0.065 ... 0.079): about 2x the errors measured on an MI355X, all below the 1e-3
# absolute of test_hip_fullsize's compressor tests.  Measured (max over the three cases): rows / sample 8.1e-5 absolute,
# maxabs 4.4e-4 of max|ref|, row_norm 3.2e-5, col_sum 7.1e-4 of max|ref|, sumsq 1.2e-6.
COMP_ABS = 2e-4


@pytest.mark.parametrize("K,N", [(144, 156), (16, 156), (16, 84)])
def test_fulldim_qformer(sd, K, N):
    """One 8-frame chunk through the whole a11-a19 path (fp16): key frame pooled to K windows, query_proj, the bert-base
    Q-Former (12 layers, cross-attention to N tokens of H = 3584), vision_proj, L2 norm.  The key frame's N rows are emitted
    verbatim; the 7 other frames' compressed rows are compared with the reference's digest."""
    W = {k: v for k, v in sd.items() if not k.startswith("vision_tower_aux_list.")}
    enc = encoder(W, torch.float16, K=K)
    d, z = digest("fulldim_qformer.npz", "out_K%d_N%d" % (K, N))
    chunk = synth.synth_input("features/qformer_N%d" % N, (8, N, H))
    X = chunk.reshape(8 * N, H).half().cuda().contiguous()
    pid = [int(i) for i in z["prompt_ids"]]
    keep = {}
    out = enc.compress(X, 8, N, [], pid, 10 ** 9, keep=keep)
    plan = keep["plan"]
    assert list(plan["comp_frames"]) == list(range(1, 8)) and out.shape == ((N + 1) + 7 * (K + 1), H)
    assert torch.equal(out[:N], X[:N])                                                    # the key frame, verbatim
    got = keep["compressed"][: 7 * K, :H].float().reshape(7, K, H)
    mx = float(d["maxabs"])
    R = 7 * K
    tol = dict(rows=COMP_ABS / mx, sample=COMP_ABS / mx, maxabs=1e-3, row_norm=8e-5, col_sum=1.5e-3, sumsq=3e-6)
    bad = {}
    e = check("qformer K=%d N=%d" % (K, N), d, got, tol, bad)
    print("   as absolute errors: rows %.2e sample %.2e (max|ref| %.3f, R = %d)" % (e["rows"] * mx, e["sample"] * mx, mx, R))
    assert not bad, bad
