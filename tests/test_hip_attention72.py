"""Head-dim-72 tower attention (attention32.hip: two query blocks per wave, K / V tiles by LDS-DMA) against an fp32 torch
softmax reference, through ops.attention (run with -m gpu).

A workgroup covers 256 queries (4 waves x 2 blocks of 32) and walks the keys in tiles of 64 (2 blocks of 32); query blocks and
key blocks past the end of the sequence are skipped whole, so the sequence lengths below are the ones at which each of those
branches runs.  The tolerance is the one tests/test_hip_ops.py::test_attention applies to the same kernel form."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
B, H, D72 = 2, 2, 72
SCALE = 1.0 / math.sqrt(D72)


def tol(dtype):
    return 2 * (2e-3 if dtype == torch.float16 else 1.6e-2)


@pytest.fixture(scope="module")
def ops():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops as o
    assert torch.cuda.is_available()
    return o


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def make_qkv(ops, S, dtype, seed):
    """fused-QKV buffer as the towers hold it: [B * S, pad64(3 * H * d)], q | k | v side by side"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B * S, ops.pad64(3 * H * D72), device="cuda", generator=g).to(dtype)


def heads_of(t, S):
    return t.reshape(B, S, H, D72).transpose(1, 2).float()          # [B, H, S, d]


def reference(qkv, S, k_len=None, kv_index=None):
    D = H * D72
    q, k, v = (heads_of(qkv[:, i * D:(i + 1) * D], S) for i in range(3))
    if kv_index is not None:
        k, v = k[kv_index], v[kv_index]
    s = (q @ k.transpose(-1, -2)) * SCALE
    if k_len is not None:
        keys = torch.arange(S, device=s.device).view(1, 1, 1, S)
        s = s.masked_fill(keys >= torch.tensor(k_len, device=s.device).view(B, 1, 1, 1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * S, D)


def run(ops, qkv, S, **kw):
    D = H * D72
    ld = qkv.stride(0)
    out = torch.zeros(B * S, ops.pad64(D), device="cuda", dtype=qkv.dtype)
    ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], out, B, H, D72, S, S, SCALE,
                  S * ld, S * ld, S * ld, S * out.stride(0), **kw)
    assert torch.count_nonzero(out[:, D:]) == 0
    return out[:, :D]


# 256: exact tiles, the masked last tile has nothing to mask; 257: a second workgroup whose waves hold 1, 0, 0, 0 query
# blocks, last tile of 1 key; 289: last tile of 33 keys (two key blocks); 577: last workgroup 2, 1, 0, 0, last tile of 1 key;
# 729: the workload's own tail, 2, 2, 2, 1 and 25 keys
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("S", [256, 257, 289, 577, 729])
def test_sequence_lengths(ops, dtype, S):
    qkv = make_qkv(ops, S, dtype, 11 + S)
    err = relerr(run(ops, qkv, S), reference(qkv, S))
    print("S=%d %s relerr %.3e" % (S, dtype, err))
    assert err < tol(dtype)


@pytest.mark.parametrize("dtype", DT)
def test_per_item_key_counts_and_shared_source(ops, dtype):
    """items of 729 and 300 keys that both read the K / V of slot 0 (tdc_attn_desc.k_len / kv_index)"""
    S = 729
    qkv = make_qkv(ops, S, dtype, 5)
    k_len, kv_index = [729, 300], [0, 0]
    got = run(ops, qkv, S, k_len=k_len, kv_index=kv_index)
    err = relerr(got, reference(qkv, S, k_len, kv_index))
    print("k_len/kv_index %s relerr %.3e" % (dtype, err))
    assert err < tol(dtype)


@pytest.mark.parametrize("dtype", DT)
def test_running_maximum_moves_late(ops, dtype):
    """Bounded random scores never move the running maximum after the first tiles, so the deferred rescale (it follows a tile's
    maximum only when that exceeds the running one by more than 8 base-2 units) would go unexercised: every third query gets
    a key in tile 2 that beats everything before it by ~20 units and one in tile 5 that beats that one by ~9.5."""
    S = 729
    D = H * D72
    qkv = make_qkv(ops, S, dtype, 7)
    planted = torch.arange(0, B * S, 3, device="cuda")
    for h in range(H):
        qkv[:, h * D72] = 0
        qkv[planted, h * D72] = 4.0                                  # q column 0 of the planted queries
        qkv[:, D + h * D72] = 0                                      # k column 0: zero but for the two planted keys
        for b in range(B):
            qkv[b * S + 130, D + h * D72] = 30.0                     # tile 2: 4 * 30 / sqrt(72) * log2(e) = 20.4 units
            qkv[b * S + 325, D + h * D72] = 44.0                     # tile 5: 29.9 units
    got, ref = run(ops, qkv, S), reference(qkv, S)
    err, err_planted = relerr(got, ref), relerr(got[planted], ref[planted])
    print("late maximum %s relerr %.3e planted rows %.3e" % (dtype, err, err_planted))
    assert err_planted < tol(dtype)
    assert err < tol(dtype)


@pytest.mark.parametrize("dtype", DT)
def test_huge_last_key_columns_64_to_71(ops, dtype):
    """The QK^T contraction is 80 wide at head dim 72; what stands in for K columns 72-79 is a second copy of columns 64-71 and
    must meet zeros.  1e4 in those columns of the last key row (the row that also stands in for the keys past the end), with
    q chosen so that the true score of that key is ~4.6 and gives it ~10 % of the weight: counted twice it would take ~90 %."""
    S = 729
    D = H * D72
    qkv = make_qkv(ops, S, dtype, 9)
    for h in range(H):
        qkv[:, h * D72 + 64:h * D72 + 72] = 0
        qkv[:, h * D72 + 64] = 2.0 ** -8
        for b in range(B):
            qkv[b * S + S - 1, D + h * D72 + 64:D + h * D72 + 72] = 1e4
    got, ref = run(ops, qkv, S), reference(qkv, S)
    assert torch.isfinite(got.float()).all()
    err = relerr(got, ref)
    print("huge K columns %s relerr %.3e" % (dtype, err))
    assert err < tol(dtype)
