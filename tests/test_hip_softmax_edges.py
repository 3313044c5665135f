"""GPU (-m gpu): every attention kernel form under the adversarial softmax inputs of tests/softmax_cases.py, against fp64.

The value tests elsewhere feed `randn` q / k / v, whose softmax at these lengths is nearly uniform: the running maximum settles
in the first key tile and no single key decides a row.  Here the maximum moves late, sits on both sides of the deferred rescale's
threshold, the decisive key is the last valid key of a masked tile, the key behind a `k_len` or under a `key_mask`, one key
holds all or half of the weight, or every score is far negative.  The assertion is softmax_cases.BOUND (3 u A per element, derived
there) over all rows and over the planted rows; tests/test_softmax_cases.py shows on a CPU that a faithful online softmax keeps
it (1.75) and that the modelled defects miss it by orders of magnitude.  Each test prints `RATIO <form> <type> <all> <planted>`.

Shapes are the smallest that reach each instantiation (launch_qt / launch of attention.hip, tdc_attention32 of attention32.hip):
B = H = 2, at most 330 queries and keys."""
import math

import pytest
import torch

import softmax_cases as sc

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
B, H = 2, 2


@pytest.fixture(scope="module")
def ops():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops as o
    assert torch.cuda.is_available()
    return o


def to2d(ops, t, off=0):
    """[B, H, s, d] -> the [B * s, H * d] column view (offset `off` elements) of a zero-padded device buffer"""
    b, h, s, d = t.shape
    buf = torch.zeros(b * s, ops.pad64(h * d + off), dtype=t.dtype, device="cuda")
    buf[:, off:off + h * d] = t.permute(0, 2, 1, 3).reshape(b * s, h * d).cuda()
    return buf[:, off:off + h * d]


def from2d(x, b, h, s, d):
    return x.reshape(b, s, h, d).permute(0, 2, 1, 3).cpu()


def run_attention(ops, case, form=0, off=0, kv_index=None):
    b, h, sq, d = case.q.shape
    sk = case.k.shape[2]
    k, v = case.k, case.v
    if kv_index is not None:                     # item i reads slot kv_index[i]: store its K / V there
        slot = torch.empty(b, dtype=torch.long)
        slot[torch.tensor(kv_index)] = torch.arange(b)
        assert sorted(kv_index) == list(range(b))
        k, v = k[slot], v[slot]
    q2, k2, v2 = to2d(ops, case.q, off), to2d(ops, k, off), to2d(ops, v, off)
    out = torch.full((b * sq, ops.pad64(h * d + off)), 77.0, dtype=case.dtype, device="cuda")
    o2 = out[:, off:off + h * d]
    kw = {}
    if case.bias is not None:
        kw = dict(bias=case.bias.cuda().contiguous(), gate=case.gate.reshape(b * sq, h).cuda().contiguous())
        if case.key_mask is not None:
            kw["key_mask"] = case.key_mask.to(torch.uint8).cuda().contiguous()
    ops.attention(q2, k2, v2, o2, b, h, d, sq, sk, case.scale, sq * q2.stride(0), sk * k2.stride(0), sk * v2.stride(0),
                  sq * out.stride(0), form=form, k_len=case.k_len, kv_index=kv_index, **kw)
    torch.cuda.synchronize()
    assert (out[:, :off] == 77.0).all() and (out[:, off + h * d:] == 77.0).all()
    return from2d(o2, b, h, sq, d)


def check(case, got, worst):
    assert torch.isfinite(got.float()).all(), case.name
    r_all, r_pl = case.ratios(got)
    worst[0], worst[1] = max(worst[0], r_all), max(worst[1], r_pl)
    assert r_all <= sc.BOUND and r_pl <= sc.BOUND, (case.name, tuple(case.q.shape), case.k.shape[2], r_all, r_pl)
    if case.name == "one_hot":
        assert case.one_hot_error(got) <= sc.FLOOR, case.name


# attn_kernel<T, DK, NDV, QT, VEC, BIAS> instantiations: (label, head dim, sq, form, column offset of the views)
FORMS16 = [("qt1_dk64", 64, 40, 0, 0), ("qt2_dk64", 64, 100, 0, 0), ("qt2_dk96_d72", 72, 150, 0, 0), ("qt3_dk64", 64, 144, 0, 0),
           ("qt4_dk64", 64, 260, 1, 0), ("dk32_d16", 16, 40, 0, 0), ("dk64_d40", 40, 100, 0, 0), ("dk96_d80", 80, 40, 0, 0),
           ("elementwise_d12", 12, 100, 0, 0), ("elementwise_d64_offset4", 64, 100, 0, 4)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("label,d,sq,form,off", FORMS16, ids=[f[0] for f in FORMS16])
def test_attention_16x16_forms(ops, dtype, label, d, sq, form, off):
    """keys: 192 and 256 (exact tiles), 193 and 225 (last tiles of 1 and 33 keys)"""
    worst = [0.0, 0.0]
    for sk in (192, 193, 225, 256):
        for name in sc.NAMES:
            case = sc.make(name, B, H, sq, sk, d, dtype, tile=64)
            check(case, run_attention(ops, case, form=form, off=off), worst)
    print("RATIO 16x16x32 %s %s %.2f %.2f" % (label, dtype, worst[0], worst[1]))


# the 32x32x16 form under AUTO: head dim 64 (two query blocks per wave, register-staged), 80 (one block), 72 (two blocks, LDS-DMA)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("d", [64, 80, 72])
def test_attention_32x32_form(ops, dtype, d):
    """self-attention lengths 256 (exact), 257 (a second workgroup, last tile of 1 key), 289 (33 keys), 330 (10 keys); plants
    placed by 64-key tiles and by the 32-key blocks inside them"""
    worst = [0.0, 0.0]
    for S in (256, 257, 289, 330):
        for name in sc.NAMES:
            for tile in ((64, 32) if name in ("late_max", "threshold", "half_and_half") else (64,)):
                case = sc.make(name, B, H, S, S, d, dtype, tile=tile)
                check(case, run_attention(ops, case), worst)
    print("RATIO 32x32x16 d%d %s %.2f %.2f" % (d, dtype, worst[0], worst[1]))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("label,sq,sk,k_len", [("16x16", 100, 256, [193, 97]), ("32x32", 330, 330, [289, 130])])
def test_attention_k_len_and_kv_index(ops, dtype, label, sq, sk, k_len):
    """the winner is key k_len[b] - 1; a far larger key sits at k_len[b] and NaN behind it; the items read each other's slot"""
    worst = [0.0, 0.0]
    case = sc.make("k_len_edge", B, H, sq, sk, 64, dtype, k_len=k_len)
    check(case, run_attention(ops, case), worst)
    check(case, run_attention(ops, case, kv_index=[1, 0]), worst)
    print("RATIO k_len %s %s %.2f %.2f" % (label, dtype, worst[0], worst[1]))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("d", [16, 32, 64])
def test_attention_biased_form(ops, dtype, d):
    worst = [0.0, 0.0]
    for case in (sc.make_biased("late_max", B, H, 70, 196, d, dtype), sc.make_biased("late_max", B, H, 70, 196, d, dtype, masked=True),
                 sc.make_biased("masked_winner", B, H, 70, 196, d, dtype)):
        check(case, run_attention(ops, case), worst)
    print("RATIO biased d%d %s %.2f %.2f" % (d, dtype, worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------------ the scale contract
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("sq,sk", [(100, 256), (256, 256)])           # a 16x16x32 kernel; the 32x32x16 form
def test_attention_scale_contract(ops, dtype, sq, sk):
    """tdc_attn_desc.scale: negative or non-finite is refused and nothing is written; 0 gives the mean of V - exactly, with
    integer V and 256 keys (the sums and 1 / 256 are exact in fp32)"""
    case = sc.make("randn", B, H, sq, sk, 64, dtype)
    case.v = sc.make("one_hot", B, H, sq, sk, 64, dtype).v
    for bad in (-0.125, float("nan"), float("inf"), float("-inf")):
        case.scale = bad
        q2, k2, v2 = to2d(ops, case.q), to2d(ops, case.k), to2d(ops, case.v)
        out = torch.full((B * sq, H * 64), 77.0, dtype=dtype, device="cuda")
        with pytest.raises(RuntimeError, match="code -2"):            # TDC_E_BADARG
            ops.attention(q2, k2, v2, out, B, H, 64, sq, sk, bad, sq * q2.stride(0), sk * k2.stride(0), sk * v2.stride(0), sq * out.stride(0))
        torch.cuda.synchronize()
        assert (out == 77.0).all()
    case.scale = 0.0
    got = run_attention(ops, case)
    mean = case.v.double().mean(2, keepdim=True).to(dtype).expand(B, H, sq, 64)
    assert torch.equal(got, mean)
    ragged = sc.make("randn", B, H, sq, 193, 64, dtype)          # a masked last tile: 0 * -inf must not reach P
    ragged.scale = 0.0
    check(ragged, run_attention(ops, ragged, form=1 if sq < 256 else 0), [0.0, 0.0])


# ------------------------------------------------------------------------------------------------------ tdc_sva_attention
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("towers", [1, 2])
@pytest.mark.parametrize("dim,heads", [(1024, 16), (64, 16)])          # the 16-byte-access kernel; the element-wise one (head dim 4)
def test_sva_attention_decisive_keys(ops, dtype, dim, heads, towers):
    """T = 2, side = 3, r = 2: 18 queries over the 4 / 8 keys of their 2 x 2 windows.  Query i's decisive key is key i mod nkv
    (each position in turn), +25 base-2 units through column 0 of every head.  Softmax and PV run in fp32 in these kernels."""
    T, side, r = 2, 3, 2
    n, nq, nkv, hd = side * r, T * side * side, towers * r * r, dim // heads
    scale = 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(dim + towers)
    worst = [0.0, 0.0]

    def unwindow(x):                                         # [nq, r * r, C] -> the tower's token rows [T * n * n, C]
        return x.view(T, side, side, r, r, -1).permute(0, 1, 3, 2, 4, 5).reshape(T * n * n, -1)
    pos = torch.arange(nq) % nkv
    for variant in ("decisive", "decisive_masked", "all_but_one_masked", "far_negative"):
        q = torch.randn(nq, heads, 1, hd, generator=g)
        k = torch.randn(nq, heads, nkv, hd, generator=g)
        v = torch.randn(nq, heads, nkv, hd, generator=g)
        mask = torch.ones(nq, nkv, dtype=torch.bool)
        k[..., 0] = 0
        if variant == "far_negative":
            q[..., 0] = 16.0
            k[..., 0] = -250.0 / (16.0 * scale)
            mask = torch.rand(nq, nkv, generator=g) > 0.3
            mask[torch.arange(nq), pos] = True
        else:
            q[..., 0] = sc.QA
            k[torch.arange(nq), :, pos, 0] = 25.0 / (sc.QA * scale * sc.LOG2E)
            if variant == "decisive_masked":
                mask[torch.arange(nq), pos] = False
            if variant == "all_but_one_masked":
                mask[:] = False
                mask[torch.arange(nq), (3 * torch.arange(nq) + 1) % nkv] = True
        case = sc.Case(variant, q, k, v, scale, dtype, key_mask=~mask, p16=False)     # fp32 P: the plain bound, no subnormal term
        q2 = case.q.reshape(nq, dim).cuda()
        kv = []
        for tw in range(towers):
            kw = case.k[:, :, tw * r * r:(tw + 1) * r * r].permute(0, 2, 1, 3).reshape(nq, r * r, dim)
            vw = case.v[:, :, tw * r * r:(tw + 1) * r * r].permute(0, 2, 1, 3).reshape(nq, r * r, dim)
            kv.append(torch.cat([unwindow(kw), unwindow(vw)], 1).cuda().contiguous())
        out = ops.sva_attention(q2, kv, mask.to(torch.uint8).cuda().contiguous(), T, side, r, dim, heads)
        torch.cuda.synchronize()
        check(case, out[:, :dim].cpu().reshape(nq, 1, heads, hd).permute(0, 2, 1, 3), worst)
    print("RATIO sva dim%d towers%d %s %.2f %.2f" % (dim, towers, dtype, worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------------ tdc_qformer_xattn, fused
XD, XH, XK, XF = 768, 12, 16, 5


def xattn_operands(variant, Nenc, dtype, scale):
    """hidden rows h [F * K, 768] (they ARE q: Wq = identity, bq = 0), keys k [F * Nenc, 768], values v [F, heads, Nenc, 64]"""
    g = torch.Generator().manual_seed(Nenc)
    if variant == "one_hot":
        c = sc.make("one_hot", XF, XH, XK, Nenc, 64, dtype)
        q, k, v = c.q.float(), c.k.float(), c.v.float()
    else:                                                    # winner_is_last_key: key Nenc - 1 of the frame, +25 units
        q, k, v = (torch.randn(XF, XH, s, 64, generator=g) for s in (XK, Nenc, Nenc))
        q[..., 0] = 0
        k[..., 0] = 0
        q[:, :, ::3, 0] = sc.QA
        k[:, :, Nenc - 1, 0] = 25.0 / (sc.QA * scale * sc.LOG2E)
    return sc.Case(variant, q, k, v, scale, dtype, planted=None if variant == "one_hot" else torch.arange(0, XK, 3))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Nenc", [8, 20, 156, 220, 224])
@pytest.mark.parametrize("variant", ["one_hot", "winner_is_last_key"])
def test_qformer_xattn_fused_block_decisive_keys(ops, dtype, Nenc, variant):
    """Wq = Wo = identity (tiled), bq = bo = 0: q is the hidden row and the block returns LayerNorm(ctx + bv + h).  Where
    F * Nenc % 8 == 4 the 4 `vt` columns past F * Nenc that the kernel loads and masks hold NaN (0 * NaN would show a mask on
    the scores alone).  Against the fp64 block at the
    tolerances of test_hip_ops.py::test_qformer_xattn_fused_block, and against the three-kernel sequence (q GEMM, tdc_attention,
    output-projection form) on the same operands, at the same tolerance: the two paths round the same context (P once, ctx
    once) and share the projection and LayerNorm arithmetic, so they are no farther from each other than either is from fp64."""
    tol = 6e-3 if dtype == torch.float16 else 4e-2
    scale = 1.0 if variant == "one_hot" else 0.125
    case = xattn_operands(variant, Nenc, dtype, scale)
    dev = "cuda"
    g = torch.Generator().manual_seed(3)
    h16 = case.q.permute(0, 2, 1, 3).reshape(XF * XK, XD).to(dev).contiguous()
    h32 = h16.float().clone()
    k2 = case.k.permute(0, 2, 1, 3).reshape(XF * Nenc, XD).to(dev).contiguous()
    vrows = case.v.permute(0, 2, 1, 3).reshape(XF * Nenc, XD)                          # [F * Nenc, 768]
    vt = torch.zeros(XD, ops.pad64(XF * Nenc), dtype=dtype)
    vt[:, :XF * Nenc] = vrows.t()
    if (XF * Nenc) % 8 == 4:
        vt[:, XF * Nenc:XF * Nenc + 4] = float("nan")
    vt = vt.to(dev)
    eye = torch.eye(XD, dtype=dtype, device=dev)
    eye_t = ops.xattn_tile_weight(eye)
    zero = torch.zeros(XD, device=dev)
    bv = (0.1 * torch.randn(XD, generator=g)).to(dev)
    ln_g, ln_b = (1 + 0.1 * torch.randn(XD, generator=g)).to(dev), (0.1 * torch.randn(XD, generator=g)).to(dev)
    a16, a32 = h16.clone(), h32.clone()
    ops.qformer_xattn(a16, a32, XF, XK, XK, eye_t, zero, eye_t, zero, k2, vt, bv, Nenc, ln_g, ln_b, 1e-12, XD, XH, scale)
    torch.cuda.synchronize()
    assert torch.isfinite(a32).all()
    # fp64 block on the same operands (ctx rounded to the type as the kernel holds it)
    ref = case.reference()[0]
    ctx = (ref.permute(0, 2, 1, 3).reshape(XF * XK, XD) + bv.cpu().double()).to(dtype).double()
    y = torch.nn.functional.layer_norm(ctx + h32.cpu().double(), (XD,), ln_g.cpu().double(), ln_b.cpu().double(), 1e-12)
    err = (a32.cpu().double() - y).abs().max().item()
    # the three-kernel sequence
    q3 = ops.gemm(h16, eye, zero)
    ctx3 = torch.zeros(XF * XK, XD, dtype=dtype, device=dev)
    v3 = vrows.to(dev).contiguous()
    ops.attention(q3[:, :XD], k2, v3, ctx3, XF, XH, 64, XK, Nenc, scale, XK * q3.stride(0), Nenc * XD, Nenc * XD, XK * XD)
    ctx3 = (ctx3.float() + bv).to(dtype)
    b16, b32 = h16.clone(), h32.clone()
    ops.qformer_xattn_out(b16, b32, XF, XK, XK, ctx3, eye_t, zero, ln_g, ln_b, 1e-12, XD, XH)
    torch.cuda.synchronize()
    err3 = (a32 - b32).abs().max().item()
    print("XATTN %s Nenc %d %s: vs fp64 %.2e, vs the three-kernel sequence %.2e" % (variant, Nenc, dtype, err, err3))
    assert err < tol, err
    assert err3 < tol, err3
    assert torch.equal(a16, a32.to(dtype))


@pytest.mark.parametrize("dtype", DT)
def test_qformer_xattn_scale_contract(ops, dtype):
    Nenc = 20
    case = xattn_operands("winner_is_last_key", Nenc, dtype, 0.125)
    case.v = sc.make("one_hot", XF, XH, XK, Nenc, 64, dtype).v
    dev = "cuda"
    h16 = case.q.permute(0, 2, 1, 3).reshape(XF * XK, XD).to(dev).contiguous()
    h32 = h16.float().clone()
    k2 = case.k.permute(0, 2, 1, 3).reshape(XF * Nenc, XD).to(dev).contiguous()
    vt = torch.zeros(XD, ops.pad64(XF * Nenc), dtype=dtype)
    vt[:, :XF * Nenc] = case.v.permute(0, 2, 1, 3).reshape(XF * Nenc, XD).t()
    vt[:, XF * Nenc:XF * Nenc + 4] = float("nan")
    vt = vt.to(dev)
    eye_t = ops.xattn_tile_weight(torch.eye(XD, dtype=dtype, device=dev))
    zero, one = torch.zeros(XD, device=dev), torch.ones(XD, device=dev)
    for bad in (-0.125, float("nan"), float("inf")):
        a16, a32 = h16.clone(), h32.clone()
        with pytest.raises(RuntimeError, match="code -2"):            # TDC_E_BADARG
            ops.qformer_xattn(a16, a32, XF, XK, XK, eye_t, zero, eye_t, zero, k2, vt, None, Nenc, one, zero, 1e-12, XD, XH, bad)
        torch.cuda.synchronize()
        assert torch.equal(a16, h16) and torch.equal(a32, h32)
    # scale 0: ctx = the mean of the frame's V rows, rounded to the type
    a16, a32 = h16.clone(), h32.clone()
    ops.qformer_xattn(a16, a32, XF, XK, XK, eye_t, zero, eye_t, zero, k2, vt, None, Nenc, one, zero, 1e-12, XD, XH, 0.0)
    mean = case.v.double().mean(2, keepdim=True).to(dtype).expand(XF, XH, XK, 64).permute(0, 2, 1, 3).reshape(XF * XK, XD)
    y = torch.nn.functional.layer_norm(mean.double() + h32.cpu().double(), (XD,), None, None, 1e-12)
    assert (a32.cpu().double() - y).abs().max().item() < (6e-3 if dtype == torch.float16 else 4e-2)
