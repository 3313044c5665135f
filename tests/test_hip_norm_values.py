"""GPU (-m gpu): the LayerNorm kernels, tdc_qformer_embed and tdc_l2_normalize under the designed rows of tests/gemm_cases.py,
against fp64, element by element:

    |got - ref| <= BOUND (u_out |ref| + KAPPA_LN 2^-24 (rstd |gamma| (|x| + |mean|) + |beta|) + FLOOR)

once with the derived KAPPA_LN = cols + 4 and once with the tight one measured on the two-pass CPU emulation
(tests/test_gemm_cases.py, where the one-pass variance E[x^2] - mean^2 misses it tenfold).  Rows: mean 64 with deviations of a few
16-bit spacings, an outlier channel, constant rows (the output is beta up to the rstd |gamma| 2^-24 |c| of the mean's own rounding),
variance far below eps, and +-a rows whose variance is a^2 exactly.  9 rows (not a multiple of the 4 rows per block); widths on both
sides of every instantiation boundary of launch_ln / launch_ln16 / tdc_qformer_embed; the pad columns up to round_up(cols, 64) must
be zero and nothing behind them written.  Each test prints `RATIO <kernel> <rows> <type> <tight> <derived>`."""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

DT = [gc.F16, gc.BF16]
TN = {gc.F16: "fp16", gc.BF16: "bf16", gc.F32: "fp32"}
ROWS = 9
SENT = 77.0
COLS32 = (4, 60, 256, 260, 768, 772, 1024, 1028, 1280, 1284, 1536, 1540, 4096)
COLS16 = (8, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 4096)


@pytest.fixture(scope="module")
def ops():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops as o
    assert torch.cuda.is_available()
    return o


def padded(ops, x):
    """rows as stored -> the zero-padded device matrix [rows, round_up(cols, 64)]"""
    buf = torch.zeros(x.shape[0], ops.pad64(x.shape[1]), dtype=x.dtype, device="cuda")
    buf[:, :x.shape[1]] = x.cuda()
    return buf


def check_ln(got, ref, T, cols, out_dtype, worst):
    assert torch.isfinite(got.float()).all()
    tight = gc.ln_ratio(got[:, :cols], ref, T, out_dtype, gc.KAPPA_LN)
    derived = gc.ln_ratio(got[:, :cols], ref, T, out_dtype, gc.kappa_ln_derived(cols))
    worst[0], worst[1] = max(worst[0], tight), max(worst[1], derived)
    assert derived <= gc.bound(out_dtype), ("derived KAPPA_LN", cols, derived)
    assert tight <= gc.bound(out_dtype), ("tight KAPPA_LN", cols, tight, derived)
    pad = (cols + 63) // 64 * 64
    assert torch.count_nonzero(got[:, cols:pad]) == 0, "pad columns must be zero"
    assert bool((got[:, pad:] == SENT).all()), "columns behind round_up(cols, 64) were written"


def out_buf(cols, dtype):
    """sentinel-filled [ROWS, round_up(cols, 64) + 64]: the kernel owns the columns up to round_up(cols, 64)"""
    return torch.full((ROWS, (cols + 63) // 64 * 64 + 64), SENT, dtype=dtype, device="cuda")


@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", gc.LN_ROWS)
@pytest.mark.parametrize("src", ["x32", "x16"])
def test_layernorm_fp32_and_mixed_kernel(ops, dtype, name, src):
    """ln_kernel<T, NV4>: fp32 or 16-bit rows in, 16-bit and fp32 rows out, with and without the additive table (3 table rows,
    row r takes r mod 3)"""
    w = [0.0, 0.0]
    for cols in COLS32:
        gamma, beta = (t.cuda() for t in gc.ln_params(cols))
        x = gc.ln_rows(name, ROWS, cols, gc.F32 if src == "x32" else dtype)
        xd = padded(ops, x)
        for with_add in (False, True):
            add = add_rows = None
            if with_add:
                g = torch.Generator().manual_seed(cols)
                add = torch.zeros(3, ops.pad64(cols), device="cuda")
                add[:, :cols] = (0.25 * torch.randn(3, cols, generator=g)).cuda()
                add_rows = add[torch.arange(ROWS, device="cuda") % 3, :cols]
            ref, T = gc.ln_reference(xd[:, :cols], gamma, beta, gc.LN_EPS, add_rows)
            y16, y32 = out_buf(cols, dtype), out_buf(cols, gc.F32)
            ops.layernorm(xd, gamma, beta, gc.LN_EPS, cols, dtype, y16=y16, y32=y32, add=add, add_period=3 if with_add else 0)
            check_ln(y16, ref, T, cols, dtype, w)
            check_ln(y32, ref, T, cols, gc.F32, w)
            if name == "constant" and not with_add:      # the reference IS beta: the metric above bounds |y - beta| by the mean's rounding
                assert bool(((ref - beta.double()[None, :]).abs() <= 1e-9).all())
    print("RATIO ln_%s %s %s %.3f %.3f" % (src, name, TN[dtype], w[0], w[1]))


def test_layernorm_refuses_4100_columns(ops):
    cols = 4100
    gamma, beta = (t.cuda() for t in gc.ln_params(cols))
    x = padded(ops, gc.ln_rows("two_level", ROWS, cols, gc.F32))
    y16 = torch.full((ROWS, ops.pad64(cols)), SENT, dtype=gc.F16, device="cuda")
    with pytest.raises(Exception):
        ops.layernorm(x, gamma, beta, gc.LN_EPS, cols, gc.F16, y16=y16)
    torch.cuda.synchronize()
    assert bool((y16 == SENT).all())


@pytest.mark.parametrize("dtype", DT, ids=["out_fp16", "out_bf16"])
@pytest.mark.parametrize("xdtype", DT, ids=["in_fp16", "in_bf16"])
@pytest.mark.parametrize("name", gc.LN_ROWS)
def test_layernorm_16bit_kernel(ops, dtype, xdtype, name):
    """ln16_kernel<TI, TO, NV8>, all four type pairs"""
    w = [0.0, 0.0]
    for cols in COLS16:
        gamma, beta = (t.cuda() for t in gc.ln_params(cols))
        xd = padded(ops, gc.ln_rows(name, ROWS, cols, xdtype))
        ref, T = gc.ln_reference(xd[:, :cols], gamma, beta)
        y16 = out_buf(cols, dtype)
        ops.layernorm(xd, gamma, beta, gc.LN_EPS, cols, dtype, y16=y16, x16_kernel=True)
        check_ln(y16, ref, T, cols, dtype, w)
    print("RATIO ln16_%s %s %s %.3f %.3f" % (TN[xdtype], name, TN[dtype], w[0], w[1]))


@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("cols", [100, 768, 772, 1024])
def test_qformer_embed_rows(ops, dtype, cols):
    """qembed_kernel<T, 2 / 12 / 16>: the query rows (16-bit) and the text rows word[id] + pos[t] (fp32 sum) are the designed rows"""
    K, F_ = len(gc.LN_ROWS), 3
    gamma, beta = (t.cuda() for t in gc.ln_params(cols))
    query = padded(ops, torch.cat([torch.stack([gc.ln_rows(n, 2, cols, dtype)[i] for n in gc.LN_ROWS]) for i in range(2)]))
    word = padded(ops, torch.cat([gc.ln_rows(n, 1, cols, gc.F32, seed=3) for n in gc.LN_ROWS]))
    g = torch.Generator().manual_seed(cols)
    pos = padded(ops, 2.0 ** -10 * torch.randn(K, cols, generator=g))
    qsrc = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    ids = torch.tensor([4, 2, 0, 1, 3], dtype=torch.int32, device="cuda")
    h32, h16 = ops.qformer_embed(query, qsrc, word, pos, ids, gamma, beta, gc.LN_EPS, F_, K, cols, dtype)
    text = word[ids.long(), :cols] + pos[:, :cols]                    # the kernel's own fp32 sum: the rows as normalised
    rows = torch.cat([torch.cat([query.view(2, K, -1)[int(q), :, :cols].float(), text]) for q in qsrc.tolist()])
    ref, T = gc.ln_reference(rows, gamma, beta)
    w = [0.0, 0.0]
    for got, odt in ((h32, gc.F32), (h16, dtype)):
        assert torch.isfinite(got.float()).all() and torch.count_nonzero(got[:, cols:]) == 0
        tight, derived = (gc.ln_ratio(got[:, :cols], ref, T, odt, k) for k in (gc.KAPPA_LN, gc.kappa_ln_derived(cols)))
        w[0], w[1] = max(w[0], tight), max(w[1], derived)
        assert derived <= gc.bound(odt) and tight <= gc.bound(odt), (odt, tight, derived)
    print("RATIO qembed all %s %.3f %.3f" % (TN[dtype], w[0], w[1]))


@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("cols", [4, 60, 64, 772])
def test_l2_normalize_rows(ops, dtype, cols):
    """x / max(||x||, 1e-12) in place over `cols` columns: |got - ref| <= 1.25 (u |ref| + (cols / 2 + 4) 2^-24 |ref| + FLOOR) - the
    fp32 sum of `cols` squares in any order errs by at most cols 2^-24 of itself, half of that on the norm; pad columns untouched"""
    w = 0.0
    for name in gc.LN_ROWS:
        x = gc.ln_rows(name, ROWS, cols, dtype)
        buf = torch.full((ROWS, ops.pad64(cols)), SENT, dtype=dtype, device="cuda")
        buf[:, :cols] = x.cuda()
        ops.l2_normalize(buf, ROWS, cols)
        xd = x.double().cuda()
        ref = xd / xd.norm(dim=1, keepdim=True).clamp_min(1e-12)
        den = gc.U[dtype] * ref.abs() + (cols / 2 + 4) * gc.U32 * ref.abs() + gc.FLOORS[dtype]
        r = torch.nan_to_num((buf[:, :cols].double() - ref).abs() / den, nan=float("inf")).max().item()
        w = max(w, r)
        assert r <= gc.BOUND16, (name, r)
        assert bool((buf[:, cols:] == SENT).all())
    print("RATIO l2_normalize all %s %.3f %.3f" % (TN[dtype], w, w))
