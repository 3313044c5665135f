"""GPU (-m gpu): the MEMORY contract of every kernel-launching entry point of include/tdc_hip.h - what a call may write and
what its result may depend on.  The value tests (test_hip_ops.py, test_hip_beats.py, ...) hand the kernels exactly-sized
tensors: a store past a ragged tile or a load of memory the contract does not give lands in some other allocator block and
nothing notices.  Here every output is the middle of a sentinel-filled arena and every input is surrounded by poison
(tests/memcheck.py); each call runs twice - surroundings all-zero bytes, then 0xFF bytes (NaN in every type of the path,
-1 as an index) - and three things are asserted:

  1. write set   the arena is byte-identical to the sentinel outside the write set the header documents;
  2. read set    the two runs' outputs are bit-identical and finite;
  3. value       the output matches the fp32 torch reference of test_hip_ops.py under that file's tolerance.

The shapes put a ragged edge on every kernel form the dispatchers can pick (thresholds read from the launch code: launch_qt
and tdc_attention32, use_256 of gemm_impl.h, the fast / element-wise choices of misc.hip).  No test accesses memory outside
an allocation it owns and none can fault: a violation is a changed sentinel or a NaN."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import memcheck as mc
from test_hip_ops import relerr, tol

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
BAND = 256                       # rows: one full tile of the largest tile any kernel here uses (256 x 256 GEMM, 256-row attention)

# the entry points of include/tdc_hip.h that launch no kernel (queries, switches, the profiler's bookkeeping)
NON_LAUNCHING = {
    "tdc_gemm_set_debug", "tdc_gemm_set_persistent_grid",                   # host-side switches
    "tdc_frame_cossim_scratch_floats", "tdc_pair_cossim_scratch_floats",    # size queries
    "tdc_fingerprint_rows_scratch_bytes", "tdc_preprocess_scratch_bytes",
    "tdc_vit_workspace_bytes", "tdc_qformer_workspace_bytes", "tdc_connector_workspace_bytes",
    "tdc_qformer_xattn_supported", "tdc_fbank_frames",                      # shape predicates
    "tdc_profile_start", "tdc_profile_stop", "tdc_profile_tag",             # event records around other calls' launches
    "tdc_version", "tdc_device_info",
}
COVERED = {}                     # entry point -> names of the tests below that run it inside guarded / poisoned memory


# how a test reaches an entry point when it does not name the symbol itself: the ops / engine call that wraps it
WRAPPERS = {"tdc_gemm": "ops.gemm(", "tdc_ln_finalize": "ops.ln_finalize(", "tdc_quantize_rows_fp8": "ops.quantize_rows_fp8(",
            "tdc_layernorm": "ops.layernorm(", "tdc_l2_normalize": "ops.l2_normalize(", "tdc_attention": "ops.attention(",
            "tdc_sva_attention": "ops.sva_attention(", "tdc_qformer_xattn": "ops.qformer_xattn", "tdc_gather_rows": "ops.gather_rows(",
            "tdc_relpos_gate": "ops.relpos_gate(", "tdc_vit_fwd": "enc.tower(", "tdc_connector_fwd": "enc.connector(",
            "tdc_qformer_fwd": "enc.encode_video("}


def covers(*names):
    def deco(fn):
        for n in names:
            COVERED.setdefault(n, []).append(fn.__name__)
        return fn
    return deco


@pytest.fixture(scope="module")
def ops():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops as o
    assert torch.cuda.is_available()
    return o


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, s=1.0):
    return torch.randn(*shape, generator=g) * s


def pin(data, fill, ld=None, band=BAND, **kw):
    """an input: `data` (host or device) surrounded by `fill` bytes; -> the device view"""
    return mc.poisoned(data.cuda(), band, band, ld=ld, fill=fill, **kw)[0]


def pout(shape, dtype, fill, ld=None, band=BAND):
    """a pure output: -> (view, arena), previous contents = `fill` as well"""
    return mc.guarded(shape, dtype, "cuda", band, band, ld=ld, fill=fill)


def two_runs(case):
    """case(fill) -> list of output tensors (it asserts its own write sets).  Runs it with zero and with 0xFF surroundings;
    -> the outputs (of the 0xFF run) after asserting that both runs agree bit for bit and are finite."""
    outs = []
    for fill in mc.PATTERNS:
        o = case(fill)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in o])
    for i, (a, b) in enumerate(zip(*outs)):
        assert mc.all_finite(b), "output %d is not finite with 0xFF surroundings" % i
        assert mc.all_finite(a), "output %d is not finite with zero surroundings" % i
        assert mc.same_bits(a, b), "output %d depends on memory outside the declared read set" % i
    return outs[1]


def rowmap(m, M):
    if m is None:
        return torch.arange(M)
    seg, stride, off, inner = m
    i = torch.arange(M)
    return (i // seg) * stride + off + (i % seg) * inner


def rowmask(rows, total):
    w = torch.zeros(total, dtype=torch.bool)
    w[rows] = True
    return w


def colmask(rows_mask, ncols, ld):
    m = torch.zeros(rows_mask.numel(), ld, dtype=torch.bool)
    m[:, :ncols] = rows_mask[:, None]
    return m


# ====================================================================================================== tdc_gemm
def _act_ref(L, lin, act):
    if act == L.ACT_GELU_ERF:
        return F.gelu(lin)
    if act == L.ACT_GELU_TANH:
        return F.gelu(lin, approximate="tanh")
    if act == L.ACT_SWIGLU:
        return F.silu(lin[:, 0::2]) * lin[:, 1::2]
    return lin


# M around the tile edges of the two kernels (128 x 128; the persistent 256 x 256 one takes a launch of >= 192 tiles of
# 256 x 256 with K >= 128: N = 2052 / 2064 are 9 column tiles, so 22 / 23 row tiles; M = 1 needs 192 column tiles).  Two classes of
# N, both with N % 64 != 0: N % 8 == 4 (68, 132, 2052, 191 * 256 + 4) - the LDS-staged 16-byte-store epilogues refuse the whole
# launch (epilogue_staged_f: (N & 7) without c_pad8) and every tile goes through the element-wise MFMA-layout epilogue - and
# N % 16 == 0 (144, 2064, 191 * 256 + 16): the staged epilogues themselves (epi_staged16, the SWIGLU one, the 16-bit read-modify-
# write one) with a ragged last column group and a ragged last row tile.  136: N % 8 == 0 but N % 16 == 8 (SWIGLU unstaged).
GEMM_SHAPES = [(1, 68, 64), (127, 68, 64), (129, 132, 128), (255, 136, 64), (257, 132, 64),
               (22 * 256 - 1, 2052, 128), (22 * 256 + 1, 2052, 128), (1, 191 * 256 + 4, 128),
               (1, 144, 64), (127, 144, 64), (129, 144, 128), (257, 144, 64),
               (22 * 256 - 1, 2064, 128), (22 * 256 + 1, 2064, 128), (1, 191 * 256 + 16, 128)]


@covers("tdc_gemm")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_plain_and_activations(ops, dtype, M, N, K):
    from tdc_video_amd import lib as L
    g = gen(M + N)
    a, w, bias = randn(g, M, K).to(dtype), randn(g, N, K, s=1 / math.sqrt(K)).to(dtype), randn(g, N)
    lin = a.cuda().float() @ w.cuda().float().t() + bias.cuda()
    acts = [L.ACT_NONE, L.ACT_GELU_ERF, L.ACT_GELU_TANH] + ([L.ACT_SWIGLU] if N % 8 == 0 else [])
    if (M > 1000 or N > 10000) and N % 8:
        acts = [L.ACT_NONE, L.ACT_GELU_TANH]
    for act in acts:
        for f32 in (False, True):
            if f32 and act != L.ACT_NONE:
                continue                                   # refused: test_gemm_refuses_an_activation_with_an_fp32_output
            n_out = N // 2 if act == L.ACT_SWIGLU else N
            ldc = ops.pad64(n_out) + 64

            def case(fill):
                A, Wt, b = pin(a, fill, ld=K + 64), pin(w, fill, ld=K + 64), pin(bias, fill)
                c, ca = pout((M, n_out), torch.float32 if f32 else dtype, fill, ld=ldc)
                ops.gemm(A, Wt, b, act=act, out=c, out_f32=f32)
                mc.assert_untouched(ca, what="C (act %d, f32 %d)" % (act, f32))
                return [c]
            out, = two_runs(case)
            assert relerr(out, _act_ref(L, lin, act)) < tol(dtype), (act, f32)


def test_gemm_refuses_an_activation_with_an_fp32_output(ops):
    """Found by this module: act != NONE with out_f32 ran the 16-bit activation epilogue on the fp32 C - 2-byte values over the
    first half of every row, the other half left as it was (with 0xFF there: NaN).  tdc_gemm now refuses the combination
    and writes nothing."""
    from tdc_video_amd import lib as L
    a, w = torch.randn(129, 64, device="cuda").half(), torch.randn(68, 64, device="cuda").half()
    c, ca = pout((129, 68), torch.float32, mc.NAN_FF, ld=128)
    d = L.GemmDesc()
    d.A, d.lda, d.W, d.ldw, d.C, d.ldc = a.data_ptr(), 64, w.data_ptr(), 64, c.data_ptr(), 128
    d.M, d.N, d.K, d.dtype, d.out_f32 = 129, 68, 64, L.F16, 1
    for act in (L.ACT_GELU_ERF, L.ACT_GELU_TANH):
        d.act = act
        assert L.load().tdc_gemm(C.byref(d), ops._stream()) == -2           # TDC_E_BADARG
        with pytest.raises(AssertionError):
            ops.gemm(a, w, act=act, out_f32=True)
    torch.cuda.synchronize()
    mc.assert_untouched(ca, torch.zeros(129, dtype=torch.bool))


@covers("tdc_gemm")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M,N,K", [(129, 132, 64), (22 * 256 + 1, 2052, 128), (127, 144, 64), (129, 144, 64), (257, 144, 128),
                                   (22 * 256 - 1, 2064, 128), (22 * 256 + 1, 2064, 128), (1, 191 * 256 + 16, 128)])
def test_gemm_residuals(ops, dtype, M, N, K):
    """fp32 and 16-bit residual, out of place and in place (C == res: the residual arena is then the guarded output)"""
    g = gen(M)
    a, w, bias = randn(g, M, K).to(dtype), randn(g, N, K, s=1 / math.sqrt(K)).to(dtype), randn(g, N)
    r32 = randn(g, M, N)
    lin = a.cuda().float() @ w.cuda().float().t() + bias.cuda()
    ld = ops.pad64(N) + 64
    for rdt in (torch.float32, dtype):
        res = r32.to(rdt)
        for inplace in (False, True):
            def case(fill):
                A, Wt, b = pin(a, fill), pin(w, fill), pin(bias, fill)
                r, ra = mc.poisoned(res.cuda(), BAND, BAND, ld=ld, fill=fill, pad="poison")
                if inplace:
                    before = ra.buf.clone()
                    ops.gemm(A, Wt, b, res=r, out=r, out_f32=rdt == torch.float32)
                    mc.assert_unchanged(ra, before, what="the residual stream updated in place")   # bands and pad columns keep their bytes
                    return [r]
                c, ca = pout((M, N), rdt, fill, ld=ld)
                ops.gemm(A, Wt, b, res=r, out=c, out_f32=rdt == torch.float32)
                mc.assert_untouched(ca)
                return [c]
            out, = two_runs(case)
            assert relerr(out, lin + res.cuda().float()) < tol(dtype), (rdt, inplace)


@covers("tdc_gemm")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("big", [False, True])
def test_gemm_row_maps_with_gaps(ops, dtype, big):
    """a_map / c_map / r_map with stride > seg and an offset: the rows no m < M maps to are poison (A, res) and guarded (C)"""
    g = gen(7)
    N, K = (2052, 128) if big else (68, 64)
    M = 22 * 256 + 77 if big else 150
    am, cm, rm = (144, 156, 5, 1), (144, 150, 3, 1), (144, 145, 1, 1)
    ar, cr, rr = rowmap(am, M), rowmap(cm, M), rowmap(rm, M)
    a, w, bias = randn(g, M, K).to(dtype), randn(g, N, K, s=1 / math.sqrt(K)).to(dtype), randn(g, N)
    res = randn(g, M, N)
    ldc = ops.pad64(N) + 64
    rows_c = int(cr.max()) + 7

    def case(fill):
        A = pin(a, fill, rows=ar, total_rows=int(ar.max()) + 9)
        R = pin(res, fill, rows=rr, total_rows=int(rr.max()) + 9)
        Wt, b = pin(w, fill), pin(bias, fill)
        c, ca = pout((rows_c, N), torch.float32, fill, ld=ldc)
        ops.gemm(A, Wt, b, res=R, out=c, out_f32=True, M=M, a_map=am, c_map=cm, r_map=rm)
        mc.assert_untouched(ca, rowmask(cr, rows_c))
        return [c[cr.cuda()]]
    out, = two_runs(case)
    ref = a.cuda().float() @ w.cuda().float().t() + bias.cuda() + res.cuda()
    assert relerr(out, ref) < tol(dtype)


@covers("tdc_gemm", "tdc_ln_finalize")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M", [129, 55 * 256 + 1])       # 128 x 128; persistent (N = 256: one column tile x 56 row tiles x ... see below)
def test_gemm_layernorm_fusion_producers_and_consumer(ops, dtype, M):
    """LayerNorm-fusion producer over the fp32 stream (x16 + ln_part) and over a 16-bit stream (ln_part only), tdc_ln_finalize,
    and the consumer (ln_stats / ln_c1)"""
    from tdc_video_amd import lib as L
    g = gen(M)
    D, K, N2, eps = (1024, 128, 1040, 1e-6) if M > 1000 else (128, 64, 72, 1e-6)     # 56 x 4 = 224 tiles of 256 x 256
    a, w, b = randn(g, M, K).to(dtype), randn(g, D, K, s=1 / math.sqrt(K)).to(dtype), randn(g, D)
    x0 = randn(g, M, D, s=2) + 0.7
    slots = D // 64

    def producer32(fill):
        A, Wt, bb = pin(a, fill), pin(w, fill), pin(b, fill)
        x, xa = mc.poisoned(x0.cuda(), BAND, BAND, fill=fill)
        x16, x16a = pout((M, D), dtype, fill, ld=D + 64)
        part, pa = pout((slots, M, 2), torch.float32, fill, band=2)
        ops.gemm(A, Wt, bb, res=x, out=x, out_f32=True, x16=x16, ln_part=part)
        st, sa = pout((M, 2), torch.float32, fill)
        ops.ln_finalize(part, slots, M, eps, stats=st)
        for ar, nm in ((xa, "x"), (x16a, "x16"), (pa, "ln_part"), (sa, "stats")):
            mc.assert_untouched(ar, what=nm)
        return [x, x16, part, st]
    x, x16, part, stats = two_runs(producer32)
    ref = a.cuda().float() @ w.cuda().float().t() + b.cuda() + x0.cuda()
    assert relerr(x, ref) < tol(dtype) and torch.equal(x16, x.to(dtype))
    mean, rstd = x.mean(1), (x.var(1, unbiased=False) + eps).rsqrt()
    assert (stats[:, 0] - mean).abs().max().item() < 1e-5 * x.abs().max().item()
    assert ((stats[:, 1] - rstd).abs() / rstd).max().item() < 1e-5

    x0h = x0.to(dtype)

    def producer16(fill):
        A, Wt, bb = pin(a, fill), pin(w, fill), pin(b, fill)
        xs, xsa = mc.poisoned(x0h.cuda(), BAND, BAND, fill=fill)
        part, pa = pout((slots, M, 2), torch.float32, fill, band=2)
        ops.gemm(A, Wt, bb, res=xs, out=xs, ln_part=part)
        mc.assert_untouched(xsa, what="stream")
        mc.assert_untouched(pa, what="ln_part")
        return [xs, part]
    xs, part16 = two_runs(producer16)
    s32 = a.cuda().float() @ w.cuda().float().t() + b.cuda() + x0h.cuda().float()
    assert relerr(xs, s32) < tol(dtype)

    gamma, beta = 1.0 + 0.1 * randn(g, D), 0.1 * randn(g, D)
    w2, b2 = randn(g, N2, D, s=1 / math.sqrt(D)), randn(g, N2)
    wf = (w2 * gamma[None, :]).to(dtype)
    c1, c2 = wf.float().sum(1).contiguous(), (w2 @ beta + b2).contiguous()
    lin = F.layer_norm(x, (D,), gamma.cuda(), beta.cuda(), eps) @ w2.cuda().t() + b2.cuda()
    x16h, sth = x16.cpu(), stats.cpu()
    for act in (L.ACT_NONE, L.ACT_GELU_TANH, L.ACT_SWIGLU):
        n_out = N2 // 2 if act == L.ACT_SWIGLU else N2

        def consumer(fill):
            X, Wf = pin(x16h, fill, ld=D + 64), pin(wf, fill)
            st, cc1, cc2 = pin(sth, fill), pin(c1, fill), pin(c2, fill)
            c, ca = pout((M, n_out), dtype, fill, ld=ops.pad64(n_out) + 64)
            ops.gemm(X, Wf, cc2, act=act, out=c, ln_stats=st, ln_c1=cc1)
            mc.assert_untouched(ca)
            return [c]
        out, = two_runs(consumer)
        assert relerr(out, _act_ref(L, lin, act)) < 2 * tol(dtype), act


@covers("tdc_gemm", "tdc_quantize_rows_fp8")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M", [129, 50 * 256 + 1])       # 128 x 128; persistent (5 column tiles x 51 row tiles)
def test_gemm_fp8_operands_and_fp8_output(ops, dtype, M):
    """in_fp8 (A from tdc_quantize_rows_fp8 into a guarded e4m3 matrix) and out_fp8 (C and out_stats guarded)"""
    from tdc_video_amd import lib as L
    g = gen(M + 1)
    K, N, ws2 = 256, 1216, 0.37
    x = (randn(g, M, K) * (0.5 + torch.rand(M, 1, generator=g))).to(dtype)
    w = randn(g, N, K, s=1 / math.sqrt(K))
    b = randn(g, N)
    sw = (w.abs().max() / 448.0).item()
    w8 = (w / sw).to(torch.float8_e4m3fn).view(torch.uint8)

    def quant(fill):
        X = pin(x, fill, ld=K + 64)
        y8, ya = pout((M, K), torch.uint8, fill, ld=K + 128)
        st, sa = pout((M, 2), torch.float32, fill)
        ops.quantize_rows_fp8(X, K, sw, y8=y8, stats=st)
        mc.assert_untouched(ya, what="y8")            # K % 128 == 0: no pad bytes to zero
        mc.assert_untouched(sa, what="stats")
        return [y8, st]
    x8, st = two_runs(quant)
    sa_ref = x.cuda().float().abs().amax(1) / 448.0
    assert ((st[:, 1] / sw - sa_ref).abs() / sa_ref).max().item() < 1e-6 and torch.count_nonzero(st[:, 0]) == 0
    want = (x.cuda().float() / sa_ref[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert (want != x8).float().mean().item() < 1e-3
    x8f = x8.view(torch.float8_e4m3fn).float()
    lin = (x8f * sa_ref[:, None]) @ (w8.cuda().view(torch.float8_e4m3fn).float() * sw).t() + b.cuda()
    x8h, sth = x8.cpu(), st.cpu()
    c1 = torch.zeros(N)
    for act in (L.ACT_NONE, L.ACT_SWIGLU):
        n_out = N // 2 if act == L.ACT_SWIGLU else N

        def case(fill):
            A, Wt = pin(x8h, fill, ld=K + 128), pin(w8, fill, ld=K + 128)
            c, ca = pout((M, n_out), dtype, fill, ld=ops.pad64(n_out) + 64)
            ops.gemm(A, Wt, pin(b, fill), act=act, out=c, ln_stats=pin(sth, fill), ln_c1=pin(c1, fill), out_dtype=dtype)
            mc.assert_untouched(ca)
            return [c]
        out, = two_runs(case)
        assert relerr(out, _act_ref(L, lin, act)) < tol(dtype), act
    # e4m3 output with analytic row scales: C bytes [M, n_out] and out_stats [M, 2], nothing else
    norm = x8f.norm(dim=1) * 1.01
    stats2 = torch.stack([norm, sa_ref * sw], 1).contiguous().cpu()
    w2max, bmax = w8.view(torch.float8_e4m3fn).float().norm(dim=1).max().item(), b.abs().max().item()
    bound = (sa_ref * sw * norm * w2max + bmax)

    def case8(fill):
        A, Wt = pin(x8h, fill, ld=K + 128), pin(w8, fill, ld=K + 128)
        c, ca = pout((M, N), torch.uint8, fill, ld=N + 128)
        os_, oa = pout((M, 2), torch.float32, fill)
        ops.gemm(A, Wt, pin(b, fill), out=c, ln_stats=pin(stats2, fill), ln_c1=pin(c1, fill), out_dtype=dtype, out_stats=os_,
                 out_w2max=w2max, out_bmax=bmax, out_wscale=ws2)
        mc.assert_untouched(ca, what="C (e4m3)")
        mc.assert_untouched(oa, what="out_stats")
        return [c, os_]
    c8, os_ = two_runs(case8)
    sh = bound / 448.0
    assert torch.count_nonzero(os_[:, 0]) == 0 and ((os_[:, 1] / ws2 - sh).abs() / sh).max().item() < 1e-5
    o = c8.contiguous().view(torch.float8_e4m3fn).float()
    assert relerr(o * sh[:, None], lin) < 0.07          # test_gemm_fp8_output's bound: half an e4m3 ulp on the largest element


@covers("tdc_gemm")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M,N", [(768, 5 * 156), (768, 37 * 156), (200, 7 * 20), (768, 64 * 256 + 4), (4607, 11 * 256 + 4)])
def test_gemm_c_pad8_transposed_values(ops, dtype, M, N):
    """c_pad8: columns N .. round_up(N, 8) of C may be written (unspecified values), round_up(N, 8) .. ldc may not; rows past M
    never.  N % 8 == 4 in every case.  The first three shapes run on the 128 x 128 kernel; (768, 64 * 256 + 4) - 3 x 65 = 195
    tiles, the shape class of the Q-Former's transposed value projection (M = dim, N = frames x tokens) - and (4607, 11 * 256 + 4)
    - 18 x 12 = 216 tiles, ragged in M as well - on the persistent one, whose staged epilogue makes the overhanging 16-byte store."""
    g = gen(N)
    K = 128
    assert N % 8 == 4
    a, w = randn(g, M, K, s=0.08).to(dtype), randn(g, N, K).to(dtype)
    ldc = ops.pad64(N) + 64
    n8 = (N + 7) // 8 * 8

    def case(fill):
        c, ca = pout((M, N), dtype, fill, ld=ldc)
        ops.gemm(pin(a, fill), pin(w, fill), out=ca.full[:, :n8], c_pad8=True)
        m = torch.zeros(M, ldc, dtype=torch.bool)
        m[:, :n8] = True
        mc.assert_untouched(ca, m)
        return [c]
    out, = two_runs(case)
    assert relerr(out, a.cuda().float() @ w.cuda().float().t()) < tol(dtype)


@covers("tdc_gemm")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N", [2052, 2064])               # element-wise epilogue / the staged 16-bit read-modify-write one
@pytest.mark.parametrize("M", [127, 129, 22 * 256 - 1, 22 * 256 + 1])
def test_gemm_c16_dtype_other_type_residual_stream(ops, dtype, M, N):
    """c16_dtype_p1: C and the 16-bit residual of the OTHER 16-bit type, out of place and in place (the towers' fp16 residual
    stream under bf16 operands is updated in place)"""
    cdt = torch.bfloat16 if dtype == torch.float16 else torch.float16
    g = gen(M + 3)
    K = 128
    a, w, bias = randn(g, M, K).to(dtype), randn(g, N, K, s=1 / math.sqrt(K)).to(dtype), randn(g, N)
    res = randn(g, M, N, s=3).to(cdt)

    def case(fill):
        r = pin(res, fill, ld=ops.pad64(N))
        c, ca = pout((M, N), cdt, fill, ld=ops.pad64(N) + 64)
        ops.gemm(pin(a, fill), pin(w, fill), pin(bias, fill), res=r, out=c)
        mc.assert_untouched(ca)
        return [c]
    out, = two_runs(case)
    ref = a.cuda().float() @ w.cuda().float().t() + bias.cuda() + res.cuda().float()
    ulp = 2.0 ** -10 if cdt == torch.float16 else 2.0 ** -7
    assert ((out.float() - ref).abs() / ref.abs().clamp_min(1.0)).max().item() < 1.1 * ulp

    def inplace(fill):
        r, ra = mc.poisoned(res.cuda(), BAND, BAND, ld=ops.pad64(N) + 64, fill=fill, pad="poison")
        before = ra.buf.clone()
        ops.gemm(pin(a, fill), pin(w, fill), pin(bias, fill), res=r, out=r)
        mc.assert_unchanged(ra, before, what="the other-type residual stream updated in place")
        return [r]
    out2, = two_runs(inplace)
    assert torch.equal(out2, out)


# ====================================================================================================== LayerNorm family
@covers("tdc_quantize_rows_fp8")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("cols", [48, 72, 1152, 3584])
def test_quantize_rows_fp8(ops, dtype, cols, wide):
    """the header's two branches: y8[r, 0 .. round_up(cols, 128)) (zero bytes from `cols` on) when ldy8 >= round_up(cols, 128)
    (wide), y8[r, 0 .. cols) otherwise; stats[r][0 .. 2); x rows past `rows` and y8 / stats' previous contents are poison"""
    g = gen(cols + wide)
    rows, ws = 37, 0.25
    p128 = (cols + 127) // 128 * 128
    ldy = p128 + 64 if wide else cols + 8
    wcols = p128 if ldy >= p128 else cols
    x = (randn(g, rows, cols) * torch.rand(rows, 1, generator=g) * 5).to(dtype)

    def case(fill):
        y8, ya = pout((rows, cols), torch.uint8, fill, ld=ldy)
        st, sa = pout((rows, 2), torch.float32, fill)
        ops.quantize_rows_fp8(pin(x, fill, ld=ops.pad64(cols) + 64), cols, ws, y8=y8, stats=st)
        mc.assert_untouched(ya, colmask(torch.ones(rows, dtype=torch.bool), wcols, ldy), "y8")
        mc.assert_untouched(sa, what="stats")
        return [ya.full[:, :wcols], st]
    y8, st = two_runs(case)
    sa_ref = x.cuda().float().abs().amax(1) / 448.0
    assert ((st[:, 1] / ws - sa_ref).abs() / sa_ref).max().item() < 1e-6 and torch.count_nonzero(st[:, 0]) == 0
    want = (x.cuda().float() / sa_ref[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert (want != y8[:, :cols]).float().mean().item() < 1e-3 and torch.count_nonzero(y8[:, cols:]) == 0


@covers("tdc_layernorm")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cols", [48, 72, 1152, 3584])
def test_layernorm(ops, dtype, cols):
    """y16 / y32: columns 0 .. round_up(cols, 64) are written (the pad ones with zeros) when ld allows, nothing beyond; row
    maps with gaps; y32 aliasing x; the 16-bit-to-16-bit kernel (x_dtype_p1); the e4m3 output with its stats"""
    g = gen(cols)
    rows, p64 = 37, ops.pad64(cols)
    ld = p64 + 64
    x = randn(g, rows, cols, s=3) + 1
    gamma, beta = randn(g, cols), randn(g, cols)
    ref = F.layer_norm(x.cuda(), (cols,), gamma.cuda(), beta.cuda(), 1e-6)
    xm, ym = (5, 9, 2, 1), (5, 7, 1, 1)
    xr, yr = rowmap(xm, rows), rowmap(ym, rows)
    ytot = int(yr.max()) + 5

    def case(fill):
        X = pin(x, fill, ld=ld, rows=xr, total_rows=int(xr.max()) + 4)
        y16, a16 = pout((ytot, cols), dtype, fill, ld=ld)
        y32, a32 = pout((ytot, cols), torch.float32, fill, ld=ld)
        ops.layernorm(X, pin(gamma, fill), pin(beta, fill), 1e-6, cols, dtype, y16=y16, y32=y32, rows=rows, x_map=xm, y_map=ym)
        w = colmask(rowmask(yr, ytot), p64, ld)
        mc.assert_untouched(a16, w, "y16")
        mc.assert_untouched(a32, w, "y32")
        return [a16.full[yr.cuda(), :p64], a32.full[yr.cuda(), :p64]]
    y16, y32 = two_runs(case)
    assert (y32[:, :cols] - ref).abs().max().item() < 2e-5 and relerr(y16[:, :cols], ref) < tol(dtype)
    assert torch.count_nonzero(y16[:, cols:]) == 0 and torch.count_nonzero(y32[:, cols:]) == 0

    def alias(fill):                                  # y32 aliases x: the stream is normalised in place
        X, xa = mc.poisoned(x.cuda(), BAND, BAND, ld=ld, fill=fill)
        before = xa.buf.clone()
        ops.layernorm(X, pin(gamma, fill), pin(beta, fill), 1e-6, cols, dtype, y32=X, want16=False)
        mc.assert_unchanged(xa, before, colmask(torch.ones(rows, dtype=torch.bool), p64, ld), "x normalised in place")
        return [X]
    z, = two_runs(alias)
    assert (z - ref).abs().max().item() < 2e-5

    if cols % 8 == 0:
        for xdt in DT:
            x16 = x.to(xdt)
            r16 = F.layer_norm(x16.cuda().float(), (cols,), gamma.cuda(), beta.cuda(), 1e-6)

            def case16(fill):
                y, ya = pout((rows, cols), dtype, fill, ld=ld)
                ops.layernorm(pin(x16, fill, ld=ld), pin(gamma, fill), pin(beta, fill), 1e-6, cols, dtype, y16=y, x16_kernel=True)
                mc.assert_untouched(ya, colmask(torch.ones(rows, dtype=torch.bool), p64, ld))
                return [ya.full[:, :p64]]
            y, = two_runs(case16)
            assert relerr(y[:, :cols], r16) < tol(dtype) and torch.count_nonzero(y[:, cols:]) == 0

    def case8(fill):
        y8, ya = pout((rows, cols), torch.uint8, fill, ld=ld)
        st, sa = pout((rows, 2), torch.float32, fill)
        ops.layernorm(pin(x, fill, ld=ld), pin(gamma, fill), pin(beta, fill), 1e-6, cols, torch.bfloat16, y8=y8, y8_stats=st,
                      y8_wscale=0.5)
        mc.assert_untouched(ya, colmask(torch.ones(rows, dtype=torch.bool), p64, ld), "y8")
        mc.assert_untouched(sa, what="y8_stats")
        return [ya.full[:, :p64], st]
    y8, st = two_runs(case8)
    sc = ref.abs().amax(1) / 448.0
    assert ((st[:, 1] / 0.5 - sc).abs() / sc).max().item() < 1e-5 and torch.count_nonzero(y8[:, cols:]) == 0
    deq = y8[:, :cols].contiguous().view(torch.float8_e4m3fn).float() * sc[:, None]
    assert relerr(deq, ref) < 2 ** -4                 # test_layernorm_fp8_output's bound


@covers("tdc_l2_normalize", "tdc_qformer_embed")
@pytest.mark.parametrize("dtype", DT)
def test_l2_normalize_and_qformer_embed(ops, dtype):
    g = gen(11)
    rows, cols, ld = 61, 72, 192
    x = randn(g, rows, cols).to(dtype)

    def case(fill):
        X, xa = mc.poisoned(x.cuda(), BAND, BAND, ld=ld, fill=fill, pad="poison")
        before = xa.buf.clone()
        ops.l2_normalize(X, rows, cols)
        mc.assert_unchanged(xa, before, what="x")               # [rows, cols] only: the pad columns are neither read nor written
        return [X]
    z, = two_runs(case)
    assert relerr(z, F.normalize(x.cuda().float(), dim=-1)) < tol(dtype)

    for D, K, ids_l in ((768, 16, [3, 7, 7, 49, 0]), (72, 16, []), (768, 144, [5])):
        Fr, nchunk, Lt = 5, 2, len(ids_l)
        ld = ops.pad64(D)
        query = randn(g, nchunk * K, D).to(dtype)
        qsrc = torch.tensor([0, 0, 1, 1, 0], dtype=torch.int32)
        word, pos = randn(g, 50, D), randn(g, 32, D)
        ids = torch.tensor(ids_l, dtype=torch.int32) if Lt else None
        gamma, beta = randn(g, D), randn(g, D)
        S = K + Lt

        def qe(fill):
            from tdc_video_amd import lib as L
            d = L.QEmbedDesc()
            q_ = pin(query, fill, ld=ld + 64)
            keepalive = [q_, pin(qsrc, fill), pin(gamma, fill), pin(beta, fill)]
            d.query, d.ldq, d.qsrc = q_.data_ptr(), q_.stride(0), keepalive[1].data_ptr()
            if Lt:
                # `word` rows that `ids` never names are poison
                named = sorted(set(ids_l))
                wv = pin(word[named], fill, ld=ld, rows=named, total_rows=50)
                pv = pin(pos[:Lt], fill, ld=ld)
                iv = pin(ids, fill)
                keepalive += [wv, pv, iv]
                d.word, d.pos, d.ldw, d.ids = wv.data_ptr(), pv.data_ptr(), ld, iv.data_ptr()
            d.Lt = Lt
            d.gamma, d.beta, d.eps = keepalive[2].data_ptr(), keepalive[3].data_ptr(), 1e-12
            h32, a32 = pout((Fr * S, D), torch.float32, fill, ld=ld)
            h16, a16 = pout((Fr * S, D), dtype, fill, ld=ld)
            d.h32, d.h16, d.ld = h32.data_ptr(), h16.data_ptr(), ld
            d.F, d.K, d.cols, d.dtype = Fr, K, D, ops._dtcode(dtype)
            L.check(L.load().tdc_qformer_embed(C.byref(d), ops._stream()), "tdc_qformer_embed")
            torch.cuda.synchronize()
            full = torch.ones(Fr * S, ld, dtype=torch.bool)          # every column up to ld is written (the pad ones with zeros)
            mc.assert_untouched(a32, full, "h32")
            mc.assert_untouched(a16, full, "h16")
            return [a32.full, a16.full]
        h32, h16 = two_runs(qe)
        rows_ = query.view(nchunk, K, D)[qsrc.long()].float()
        if Lt:
            te = word[ids.long()] + pos[:Lt]
            rows_ = torch.cat([rows_, te[None].expand(Fr, -1, -1)], 1)
        ref = F.layer_norm(rows_, (D,), gamma, beta, 1e-12).reshape(-1, D).cuda()
        assert (h32[:, :D] - ref).abs().max().item() < 1e-4 and relerr(h16[:, :D], ref) < tol(dtype)
        assert torch.count_nonzero(h32[:, D:]) == 0 and torch.count_nonzero(h16[:, D:]) == 0


# ====================================================================================================== tdc_attention
def _attn_ref(q, k, v, scale, add=None):
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    if add is not None:
        s = s + add
    return torch.softmax(s, -1) @ v.float()


# (head_dim, sq, sk, form): QT = 1 (sq <= 64), QT = 2, QT = 3 (d = 64, 129 .. 192), QT = 4 (d = 64, sq > 256: form 1 keeps the
# 16x16x32 kernels where AUTO would take the 32x32x16 form), and the 32x32x16 form itself (AUTO, sq >= 256, sk >= 64, d 64 / 72)
ATTN_CASES = [(64, 1, 1, 0), (64, 63, 63, 0), (64, 64, 65, 0), (12, 1, 1, 0), (12, 63, 4, 0), (16, 64, 63, 0),
              (64, 65, 4, 0), (64, 128, 127, 0), (72, 65, 63, 0), (80, 127, 64, 0), (12, 65, 65, 0), (16, 300, 129, 0),
              (72, 300, 64, 1), (80, 257, 1, 0),
              (64, 129, 1, 0), (64, 191, 63, 0), (64, 192, 128, 0), (64, 130, 4, 0),
              (64, 257, 65, 1), (64, 511, 127, 1), (64, 258, 4, 1), (64, 257, 1, 1),
              (64, 256, 64, 0), (64, 257, 65, 0), (72, 300, 127, 0), (72, 511, 68, 0), (64, 255, 64, 0), (64, 256, 63, 0)]


@covers("tdc_attention")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("d,sq,sk,form", ATTN_CASES)
def test_attention(ops, dtype, d, sq, sk, form):
    """fused-QKV strides when sq == sk (one buffer, three column views), separate q and k|v buffers otherwise; o: only the
    heads * head_dim columns of the sq rows of every batch item are written"""
    g = gen(d * 1000 + sq + sk)
    B, H = 2, 2
    D = H * d
    scale = 1.0 / math.sqrt(d)
    ldo = ops.pad64(D) + 64
    if sq == sk:
        qkv = randn(g, B * sq, 3 * D).to(dtype)
        qh, kh, vh = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        qh = randn(g, B * sq, D).to(dtype)
        kv = randn(g, B * sk, 2 * D).to(dtype)
        kh, vh = kv[:, :D], kv[:, D:]

    def case(fill):
        if sq == sk:
            buf = pin(qkv, fill, ld=ops.pad64(3 * D))
            q, k, v = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:3 * D]
        else:
            q = pin(qh.contiguous(), fill, ld=ops.pad64(D))
            kvb = pin(kv, fill, ld=ops.pad64(2 * D))
            k, v = kvb[:, :D], kvb[:, D:2 * D]
        o, oa = pout((B * sq, D), dtype, fill, ld=ldo)
        ops.attention(q, k, v, o, B, H, d, sq, sk, scale, sq * q.stride(0), sk * k.stride(0), sk * v.stride(0), sq * ldo, form=form)
        mc.assert_untouched(oa)
        return [o]
    out, = two_runs(case)
    r = lambda t, s: t.cuda().reshape(B, s, H, d).transpose(1, 2)
    ref = _attn_ref(r(qh, sq), r(kh, sk), r(vh, sk), scale).transpose(1, 2).reshape(B * sq, D)
    assert relerr(out, ref) < 2 * tol(dtype)


@covers("tdc_attention")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d,sq,sk", [(16, 1, 4), (16, 65, 68), (64, 63, 64), (64, 130, 132), (32, 64, 8)])
def test_attention_biased_form(ops, dtype, d, sq, sk, masked):
    """the gated relative position bias with and without key_mask: bias / gate / key_mask past their extent are poison"""
    g = gen(d + sq + sk)
    B, H = 2, 3
    D = H * d
    scale = 1.0 / math.sqrt(d)
    ldo = ops.pad64(D) + 64
    q_ = randn(g, B * sq, D).to(dtype)
    kv_ = randn(g, B * sk, 2 * D).to(dtype)
    bias = randn(g, H, sq, sk)
    gate = torch.rand(B * sq, H, generator=g) * 2
    km = torch.rand(B, sk, generator=g) > 0.7
    km[:, 0] = False

    def case(fill):
        q = pin(q_, fill, ld=ops.pad64(D))
        kvb = pin(kv_, fill, ld=ops.pad64(2 * D))
        k, v = kvb[:, :D], kvb[:, D:2 * D]
        o, oa = pout((B * sq, D), dtype, fill, ld=ldo)
        bz = pin(bias.reshape(H * sq, sk), fill).view(H, sq, sk)
        gt = pin(gate, fill, ld=8, pad="poison")
        mk = pin(km.to(torch.uint8), fill) if masked else None
        ops.attention(q, k, v, o, B, H, d, sq, sk, scale, sq * q.stride(0), sk * k.stride(0), sk * v.stride(0), sq * ldo,
                      bias=bz, gate=gt, key_mask=mk)
        mc.assert_untouched(oa)
        return [o]
    out, = two_runs(case)
    r = lambda t, s: t.cuda().reshape(B, s, H, d).transpose(1, 2)
    add = gate.cuda().view(B, sq, H).permute(0, 2, 1)[..., None] * bias.cuda()[None]
    sc = (r(q_, sq).float() @ r(kv_[:, :D], sk).float().transpose(-1, -2)) * scale
    if masked:
        sc = sc.masked_fill(km.cuda()[:, None, None, :], float("-inf"))
    ref = (torch.softmax(sc + add, -1) @ r(kv_[:, D:], sk).float()).transpose(1, 2).reshape(B * sq, D)
    assert relerr(out, ref) < 2 * tol(dtype)


@covers("tdc_sva_attention")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dim,heads,towers", [(64, 16, 2), (1024, 16, 2), (512, 8, 2), (256, 16, 1), (1024, 16, 1), (1032, 3, 2)])
def test_sva_attention(ops, dtype, dim, heads, towers):
    """both kernels (element-wise: head dim 4 / 344; 16-byte: the others), 18 queries = a partly filled last workgroup at
    2 / 4 / 8 queries per workgroup, one and two towers.  out: columns 0 .. dim of the T*side*side query rows, no pad column"""
    g = gen(dim + heads)
    T, side, r = 2, 3, 2
    n, nq, nkv = side * r, T * side * side, towers * r * r
    q = randn(g, nq, dim).to(dtype)
    kv = [randn(g, T * n * n, 2 * dim).to(dtype) for _ in range(towers)]
    mask = torch.rand(nq, nkv, generator=g) > 0.3
    mask[:, 0] = True
    ld = ops.pad64(dim) + 64

    def case(fill):
        o, oa = pout((nq, dim), dtype, fill, ld=ld)
        ops.sva_attention(pin(q, fill, ld=ld), [pin(t, fill, ld=2 * dim + 64) for t in kv], pin(mask.to(torch.uint8), fill).contiguous(),
                          T, side, r, dim, heads, out=o)
        mc.assert_untouched(oa)
        return [o]
    hd_, lph = dim // heads, (dim // heads) // 8
    if hd_ % 8 == 0 and lph & (lph - 1) == 0:
        out, = two_runs(case)
    else:
        # the element-wise kernel reduces its scores through LDS atomics in an arbitrary order (test_hip_ops.test_sva_attention):
        # two launches on the SAME memory differ in the last bit, so only write set, finiteness and value are pinned for it
        outs = [case(fill)[0].clone() for fill in mc.PATTERNS]
        assert all(mc.all_finite(o) for o in outs) and relerr(outs[0], outs[1]) < 2 * tol(dtype)
        out = outs[1]

    def win(x):
        return x.view(T, side, r, side, r, -1).permute(0, 1, 3, 2, 4, 5).reshape(nq, r * r, -1)
    Kk = torch.cat([win(t[:, :dim].float()) for t in kv], 1).cuda()
    V = torch.cat([win(t[:, dim:].float()) for t in kv], 1).cuda()
    hd = dim // heads
    s = (q.cuda().float().view(nq, heads, 1, hd) @ Kk.view(nq, nkv, heads, hd).transpose(1, 2).transpose(-1, -2)) / math.sqrt(hd)
    s = s.masked_fill(~mask.cuda()[:, None, None, :], float("-inf"))
    ref = (torch.softmax(s, -1) @ V.view(nq, nkv, heads, hd).transpose(1, 2)).reshape(nq, dim)
    assert relerr(out, ref) < 2 * tol(dtype)


# ====================================================================================================== Q-Former cross-attention
@covers("tdc_qformer_xattn", "tdc_qformer_xattn_tile_weight")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Fr,K,Lt,Nenc", [(5, 144, 12, 156), (37, 16, 0, 8), (3, 144, 0, 220), (3, 16, 5, 20), (2, 16, 3, 224),
                                          (1, 16, 0, 156)])
def test_qformer_xattn(ops, dtype, Fr, K, Lt, Nenc):
    """the fused block: h16 / h32 are updated in place on the K query rows of every frame - the text rows, the bands and
    nothing else keep their bytes; k past F*Nenc rows and vt past F*Nenc columns (up to ldvt) are poison - with
    Nenc % 8 == 4 (20, 156, 220) the last frame's half-valid key group reads exactly those 4 columns"""
    D, heads, Hh = 768, 12, 256
    S = K + Lt
    g = gen(Fr * 1000 + K + Nenc)
    h16_0 = randn(g, Fr * S, D).to(dtype)
    h32_0 = h16_0.float()
    wq, wo = randn(g, D, D, s=0.05).to(dtype), randn(g, D, D, s=0.05).to(dtype)
    bq, bo, bv = randn(g, D, s=0.1), randn(g, D, s=0.1), randn(g, D, s=0.1)
    ln_g, ln_b = 1 + 0.1 * randn(g, D), 0.1 * randn(g, D)
    enc = randn(g, Fr * Nenc, Hh).to(dtype)
    wk, wv = randn(g, D, Hh, s=0.08).to(dtype), randn(g, D, Hh, s=0.08).to(dtype)
    bk = randn(g, D, s=0.1)
    kmat = ops.gemm(enc.cuda(), wk.cuda(), bk.cuda()).cpu()
    n8 = (Fr * Nenc + 7) // 8 * 8
    vt_full = torch.empty(D, n8, device="cuda", dtype=dtype)
    ops.gemm(wv.cuda(), enc.cuda(), out=vt_full, c_pad8=True)
    vt0 = vt_full[:, :Fr * Nenc].contiguous().cpu()
    ldvt = n8 if n8 != Fr * Nenc else n8 + 8
    qrows = (torch.arange(Fr)[:, None] * S + torch.arange(K)[None, :]).reshape(-1)

    def tile(fill, w):
        t, ta = pout((D * D,), dtype, fill)
        from tdc_video_amd import lib as L
        W = pin(w, fill, ld=D + 64)
        L.check(L.load().tdc_qformer_xattn_tile_weight(ops._ptr(W), W.stride(0), ops._ptr(t), ops._dt(W), ops._stream()), "tile_weight")
        torch.cuda.synchronize()
        mc.assert_untouched(ta, what="tiled weight")
        return t

    def case(fill):
        h16, a16 = mc.poisoned(h16_0.cuda(), BAND, BAND, ld=D + 64, fill=fill, pad="poison")
        h32, a32 = mc.poisoned(h32_0.cuda(), BAND, BAND, ld=D + 64, fill=fill, pad="poison")
        before16, before32 = a16.buf.clone(), a32.buf.clone()
        wq_t, wo_t = tile(fill, wq), tile(fill, wo)
        k = pin(kmat, fill, ld=D + 64, pad="poison")
        vt = pin(vt0, fill, ld=ldvt, pad="poison")
        ops.qformer_xattn(h16, h32, Fr, K, S, wq_t, pin(bq, fill), wo_t, pin(bo, fill), k, vt, pin(bv, fill), Nenc, pin(ln_g, fill),
                          pin(ln_b, fill), 1e-12, D, heads, 0.125)
        torch.cuda.synchronize()
        mc.assert_unchanged(a16, before16, rowmask(qrows, Fr * S), "h16")
        mc.assert_unchanged(a32, before32, rowmask(qrows, Fr * S), "h32")
        return [h16[qrows.cuda()], h32[qrows.cuda()], wq_t]
    o16, o32, wq_t = two_runs(case)
    assert mc.same_bits(wq_t, ops.xattn_tile_weight(wq.cuda()))
    x = h16_0.cuda()[qrows.cuda()].float()
    q = (x @ wq.cuda().float().t() + bq.cuda()).to(dtype).float().view(Fr, K, heads, 64).transpose(1, 2)
    kk = kmat.cuda().float().view(Fr, Nenc, heads, 64).transpose(1, 2)
    vv = vt0.cuda().float().t().reshape(Fr, Nenc, heads, 64).transpose(1, 2)
    p = torch.softmax(q @ kk.transpose(-1, -2) * 0.125, dim=-1)
    ctx = ((p @ vv).transpose(1, 2).reshape(Fr * K, D) + bv.cuda()).to(dtype).float()
    y = F.layer_norm(ctx @ wo.cuda().float().t() + bo.cuda() + h32_0.cuda()[qrows.cuda()], (D,), ln_g.cuda(), ln_b.cuda(), 1e-12)
    assert (o32 - y).abs().max().item() < (6e-3 if dtype == torch.float16 else 4e-2)      # test_qformer_xattn_fused_block's bound
    assert torch.equal(o16, o32.to(dtype))


@covers("tdc_qformer_xattn")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("res16", [False, True])
@pytest.mark.parametrize("Fr,K,Lt", [(5, 144, 12), (9, 16, 0), (3, 16, 7)])
def test_qformer_xattn_output_projection_form(ops, dtype, res16, Fr, K, Lt):
    """the ctx form (and res16: h32 absent): ctx rows past F*K are poison; h16 (/ h32) change on the query rows only"""
    D, heads = 768, 12
    S = K + Lt
    g = gen(Fr + K + Lt)
    h16_0 = randn(g, Fr * S, D).to(dtype)
    ctx0 = randn(g, Fr * K, D).to(dtype)
    wo = randn(g, D, D, s=0.05).to(dtype)
    bo, ln_g, ln_b = randn(g, D, s=0.1), 1 + 0.1 * randn(g, D), 0.1 * randn(g, D)
    qrows = (torch.arange(Fr)[:, None] * S + torch.arange(K)[None, :]).reshape(-1)
    wo_t = ops.xattn_tile_weight(wo.cuda())

    def case(fill):
        h16, a16 = mc.poisoned(h16_0.cuda(), BAND, BAND, ld=D + 64, fill=fill, pad="poison")
        h32, a32 = mc.poisoned(h16_0.float().cuda(), BAND, BAND, ld=D + 64, fill=fill, pad="poison")
        b16, b32 = a16.buf.clone(), a32.buf.clone()
        ops.qformer_xattn_out(h16, None if res16 else h32, Fr, K, S, pin(ctx0, fill, ld=D + 64, pad="poison"), wo_t, pin(bo, fill),
                              pin(ln_g, fill), pin(ln_b, fill), 1e-12, D, heads, res16=res16)
        torch.cuda.synchronize()
        none = torch.zeros(Fr * S, dtype=torch.bool)
        mc.assert_unchanged(a16, b16, rowmask(qrows, Fr * S), "h16")
        mc.assert_unchanged(a32, b32, none if res16 else rowmask(qrows, Fr * S), "h32")
        return [h16[qrows.cuda()]] + ([] if res16 else [h32[qrows.cuda()]])
    outs = two_runs(case)
    y = F.layer_norm(ctx0.cuda().float() @ wo.cuda().float().t() + bo.cuda() + h16_0.cuda()[qrows.cuda()].float(), (D,),
                     ln_g.cuda(), ln_b.cuda(), 1e-12)
    if res16:
        assert (outs[0].float() - y).abs().max().item() < (4e-3 if dtype == torch.float16 else 3e-2)
    else:
        assert (outs[1] - y).abs().max().item() < (2e-3 if dtype == torch.float16 else 1.5e-2)
        assert torch.equal(outs[0], outs[1].to(dtype))


# ====================================================================================================== small kernels
def _call(name, *args):
    """a raw C-ABI call; tensors among `args` are passed as their data pointers and stay referenced until the launch has
    finished (a temporary dropped before that would hand its block back to the allocator while the kernel still reads it)"""
    from tdc_video_amd import lib as L
    raw = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    L.check(getattr(L.load(), name)(*raw), name)
    torch.cuda.synchronize()


@covers("tdc_im2col", "tdc_resample_tokens", "tdc_set_rows", "tdc_set_rows16", "tdc_token_mean", "tdc_adaptive_pool_tokens",
        "tdc_gather_rows", "tdc_fill_rows")
@pytest.mark.parametrize("dtype", DT)
def test_small_kernels(ops, dtype):
    """the shapes of test_hip_ops.test_small_kernels, each with ld > cols.  Write sets: im2col, resample, set_rows(16),
    token_mean, adaptive_pool and fill_rows write WHOLE rows of `ld` elements (im2col / resample: zeros beyond the real
    columns); gather_rows writes `cols` columns."""
    from tdc_video_amd import ops as o_
    g = gen(5)
    dc = ops._dtcode(dtype)
    st = ops._stream
    # ---- im2col: fp32 pixels (element-wise kernel), 16-bit pixels of either type (LDS-staged kernel); pixel rows past the last frame poison
    for (Hh, Ww), kinds in (((42, 56), (torch.float32, torch.float16, torch.bfloat16)), ((44, 54), (torch.float16,)),
                            ((30, 378), (torch.bfloat16, torch.float32))):
        for pdt in kinds:
            px = randn(g, 2, 3, Hh, Ww).to(pdt)
            gh, gw, ldp = Hh // 14, Ww // 14, 640 + 64

            def case(fill):
                P = pin(px.reshape(2 * 3 * Hh, Ww), fill, band=64)
                out, oa = pout((2 * gh * gw, 588), dtype, fill, ld=ldp)
                _call("tdc_im2col", ops._ptr(P), o_.px_kind(px, dtype), ops._ptr(out), ldp, 2, Hh, Ww, 14, dc, st())
                mc.assert_untouched(oa, torch.ones(2 * gh * gw, ldp, dtype=torch.bool), "patches")
                return [oa.full]
            pat, = two_runs(case)
            ref = F.unfold(px.float(), 14, stride=14).transpose(1, 2).reshape(2 * gh * gw, -1).cuda()
            assert relerr(pat[:, :588], ref) < tol(dtype) and torch.count_nonzero(pat[:, 588:]) == 0
    # ---- resample: fp32 input (element-wise), 16-bit input (16-byte kernel), with and without a cls row; index tables poisoned past n_out
    for (Dw, off, n_i, n_o, xdt) in [(64, 1, 9, 8, torch.float32), (72, 0, 9, 8, dtype), (1152, 1, 5, 4, dtype), (64, 1, 27, 24, dtype),
                                      (72, 1, 5, 4, torch.float32)]:
        B = 2
        x = randn(g, B * (off + n_i * n_i), Dw).to(xdt)
        i0, i1, fr = [t.cpu() for t in ops.bilinear_tables(n_i, n_o, "cuda")]
        ldx, ldy = ops.pad64(Dw) + 64, ops.pad64(Dw) + 64
        for odt in DT:
            def case(fill):
                X = pin(x, fill, ld=ldx)
                y, ya = pout((B * n_o * n_o, Dw), odt, fill, ld=ldy)
                _call("tdc_resample_tokens", ops._ptr(X), int(xdt == torch.float32), ldx, off, n_i, ops._ptr(y), ldy, n_o,
                      (pin(i0, fill)), (pin(i1, fill)), (pin(fr, fill)), B, Dw, dc, ops._dtcode(odt), st())
                mc.assert_untouched(ya, torch.ones(B * n_o * n_o, ldy, dtype=torch.bool), "resampled tokens")
                return [ya.full]
            y, = two_runs(case)
            grid = x.float().view(B, off + n_i * n_i, Dw)[:, off:].reshape(B, n_i, n_i, Dw).permute(0, 3, 1, 2)
            refi = F.interpolate(grid, size=(n_o, n_o), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).reshape(-1, Dw)
            assert relerr(y[:, :Dw], refi.cuda()) < tol(odt) and torch.count_nonzero(y[:, Dw:]) == 0
    # ---- set_rows / set_rows16: row `row` of every batch item, whole ld; vec past ld poison
    Bs, S, ld = 3, 5, 128
    vec = randn(g, ld)
    for f32 in (True, False):
        def case(fill):
            x, xa = pout((Bs * S, ld), torch.float32 if f32 else dtype, fill)
            if f32:
                _call("tdc_set_rows", ops._ptr(x), ld, Bs, S, 2, (pin(vec, fill)), st())
            else:
                _call("tdc_set_rows16", ops._ptr(x), ld, Bs, S, 2, (pin(vec, fill)), dc, st())
            rows = torch.arange(Bs) * S + 2
            mc.assert_untouched(xa, rowmask(rows, Bs * S))
            return [x[rows.cuda()]]
        got, = two_runs(case)
        assert torch.equal(got, vec.cuda().to(got.dtype).expand(Bs, ld))
    # ---- token mean / adaptive pool / gather / fill
    Bt, P, cols, ld = 3, 20, 72, 192
    x16 = randn(g, Bt * P, cols).to(dtype)

    def case(fill):
        y, ya = pout((Bt, ld), dtype, fill)
        _call("tdc_token_mean", (pin(x16, fill, ld=ld)), P, ld, ops._ptr(y), Bt, dc, st())
        mc.assert_untouched(ya)
        return [y]
    y, = two_runs(case)
    assert relerr(y[:, :cols], x16.cuda().view(Bt, P, cols).float().mean(1)) < tol(dtype) and torch.count_nonzero(y[:, cols:]) == 0
    src_row = torch.tensor([2, 0], dtype=torch.int32)
    frame_rows, Np, Kp = 23, 20, 6                      # 3 extra rows per frame that are not pooled: poison
    keep_rows = torch.cat([torch.arange(Np) + f * frame_rows for f in range(3)])
    xg = randn(g, 3 * Np, cols).to(dtype)

    def case(fill):
        y, ya = pout((2 * Kp, ld), dtype, fill)
        X = pin(xg, fill, ld=ld, rows=keep_rows, total_rows=3 * frame_rows)
        _call("tdc_adaptive_pool_tokens", ops._ptr(X), Np, frame_rows, ld, ops._ptr(y), Kp, 2, (pin(src_row, fill)), dc, st())
        mc.assert_untouched(ya)
        return [y]
    y, = two_runs(case)
    refp = F.adaptive_avg_pool1d(xg.cuda().view(3, Np, cols)[[2, 0]].float().transpose(1, 2), Kp).transpose(1, 2)
    assert relerr(y[:, :cols], refp.reshape(2 * Kp, cols)) < tol(dtype) and torch.count_nonzero(y[:, cols:]) == 0
    # gather: table rows that `src` never names are poison; 72 columns -> the 16-byte path, 76 with an odd ld -> element-wise
    for gcols, gld, ldo in ((72, 192, 136), (76, 190, 132)):
        tab = randn(g, 60, gcols).to(dtype)
        vecr = randn(g, 1, gcols).to(dtype)
        src = torch.tensor([[0, 5], [1, 0], [0, 59], [1, 0], [0, 5]], dtype=torch.int32)

        def case(fill):
            T0 = pin(tab[[5, 59]], fill, ld=gld, rows=[5, 59], total_rows=60)
            T1 = pin(vecr, fill, ld=gld)
            out, oa = pout((5, gcols), dtype, fill, ld=ldo)
            ops.gather_rows([T0, T1], pin(src, fill), 5, gcols, out=out, validated=True)
            mc.assert_untouched(oa)
            return [out]
        got, = two_runs(case)
        assert torch.equal(got, torch.stack([tab[5], vecr[0], tab[59], vecr[0], tab[5]]).cuda())
    rowv = randn(g, 1, 136).to(dtype)

    def case(fill):
        out, oa = pout((37, 136), dtype, fill)
        _call("tdc_fill_rows", (pin(rowv, fill)), ops._ptr(out), 136, 37, st())
        mc.assert_untouched(oa)
        return [out]
    got, = two_runs(case)
    assert torch.equal(got, rowv.cuda().expand(37, 136))


@covers("tdc_frame_cossim", "tdc_pair_cossim", "tdc_fingerprint_rows")
@pytest.mark.parametrize("dtype", DT)
def test_cossim_and_fingerprints(ops, dtype):
    """scratch buffers are poison on entry and guarded to exactly the size the *_scratch_* query names; T = 2, n_pairs = 1;
    fingerprint rows at odd byte offsets with odd lengths: the bytes just past a row never reach the fingerprint"""
    from tdc_video_amd import lib as L
    from tdc_video_amd.cache import fingerprint_rows_host
    lib = L.load()
    g = gen(9)
    dc, st = ops._dtcode(dtype), ops._stream
    for T, n in ((2, 64), (2, 8), (7, 64 * 40), (3, 8 * 33)):
        f = randn(g, T, n).to(dtype)

        def case(fill):
            sims, sa = pout((T - 1,), torch.float32, fill)
            scr, ca = pout((lib.tdc_frame_cossim_scratch_floats(T),), torch.float32, fill)
            _call("tdc_frame_cossim", (pin(f, fill)), n, T, ops._ptr(sims), ops._ptr(scr), dc, st())
            mc.assert_untouched(sa, what="sims")
            mc.assert_untouched(ca, what="scratch")
            return [sims]
        sims, = two_runs(case)
        refs = F.cosine_similarity(f[:-1].cuda().float(), f[1:].cuda().float(), dim=1)
        assert (sims - refs).abs().max().item() < 1e-5
    # pairs over a slab with slot_stride > n: the gap behind every slot and the slots no pair names are poison
    slots, n, stride = 6, 8 * 33, 8 * 40
    slab = randn(g, slots, n).to(dtype)
    for pairs in ([(3, 1)], [(0, 3), (3, 5), (5, 1), (2, 2)]):
        used = sorted({s for p in pairs for s in p})
        pt = torch.tensor(pairs, dtype=torch.int32)

        def case(fill):
            Sl = pin(slab[used], fill, ld=stride, rows=used, total_rows=slots, pad="poison")
            sims, sa = pout((len(pairs),), torch.float32, fill)
            scr, ca = pout((lib.tdc_pair_cossim_scratch_floats(len(pairs)),), torch.float32, fill)
            _call("tdc_pair_cossim", ops._ptr(Sl), stride, n, (pin(pt, fill)), len(pairs), ops._ptr(sims), ops._ptr(scr), dc, st())
            mc.assert_untouched(sa, what="sims")
            mc.assert_untouched(ca, what="scratch")
            return [sims]
        sims, = two_runs(case)
        refs = torch.stack([F.cosine_similarity(slab[a].cuda().float(), slab[b].cuda().float(), dim=0) for a, b in pairs])
        assert (sims - refs).abs().max().item() < 1e-5
    # fingerprints: row_bytes odd, stride odd, base at an odd address (a 5-row front band of 13 bytes)
    for row_bytes, stride, front in ((11, 13, 5), (1001, 1003, 3), (17, 17, 1), (8, 24, 1), (4099, 4104, 0)):
        nrows = 9
        data = torch.randint(0, 256, (nrows, row_bytes), generator=g, dtype=torch.uint8)
        rows = [0, 1, 5, 8]
        rt = torch.tensor(rows, dtype=torch.int32)

        def case(fill):
            X = mc.poisoned(data[rows].cuda(), front, 1, ld=stride, fill=fill, rows=rows, total_rows=nrows, pad="poison", align=1)[0]
            out, oa = pout((len(rows), 2), torch.int64, fill)
            scr, ca = pout((lib.tdc_fingerprint_rows_scratch_bytes(len(rows)),), torch.uint8, fill)
            _call("tdc_fingerprint_rows", ops._ptr(X), stride, (pin(rt, fill)), len(rows), row_bytes, ops._ptr(out),
                  ops._ptr(scr), st())
            mc.assert_untouched(oa, what="fingerprints")
            mc.assert_untouched(ca, what="scratch")
            return [out]
        fp, = two_runs(case)
        assert np.array_equal(fp.cpu().numpy().view(np.uint64), fingerprint_rows_host(data[rows].numpy()))


@covers("tdc_preprocess_frames", "tdc_fbank", "tdc_relpos_gate")
@pytest.mark.parametrize("dtype", DT)
def test_preprocess_fbank_and_relpos_gate(ops, dtype):
    from tdc_video_amd import lib as L
    from tdc_video_amd import preprocess as pp
    from tdc_video_amd import beats
    lib = L.load()
    g = gen(13)
    dc, st = ops._dtcode(dtype), ops._stream
    # ---- relpos gate: q rows past `rows` poison; gate [rows, heads] with ldg > heads
    for rows, heads, hd in ((50, 12, 64), (1, 3, 16)):
        q = randn(g, rows, heads * hd).to(dtype)
        w2, b2, ga = randn(g, 2, hd, s=0.1), randn(g, 2), randn(g, heads)

        def case(fill):
            out, oa = pout((rows, heads), torch.float32, fill, ld=16)
            ops.relpos_gate(pin(q, fill, ld=ops.pad64(heads * hd) + 64), rows, heads, hd, pin(w2.reshape(-1), fill), pin(b2, fill), pin(ga, fill),
                            out=out)
            mc.assert_untouched(oa)
            return [out]
        gate, = two_runs(case)
        qh = q.cuda().float().view(rows, heads, hd)
        lg = torch.sigmoid(qh @ w2.cuda().t() + b2.cuda())
        ref = lg[..., 0] * (lg[..., 1] * ga.cuda()[None] - 1.0) + 2.0
        assert (gate - ref).abs().max().item() < 1e-5        # test_relpos_gate_and_biased_attention's bound
    # ---- fbank: the shortest waveform that gives one 16-frame patch row; the waveform past n_samples of the last item poison
    n = 400 + 15 * 160
    assert lib.tdc_fbank_frames(n) == 16 and lib.tdc_fbank_frames(n - 1) == 15
    tables = beats.fbank_tables(torch.device("cuda"))
    for B, wdt in ((1, torch.float32), (2, torch.float16)):
        wav = (randn(g, B, n, s=0.1)).to(wdt)

        def case(fill):
            Wv = pin(wav, fill, band=4)
            patches, pa = pout((B * 8, 256), dtype, fill)
            plain, la = pout((B * 16, 128), torch.float32, fill)
            window, tw, banks, rng = tables
            _call("tdc_fbank", ops._ptr(Wv), int(wdt == torch.float32), n, Wv.stride(0), B, ops._ptr(window), ops._ptr(tw), ops._ptr(banks),
                  ops._ptr(rng), ops._ptr(plain), ops._ptr(patches), 256, dc, 15.41663, 1.0 / (2 * 6.55582), st())
            mc.assert_untouched(pa, what="patches")
            mc.assert_untouched(la, what="plain")
            return [patches, plain]
        patches, plain = two_runs(case)
        # value: the Kaldi restatement of the oracle under test_hip_beats.test_fbank_vs_oracle's bounds; the patch layout is the
        # im2col of the 16 x 16 / stride-16 conv of the plain fbank, cast once
        from test_beats import BO
        want = BO.preprocess(wav.float())
        plain = plain.view(B, 16, 128)
        assert tuple(want.shape) == (B, 16, 128)
        err = (plain.cpu() - want).abs()
        assert float(err.max()) < 2e-3 and float(err.mean()) < 2e-5, (float(err.max()), float(err.mean()))
        im = plain.reshape(B, 1, 16, 8, 16).permute(0, 1, 3, 2, 4).reshape(B * 8, 256)
        assert torch.equal(patches, im.to(dtype))
    # ---- preprocess: non-square frames, T = 1 and 2; frames past T and the scratch are poison
    for T, Hh, Ww, R in ((1, 30, 52, 28), (2, 45, 33, 42)):
        frames = torch.randint(0, 256, (T, Hh, Ww, 3), generator=g, dtype=torch.uint8)
        mean, std = (0.5, 0.4, 0.3), (0.5, 0.25, 0.2)
        import preprocess_oracle as po       # the numpy restatement of Pillow's resample (byte-exact against Pillow: test_preprocess.py)
        ref16 = torch.from_numpy(po.process_frames(frames.numpy(), R, mean, std))
        b_, k_ = pp.resize_tables(max(Hh, Ww), R)
        ksize, pad = k_.shape[1], [int(v * 255) for v in mean]
        tabs = (torch.from_numpy(b_), torch.from_numpy(k_).contiguous(), torch.from_numpy(pp.norm_table(mean, std)).contiguous())

        def case(fill, f32=False):
            Fm = pin(frames.reshape(T * Hh, Ww * 3), fill, band=8)
            out, oa = pout((T * 3 * R, R), torch.float32 if f32 else dtype, fill, band=R)
            scr, ca = pout((lib.tdc_preprocess_scratch_bytes(T, Hh, Ww, R),), torch.uint8, fill)
            bounds, coeffs, lut = [pin(t, fill, band=4) for t in tabs]   # the tables past their R / 3 rows are poison too
            _call("tdc_preprocess_frames", ops._ptr(Fm), T, Hh, Ww, R, ops._ptr(bounds), ops._ptr(coeffs), ksize, pad[0], pad[1], pad[2],
                  ops._ptr(lut), ops._ptr(out), int(f32), dc, ops._ptr(scr), st())
            mc.assert_untouched(oa, what="out")
            mc.assert_untouched(ca, what="scratch")
            return [out]
        out, = two_runs(case)
        out32, = two_runs(lambda fill: case(fill, True))
        # test_hip_preprocess_bit_exact's assertions: the fp16 result is the oracle's, bit for bit; the 16-bit results are the
        # fp32 one rounded once
        assert torch.equal(out32.view(T, 3, R, R).half().cpu(), ref16) and torch.equal(out, out32.to(dtype))


# ====================================================================================================== detection, end to end
@covers("tdc_gemm", "tdc_attention")
def test_the_net_catches_a_kernel_that_is_given_more_than_the_test_declares(ops):
    """The detection path on the GPU, with every access inside an arena: the kernel is handed one row MORE than the test
    declares (all of it inside memory the test owns), so its legitimate store / load is an out-of-contract one to the checker."""
    g = gen(1)
    dtype = torch.float16
    M, N, K = 129, 68, 64
    a, w = randn(g, M + 1, K).to(dtype), randn(g, N, K).to(dtype)
    c, ca = pout((M, N), dtype, mc.NAN_FF, ld=128)
    ops.gemm(pin(a, mc.NAN_FF), pin(w, mc.NAN_FF), out=ca.buf[ca.front:].view(dtype)[:(M + 1) * 128].view(M + 1, 128)[:, :N], M=M + 1)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"\(%d, 0\)" % M):
        mc.assert_untouched(ca)
    # tdc_attention: sq + 1 rows written, sq declared
    B, H, d, sq, sk = 1, 2, 64, 65, 70
    D = H * d
    q, kv = randn(g, sq + 1, D).to(dtype), randn(g, sk, 2 * D).to(dtype)
    o, oa = pout((sq, D), dtype, mc.NAN_FF, ld=D)
    kvb = pin(kv, mc.NAN_FF)
    big = oa.buf[oa.front:].view(dtype)[:(sq + 1) * D].view(sq + 1, D)
    ops.attention(pin(q, mc.NAN_FF), kvb[:, :D], kvb[:, D:], big, B, H, d, sq + 1, sk, 0.125, (sq + 1) * D, sk * 2 * D, sk * 2 * D,
                  (sq + 1) * D)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"\(%d, 0\)" % sq):
        mc.assert_untouched(oa)
    # read set: one key row too few declared (sk - 1 rows of data, the kernel is told sk): zero and 0xFF runs differ

    def case(fill):
        kvp = pin(kv[:sk - 1], fill, band=4)
        k_ = kvp.as_strided((sk, D), (2 * D, 1), kvp.storage_offset())
        v_ = kvp.as_strided((sk, D), (2 * D, 1), kvp.storage_offset() + D)
        o, _ = pout((sq, D), dtype, fill, ld=D)
        ops.attention(pin(q[:sq], fill), k_, v_, o, B, H, d, sq, sk, 0.125, sq * D, sk * 2 * D, sk * 2 * D, sq * D)
        return [o]
    with pytest.raises(AssertionError, match="not finite|outside the declared read set"):
        two_runs(case)


# ====================================================================================================== composites, pipeline
def _guard_workspaces(enc, fill, arenas, refill=True):
    """enc._workspace -> a guarded arena of exactly the bytes the composite asked for (kept per key like the engine's own, so a
    second call reuses the bytes the first one left)"""
    kept = enc.__dict__.setdefault("_guarded_ws", {})

    def ws(key, nbytes):
        if key not in kept or kept[key][1].rows < nbytes:                # grown, never shrunk: as VideoEncoder._workspace
            kept[key] = mc.guarded((int(nbytes),), torch.uint8, "cuda", 4096, 4096, fill=fill)
            arenas.append((key, kept[key][1]))
        return kept[key][0][:nbytes]
    enc._workspace = ws


def _three_states(enc, run, run_other, arenas_check=True):
    """run() with the workspace all-zero, all-0xFF, then straight after a DIFFERENT input without refilling"""
    outs = []
    for fill in mc.PATTERNS:
        enc.__dict__.pop("_guarded_ws", None)
        ars = []
        _guard_workspaces(enc, fill, ars)
        outs.append(run())
        torch.cuda.synchronize()
        for key, a in ars:
            mc.assert_untouched(a, what="workspace %s" % key)          # nothing beyond *_workspace_bytes()
    run_other()
    outs.append(run())
    torch.cuda.synchronize()
    for key, a in ars:
        mc.assert_untouched(a, what="workspace %s (second use)" % key)
    return outs


def _same_all(outs):
    for o in outs[1:]:
        assert mc.same_bits(outs[0], o), "the composite's result depends on what its workspace held on entry"
    assert mc.all_finite(outs[0])


@covers("tdc_vit_fwd")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("fuse", ["0", "1"])
def test_vit_composite_workspace_and_output(dtype, fuse, monkeypatch):
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import weights as Wt
    from tdc_video_amd.pipeline import VideoEncoder
    from util import load_fixture
    out_arenas = mc.poison_empty(monkeypatch, mc.NAN_FF, guard_bytes=1 << 16)
    for name, prep in (("siglip_small.npz", "siglip"), ("dino_small.npz", "dino")):
        W, o = load_fixture(name)
        enc = VideoEncoder.__new__(VideoEncoder)
        enc.dtype, enc.dev, enc.tower_batch = dtype, torch.device("cuda"), 2
        enc._tables = {}
        enc.out_grid = [8, 8]
        enc.towers = {prep: (Wt.prep_siglip if prep == "siglip" else Wt.prep_dino)(W, 4, dtype, enc.dev, ln_fuse=fuse == "1")}
        enc.native_towers = True
        px = torch.from_numpy(o["pixels"]).cuda()
        outs = _three_states(enc, lambda: enc.tower(prep, px).clone(), lambda: enc.tower(prep, (px * 0.5 + 0.3).contiguous()))
        _same_all(outs)
        for a in out_arenas:
            mc.assert_untouched(a, what="a tensor the tower path allocated")
        enc.native_towers = False
        assert mc.same_bits(enc.tower(prep, px), outs[0]), name      # the value: bit for bit the kernel sequence


def _fixture_encoder(name, dtype):
    import synth
    from util import load_fixture, pipeline_cfg
    from test_hip_pipeline import make_encoder
    W, o = load_fixture(name)
    enc = make_encoder(W, pipeline_cfg(o), dtype)
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    return enc, o, vid


@covers("tdc_connector_fwd")
@pytest.mark.parametrize("dtype", DT)
def test_connector_composite_workspace_and_output(dtype, monkeypatch):
    for name in ("pipeline_T10_land.npz", "pipeline_T40.npz"):
        enc, o, vid = _fixture_encoder(name, dtype)
        vid = vid[:12]
        T = vid.shape[0]
        sig, dino = enc.tower("siglip", vid.cuda()), enc.tower("dino", (vid + 0.01).cuda())
        sizes = [tuple(int(v) for v in o["image_size"])] * T
        enc.native_connector = True
        with monkeypatch.context() as mp:
            out_arenas = mc.poison_empty(mp, mc.NAN_FF, guard_bytes=1 << 16)
            outs = _three_states(enc, lambda: enc.connector(sig, dino, T, sizes)[0].clone(),
                                 lambda: enc.connector((sig * 0.5).contiguous(), dino.flip(0).contiguous(), T, sizes))
            _same_all(outs)
            for a in out_arenas:
                mc.assert_untouched(a, what="a tensor the connector path allocated")
        enc.__dict__.pop("_workspace", None)
        enc.native_connector = False
        assert mc.same_bits(enc.connector(sig, dino, T, sizes)[0], outs[0]), name


@covers("tdc_qformer_fwd")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ["pipeline_T40.npz", "pipeline_T40_audio.npz"])
def test_qformer_composite_workspace_and_output(name, dtype, monkeypatch):
    import synth
    enc, o, vid = _fixture_encoder(name, dtype)
    vid = vid.cuda()
    ids = torch.from_numpy(o["input_ids"])[0]
    size = tuple(int(v) for v in o["image_size"])
    audio = None
    if "audio_wav" in o:
        audio = {"beats_windows": synth.beats_windows(torch.from_numpy(o["audio_wav"].astype(np.float32)))}
    pid = [int(i) for i in o["prompt_ids"]]
    run = lambda v=vid, p=pid: enc.encode_video(v, v + 0.01, size, len(ids), len(ids) - 1, p, audio=audio).clone()
    enc.native_qformer = True
    with monkeypatch.context() as mp:
        out_arenas = mc.poison_empty(mp, mc.NAN_FF, guard_bytes=1 << 16)
        outs = _three_states(enc, run, lambda: run(vid.flip(0).contiguous(), pid[:3]))
        _same_all(outs)
        for a in out_arenas:
            mc.assert_untouched(a, what="a tensor the pipeline allocated")
    enc.__dict__.pop("_workspace", None)
    enc.native_qformer = False
    assert mc.same_bits(run(), outs[0])


@covers("tdc_vit_fwd")
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kind", ["siglip", "dino"])
def test_vit_composite_full_width_layer_stack(kind, dtype, monkeypatch):
    """one full-width layer stack (the fixtures of test_hip_fulldim.py) through tdc_vit_fwd: workspace zero / 0xFF / reused"""
    import synth
    import test_hip_fulldim as FD
    enc = FD.encoder(synth.synth_state_dict(4, 4), dtype, tower_batch=2)
    px = synth.synth_input("pixels/" + kind, (2, 3, 384, 384) if kind == "siglip" else (2, 3, 378, 378)).cuda()
    enc.native_towers = True
    with monkeypatch.context() as mp:
        out_arenas = mc.poison_empty(mp, mc.NAN_FF, guard_bytes=1 << 16)
        outs = _three_states(enc, lambda: enc.tower(kind, px).clone(), lambda: enc.tower(kind, (px * 0.5).contiguous()))
        _same_all(outs)
        for a in out_arenas:
            mc.assert_untouched(a, what="a tensor the tower path allocated")
    enc.__dict__.pop("_workspace", None)
    enc.native_towers = False
    assert mc.same_bits(enc.tower(kind, px), outs[0])            # the value: bit for bit the kernel sequence


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ["pipeline_T40.npz", "pipeline_T10_land.npz", "pipeline_T40_audio.npz"])
@pytest.mark.parametrize("native", [True, False])
def test_encode_video_does_not_depend_on_recycled_memory(name, dtype, native, monkeypatch):
    """the whole encode_video - native composites and the Python kernel sequence - with every torch.empty of the package
    pre-filled with zero bytes and with 0xFF bytes: bit-identical, finite, within test_full_pipeline_vs_golden's tolerance;
    the same served from the frame cache and through encode_batch (cache slabs and the batch staging buffer are torch.empty)"""
    import synth
    from util import embed_fn
    from test_hip_pipeline import rel, stage_tol
    enc, o, vid = _fixture_encoder(name, dtype)
    enc.native_towers = enc.native_connector = enc.native_qformer = native
    ids = torch.from_numpy(o["input_ids"])[0]
    size = tuple(int(v) for v in o["image_size"])
    pid = [int(i) for i in o["prompt_ids"]]
    audio = None
    if "audio_wav" in o:
        audio = {"beats_windows": synth.beats_windows(torch.from_numpy(o["audio_wav"].astype(np.float32)))}
    vs, vd = vid.cuda(), (vid + 0.01).cuda()
    kw = dict(budget_text_len=len(ids), n_text_tokens=len(ids) - 1, prompt_ids=pid, audio=audio)
    res = {}
    for fill in mc.PATTERNS:
        with monkeypatch.context() as mp:
            mc.poison_empty(mp, fill)
            for k in [k for k in enc.__dict__ if k.endswith("_ws") or "_ws_" in k]:
                delattr(enc, k)                                        # the engine's kept workspaces: allocated anew, poisoned
            plain = enc.encode_video(vs, vd, size, **kw)
            cache = enc.new_cache(1 << 30)
            first = enc.encode_video(vs, vd, size, cache=cache, **kw)
            info = {}
            second = enc.encode_video(vs, vd, size, cache=cache, info=info, **kw)
            assert info["cache"]["bypassed"] is False and info["cache"]["frames_hit"] == info["cache"]["frames"] == vs.shape[0]
            assert info["cache"]["frames_encoded"] == 0                # the second question is served from the cache slabs
            sample = dict(px_siglip=vs, px_dino=vd, image_size=size, budget_text_len=len(ids), n_text_tokens=len(ids) - 1,
                          prompt_ids=pid, audio=audio, video_index=None, splice=None)
            with mp.context() as mp2:                                  # VideoEncoder.encode_batch is pipeline.encode_batch_with
                import tdc_video_amd.pipeline as PL
                calls, real_batch = [], PL.encode_batch_with
                mp2.setattr(PL, "encode_batch_with", lambda *a, **k: (calls.append(1), real_batch(*a, **k))[1])
                batch = enc.encode_batch([sample, sample])
                assert calls == [1]
            torch.cuda.synchronize()
            res[fill] = [plain, first, second] + list(batch)
    for a, b in zip(res[mc.ZERO], res[mc.NAN_FF]):
        assert mc.all_finite(b) and mc.same_bits(a, b)
    for t in res[mc.NAN_FF][1:]:
        assert mc.same_bits(t, res[mc.NAN_FF][0])                     # cached / batched == plain, bit for bit
    emb = embed_fn(o)
    pos = int(torch.where(ids == -200)[0][0])
    full = torch.cat([emb(ids[:pos]), res[mc.NAN_FF][0].float().cpu(), emb(ids[pos + 1:])])
    ref = torch.from_numpy(o["out_inputs_embeds"])[0]
    assert full.shape == ref.shape and rel(full, ref) < stage_tol(dtype)
