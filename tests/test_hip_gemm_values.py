"""GPU (-m gpu): both GEMM kernels and every epilogue form under the designed inputs of tests/gemm_cases.py, against fp64.

The value tests of test_hip_ops.py feed `randn` operands and assert max|got - ref| / max|ref|: blind to an error on a small element,
a wrong activation tail, a double rounding, a 16-bit bias.  Here every output element is bounded by gemm_cases' metric (one
rounding of the output type + KAPPA 2^-24 |f'| S + the activation's own term), once with the derived KAPPA = K + 2 and once with the
tight KAPPA_TIGHT measured on the CPU emulation (tests/test_gemm_cases.py shows there that the faithful emulation keeps it and the
modelled defects miss it); integer cases are asserted bit-exact.  Each test prints `RATIO <kernel> <epilogue> <type> <all> <planted>`.

Shapes are the smallest that reach the code.  128 x 128 kernel: M = 200, N in {132, 136, 144, 192}, K in {64, 128, 192}.
Persistent kernel: M = 96 * 256 - 19, N in {388, 392, 400, 448} - 192 tiles of 256 x 256 in 2 column tiles, the second with interior
sub-tiles, an edge sub-tile and an idle wave -, K in {128, 192, 256} (2, 3, 4 K tiles: both parities of the buffer toggle).  Every
persistent launch runs under the default grid, under 8 workgroups (24 tiles each) and under 64 (3 each): the outputs must be
bit-equal to one another and, on three 200-row windows, to the 128 x 128 kernel's rows of the same data."""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

DT = [gc.F16, gc.BF16]
TN = {gc.F16: "fp16", gc.BF16: "bf16", gc.F32: "fp32"}
M_SMALL, M_PERS = 200, 96 * 256 - 19
WINDOWS = (0, 48 * 256 - 100, M_PERS - 200)
SENT = 77.0


@pytest.fixture(scope="module")
def ops():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops as o
    assert torch.cuda.is_available()
    return o


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def launch(ops, c, off=0, ldc=None, c_map=None, c_pad8=False, ln_part=False, x16=False, separate_res=False):
    """one tdc_gemm of the device-resident case c -> dict(out=[M, n_out] (rows gathered back through c_map), part=, x16=).
    A residual is updated in place unless separate_res; off / ldc: column offset of C inside its buffer / its row stride."""
    n_out = c.N // 2 if c.act == gc.SWIGLU else c.N
    kw = {}
    if c.stats is not None:
        kw.update(ln_stats=c.stats, ln_c1=c.c1)
    if c.fp8:
        kw["out_dtype"] = c.dtype
    r = {}
    if ln_part:
        r["part"] = torch.full((c.N // 64, c.M, 2), SENT, device="cuda")
        kw["ln_part"] = r["part"]
    if x16:
        r["x16"] = torch.full((c.M, c.N), SENT, device="cuda", dtype=c.dtype)
        kw["x16"] = r["x16"]
    if c.res is not None and not separate_res:
        out = c.res.clone()
        ops.gemm(c.a, c.w, c.bias, res=out, out=out, out_f32=c.out == gc.F32, **kw)
        r["out"] = out
        return r
    rows = c.M if c_map is None else ops._map_max(c_map, c.M) + 2
    wide = (n_out + 7) // 8 * 8 if c_pad8 else n_out
    ld = ldc if ldc is not None else ops.pad64(wide + off) + 64
    buf = torch.full((rows, ld), SENT, device="cuda", dtype=c.out)
    ops.gemm(c.a, c.w, c.bias, act=c.act, res=c.res, out=buf[:, off:off + wide], out_f32=c.out == gc.F32, c_map=c_map,
             c_pad8=c_pad8, **kw)
    assert bool((buf[:, :off] == SENT).all()) and bool((buf[:, off + wide:] == SENT).all()), "columns outside C were written"
    out = buf[:, off:off + n_out]
    if c_map is not None:
        seg, stride, o, inner = c_map
        m = torch.arange(c.M, device="cuda")
        idx = (m // seg) * stride + o + (m % seg) * inner
        hit = torch.zeros(rows, dtype=torch.bool, device="cuda")
        hit[idx] = True
        assert bool((buf[~hit] == SENT).all()), "a row no m maps to was written"
        out = out[idx]
    r["out"] = out.contiguous()
    return r


def launch_grids(ops, c, **kw):
    """the persistent launch under the default grid, 8 and 64 workgroups - bit-equal -, and three 200-row windows through the
    128 x 128 kernel - bit-equal rows"""
    from tdc_video_amd import lib as L
    lib = L.load()
    runs = []
    try:
        for g in (0, 8, 64):
            assert lib.tdc_gemm_set_persistent_grid(g) != -1
            runs.append(launch(ops, c, **kw))
            torch.cuda.synchronize()
    finally:
        lib.tdc_gemm_set_persistent_grid(0)
    for other, g in zip(runs[1:], (8, 64)):
        for key in runs[0]:
            assert same_bits(runs[0][key], other[key]), (c.name, key, "persistent grid %d differs from the default grid" % g)
    if kw.get("c_map") is None:
        for lo in WINDOWS:
            sub = launch(ops, c.rows(lo, lo + 200), **kw)
            for key in sub:
                big = runs[0][key][:, lo:lo + 200] if key == "part" else runs[0][key][lo:lo + 200]
                assert same_bits(sub[key], big), (c.name, key, lo, "rows differ between the two kernels")
    return runs[0]


def run(ops, c, pers, **kw):
    return (launch_grids if pers else launch)(ops, c, **kw)


def check(c, got, worst):
    """the metric under both KAPPAs (and bit-exactness where the case has an exact answer) -> updates worst = [all, planted]"""
    assert got.dtype == c.out and torch.isfinite(got.float()).all(), c.name
    if c.exact is not None:
        assert torch.equal(got, c.exact), (c.name, TN[c.out], (got.double() - c.exact.double()).abs().max().item())
    ref3 = gc.reference(c)
    derived = gc.ratios(c, got, gc.kappa_derived(c.K), ref3)
    tight = gc.ratios(c, got, gc.KAPPA_TIGHT, ref3)
    worst[0], worst[1] = max(worst[0], tight[0]), max(worst[1], tight[1])
    b = gc.bound(c.out)
    assert max(derived) <= b, (c.name, "derived KAPPA", derived)
    assert max(tight) <= b, (c.name, "tight KAPPA", tight, derived)


def report(kernel, epi, dtype, worst):
    print("RATIO %s %s %s %.3f %.3f" % (kernel, epi, TN[dtype], worst[0], worst[1]))


NK = {False: [(N, K) for N in (132, 136, 144, 192) for K in (64, 128, 192)],
      True: [(N, K) for N in (388, 392, 400, 448) for K in (128, 192, 256)]}
NK_PARAMS = [pytest.param(p, n, k, id="%s-N%d-K%d" % ("persistent" if p else "k128", n, k)) for p in (False, True) for n, k in NK[p]]


# ------------------------------------------------------------------------------------------ plain, fp32 and residual forms
@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("pers,N,K", NK_PARAMS)
def test_store16_store32_forms(ops, dtype, pers, N, K):
    """epi_staged16 plain (N % 8 == 0; with c_pad8 at N % 8 == 4; row-mapped C), the MFMA-layout epilogue (128 x 128 kernel always;
    persistent kernel at N % 8 == 4, a C offset by 8 bytes, ldc % 8 == 4, fp32 output with a 16-bit residual), epi_staged32 without
    a residual and with an fp32 residual in place: k_one_hot bit-exact, cancel and bias_fine by the metric"""
    M = M_PERS if pers else M_SMALL
    kern = "persistent" if pers else "k128"
    dev = lambda c: c.to("cuda")
    w = [0.0, 0.0]
    for mk in (gc.k_one_hot, gc.cancel):
        check(c := dev(mk(M, N, K, dtype, dtype)), run(ops, c, pers)["out"], w)
    report(kern, "store16" if N % 8 == 0 or not pers else "mfma_n4", dtype, w)
    w = [0.0, 0.0]
    check(c := dev(gc.k_one_hot(M, N, K, dtype, dtype)), run(ops, c, pers, off=4)["out"], w)
    check(c := dev(gc.cancel(M, N, K, dtype, dtype)), run(ops, c, pers, ldc=(N + 7) // 8 * 8 + 4)["out"], w)
    report(kern, "mfma_misaligned_c_ldc4", dtype, w)
    w = [0.0, 0.0]
    check(c := dev(gc.k_one_hot(M, N, K, dtype, dtype, with_bias=False)), run(ops, c, pers, c_pad8=True)["out"], w)
    check(c := dev(gc.k_one_hot(M, N, K, dtype, dtype)), run(ops, c, pers, c_map=(7, 9, 1, 1))["out"], w)
    report(kern, "store16_pad8_rowmap", dtype, w)
    w = [0.0, 0.0]
    for c in (gc.k_one_hot(M, N, K, dtype, gc.F32), gc.cancel(M, N, K, dtype, gc.F32), gc.bias_fine(M, N, K, dtype),
              gc.k_one_hot(M, N, K, dtype, gc.F32, res_dtype=gc.F32), gc.cancel(M, N, K, dtype, gc.F32, res_dtype=gc.F32)):
        check(c := dev(c), run(ops, c, pers)["out"], w)
    report(kern, "store32_res32", dtype, w)
    w = [0.0, 0.0]
    for c in (gc.k_one_hot(M, N, K, dtype, gc.F32, res_dtype=dtype), gc.cancel(M, N, K, dtype, gc.F32, res_dtype=dtype)):
        check(c := dev(c), run(ops, c, pers, separate_res=True)["out"], w)
    report(kern, "mfma_out32_res16", dtype, w)


@pytest.mark.parametrize("ctype", DT, ids=["c_fp16", "c_bf16"])
@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("pers,N,K", NK_PARAMS)
def test_rmw16_forms(ops, dtype, ctype, pers, N, K):
    """epi_staged_rmw16 (MFMA-layout at N % 8 == 4 / on the 128 x 128 kernel), both stream types through c16_dtype_p1: the ties
    of rmw_tie that a second rounding breaks the other way, k_one_hot bit-exact, cancel; at N % 64 == 0 and one type the emitting
    form writes the same stream bits"""
    M = M_PERS if pers else M_SMALL
    w = [0.0, 0.0]
    outs = {}
    for c in (gc.rmw_tie(M, N, K, dtype, ctype), gc.k_one_hot(M, N, K, dtype, ctype, res_dtype=ctype),
              gc.cancel(M, N, K, dtype, ctype, res_dtype=ctype)):
        c = c.to("cuda")
        outs[c.name] = run(ops, c, pers)["out"]
        check(c, outs[c.name], w)
        if c.name == "rmw_tie":                  # one rounding: every planted element is the neighbour a second rounding misses
            e = gc._ulp1(ctype)
            assert torch.equal(outs[c.name].float(), torch.full_like(outs[c.name], 1.0 + e, dtype=torch.float32))
        if N % 64 == 0 and dtype == ctype:
            r = run(ops, c, pers, ln_part=True)
            assert same_bits(r["out"], outs[c.name]), c.name
    report("persistent" if pers else "k128", "rmw16", ctype, w)


# ----------------------------------------------------------------------------------------------------------- activations
ACTS = [("erf", gc.ERF), ("tanh", gc.TANH), ("swiglu", gc.SWIGLU)]


@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("act_name,act", ACTS, ids=[a[0] for a in ACTS])
@pytest.mark.parametrize("pers,N,K", [pytest.param(False, n, 64, id="k128-N%d-K64" % n) for n in (132, 136, 144, 192)] +
                         [pytest.param(True, n, k, id="persistent-N%d-K%d" % (n, k)) for n, k in ((388, 128), (392, 192), (400, 256), (448, 128))])
def test_act_sweep(ops, dtype, act_name, act, pers, N, K):
    """4096 known fp32 pre-activation values of [-12, 12], +-0, +-2^-14, +-2^-24, +-100 and the largest finite value, through
    epi_staged16 erf / tanh (N % 8 == 0), epi_staged_swiglu (N % 16 == 0) and the MFMA-layout epilogue (N % 8 == 4; SwiGLU at
    N % 16 == 8; the 128 x 128 kernel): finite, zero or correctly signed, the metric over the sweep and over lin < -3"""
    if act == gc.SWIGLU and N % 8:               # refused on the host (SwiGLU pairs columns: N % 8 == 0), nothing is written
        c = gc.act_sweep(64, 136, dtype, act)
        c = gc.Gemm(c.name, c.a, c.w[:132].contiguous(), dtype, dtype, c.bias[:132].contiguous(), act=act).to("cuda")
        with pytest.raises(Exception):
            launch(ops, c)
        return
    c = gc.act_sweep(M_PERS if pers else M_SMALL, N, dtype, act, K).to("cuda")
    got = run(ops, c, pers)["out"]
    w = [0.0, 0.0]
    check(c, got, w)
    assert gc.sign_ok(got, gc.reference(c)[0])
    report("persistent" if pers else "k128", act_name, dtype, w)
    assert c.planted.sum().item() >= 1000


# ---------------------------------------------------------------------------------------------------- the LayerNorm fold
def stats_close(stats, x, E=None):
    mean64, rstd64, _ = gc.row_stats64(x, gc.LN_EPS)
    mtol, rtol, _ = gc.stats_tol(x, gc.LN_EPS, E)
    assert torch.isfinite(stats).all()
    assert bool(((stats[:, 0].double() - mean64).abs() <= mtol).all()), ((stats[:, 0].double() - mean64).abs() / mtol).max().item()
    assert bool(((stats[:, 1].double() - rstd64).abs() / rstd64 <= rtol).all()), ((stats[:, 1].double() - rstd64).abs() / rstd64 / rtol).max().item()


def partials_close(part, x, E=None):
    p64 = gc.slot_partials64(x)
    for s in range(part.shape[0]):
        Es = E[:, 64 * s:64 * s + 64] if E is not None else None
        mt, _, m2t = gc.stats_tol(x[:, 64 * s:64 * s + 64], 0.0, Es)
        assert bool(((part[s, :, 0].double() - p64[s, :, 0]).abs() <= mt).all()), s
        assert bool(((part[s, :, 1].double() - p64[s, :, 1]).abs() <= m2t).all()), s


@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", gc.FOLD_NAMES)
@pytest.mark.parametrize("stream", ["s32", "s16"])
@pytest.mark.parametrize("pers,D,N2,Kp", [pytest.param(False, 192, 136, 64, id="k128-D192-N136"), pytest.param(False, 192, 132, 128, id="k128-D192-N132"),
                                          pytest.param(True, 448, 392, 128, id="persistent-D448-N392"),
                                          pytest.param(True, 448, 400, 192, id="persistent-D448-N400")])
def test_fold_pair(ops, dtype, name, stream, pers, D, N2, Kp):
    """the producer / consumer pair over designed stream rows.  s32: epi_staged32 with x16 + ln_part (fp32 stream, whose rows ARE the
    sums the statistics are taken of); s16: the emitting epi_staged_rmw16 (the statistics are of the unrounded fp32 sums: compared
    with the fp64 sums, each carrying the GEMM's own KAPPA 2^-24 S).  Checked against fp64: the stream by the metric, the per-slot
    partials, the finalised (mean, rstd) - finite at variance = 1e-6 mean^2 -, tdc_ln_finalize on the partials as stored, and the
    consumer (epi_staged16 / epi_staged_swiglu with the fold; MFMA-layout at N % 8 == 4) under NONE, erf, tanh and SwiGLU"""
    M = M_PERS if pers else M_SMALL
    kern = "persistent" if pers else "k128"
    p = gc.fold_producer(name, M, D, Kp, dtype, gc.F32 if stream == "s32" else dtype).to("cuda")
    r = run(ops, p, pers, ln_part=True, x16=stream == "s32")
    w = [0.0, 0.0]
    check(p, r["out"], w)
    report(kern, "producer_" + stream, p.out, w)
    if stream == "s32":
        sums, E = r["out"], None
        assert same_bits(r["x16"], sums.to(dtype))
        x = r["x16"]
    else:
        sums, _, S, _ = gc.reference(p)
        E = gc.KAPPA_TIGHT * gc.U32 * S
        x = r["out"]
    partials_close(r["part"], sums, E)
    stats = ops.ln_finalize(r["part"], D // 64, M, gc.LN_EPS)
    stats_close(stats, sums, E)
    m64, r64 = gc.finalize64(r["part"], gc.LN_EPS)
    mtol, rtol = gc.finalize_tol(r["part"], gc.LN_EPS)
    assert bool(((stats[:, 0].double() - m64).abs() <= mtol).all()) and bool(((stats[:, 1].double() - r64).abs() / r64 <= rtol).all())
    wf, c1, c2 = (t.cuda() for t in gc.fold_weights(D, N2, dtype)[:3])
    for act_name, act in [("none", gc.NONE)] + ACTS:
        if act == gc.SWIGLU and N2 % 8:
            continue
        c = gc.fold_consumer(name, x, stats, wf, c1, c2, act)
        w = [0.0, 0.0]
        check(c, run(ops, c, pers)["out"], w)
        report(kern, "fold_" + act_name, dtype, w)


def test_ln_finalize_slot_means_differ(ops):
    """every slot of a row with its own mean: the between-slot term of Chan's combination is most of the variance"""
    for rows, slots in ((9, 3), (300, 7), (1000, 18)):
        part = gc.slot_means_differ(rows, slots).cuda()
        stats = ops.ln_finalize(part, slots, rows, gc.LN_EPS)
        m64, r64 = gc.finalize64(part, gc.LN_EPS)
        mtol, rtol = gc.finalize_tol(part, gc.LN_EPS)
        assert bool(((stats[:, 0].double() - m64).abs() <= mtol).all())
        rel = (stats[:, 1].double() - r64).abs() / r64
        print("RATIO ln_finalize slot_means_differ fp32 %.3f %.3f" % ((rel / rtol).max().item(), (rel / rtol).max().item()))
        assert bool((rel <= rtol).all())
        within = (part[..., 1].double().sum(0) / (64.0 * slots) + gc.LN_EPS).rsqrt()       # without the between-slot term
        assert bool(((within - r64).abs() / r64 >= 10 * rtol).all())


# ------------------------------------------------------------------------------------------------------- e4m3 operands
@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("pers,N,K", [pytest.param(p, n, k, id="%s-N%d-K%d" % ("persistent" if p else "k128", n, k))
                                      for p, ns in ((False, (132, 136, 192)), (True, (388, 392, 448))) for n, k in zip(ns, (128, 256, 384))])
def test_e4m3_operands(ops, dtype, pers, N, K):
    """the e4m3-operand instantiations (v_mfma_f32_16x16x128_f8f6f4), scales through ln_stats exact powers of two: k_one_hot
    bit-exact and cancel by the metric, with an fp32 output + fp32 residual (epi_staged32's fold ring), a 16-bit output
    (epi_staged16 with the scale fold) and the 16-bit read-modify-write"""
    M = M_PERS if pers else M_SMALL
    w = [0.0, 0.0]
    for mk in (gc.k_one_hot, gc.cancel):
        for out, res in ((gc.F32, gc.F32), (dtype, None), (dtype, dtype)):
            if res == dtype and N % 8:
                continue                         # the 16-bit read-modify-write on e4m3 operands needs N % 8 == 0 (refused otherwise)
            c = mk(M, N, K, dtype, out, fp8=True, res_dtype=res).to("cuda")
            check(c, run(ops, c, pers)["out"], w)
    report("persistent" if pers else "k128", "e4m3", dtype, w)
