"""The designed GEMM / LayerNorm inputs themselves, on a CPU (tests/gemm_cases.py): a faithful emulation of the kernels' arithmetic
stays within the bound the GPU tests assert on every case, each modelled defect misses it on the case named for it, and the fp64
references agree with an independent path (F.gelu, F.layer_norm in fp64) away from the tails - so the inputs discriminate and
the bounds come from the arithmetic, not from the kernels.

`double_round` is the one defect that cannot miss the bound tenfold: two roundings to the same 16-bit type err by at most one
spacing = 2 u.  Its case plants that worst case on every element - the faithful result is within 0.01, the defect at 1.95 or more
on EVERY element, above BOUND = 1.25 - and that is what is asserted for it."""
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as gc

DT = [gc.F16, gc.BF16]
M = 300
ACTS = {"erf": gc.ERF, "tanh": gc.TANH, "swiglu": gc.SWIGLU}


def check(c, mutant=None):
    got = gc.emulate(c, mutant)
    return gc.ratios(c, got, gc.KAPPA_TIGHT)


def plain_cases(dtype):
    cs = []
    for N, K in ((132, 64), (136, 128), (192, 192)):
        cs += [gc.k_one_hot(M, N, K, dtype, dtype), gc.k_one_hot(M, N, K, dtype, gc.F32, res_dtype=gc.F32),
               gc.k_one_hot(M, N, K, dtype, dtype, res_dtype=dtype),
               gc.cancel(M, N, K, dtype, dtype), gc.cancel(M, N, K, dtype, gc.F32), gc.cancel(M, N, K, dtype, gc.F32, res_dtype=gc.F32),
               gc.bias_fine(M, N, K, dtype)]
        cs += [gc.rmw_tie(M, N, K, dtype, ct) for ct in DT]
    for K in (128, 256, 384):
        cs += [gc.k_one_hot(M, 136, K, dtype, gc.F32, fp8=True, res_dtype=gc.F32), gc.k_one_hot(M, 136, K, dtype, dtype, fp8=True),
               gc.cancel(M, 136, K, dtype, gc.F32, fp8=True, res_dtype=gc.F32), gc.cancel(M, 136, K, dtype, dtype, fp8=True)]
    return cs


@pytest.mark.parametrize("dtype", DT)
def test_faithful_emulation_stays_within_the_bound(dtype):
    worst_lin = 0.0
    for c in plain_cases(dtype):
        got = gc.emulate(c)
        r_all, r_pl = gc.ratios(c, got, gc.KAPPA_TIGHT)
        assert max(r_all, r_pl) <= gc.bound(c.out), (c.name, c.N, c.K, c.out, r_all)
        if c.exact is not None:
            assert torch.equal(got, c.exact), (c.name, c.N, c.K, c.out)
        c32 = gc.Gemm(c.name, c.a, c.w, c.dtype, gc.F32, c.bias, c.res, stats=c.stats, c1=c.c1)
        worst_lin = max(worst_lin, gc.lin_error(c32, gc.emulate(c32)))
        if c.name == "cancel":                   # the products really cancel to about 2^-10 of S (within 4x)
            c0 = gc.Gemm(c.name, c.a, c.w, c.dtype, gc.F32, stats=c.stats, c1=c.c1)
            ref, _, S, _ = gc.reference(c0)
            q = (ref.abs() / S).median().item()
            assert 2.0 ** -12 <= q <= 2.0 ** -8, q
    print("LIN_ERROR plain", dtype, worst_lin)
    assert worst_lin <= gc.KAPPA_EMU


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("act", list(ACTS))
def test_act_sweep_emulation(dtype, act):
    c = gc.act_sweep(M, 136 if act != "swiglu" else 144, dtype, ACTS[act])
    got = gc.emulate(c)
    ref3 = gc.reference(c)
    ref, y = ref3[0], ref3[1]
    assert torch.isfinite(got.float()).all() and torch.isfinite(ref).all()
    assert gc.sign_ok(got, ref)
    assert c.planted.sum().item() > 1000 and y.min().item() < -1e4 and y.max().item() > 1e4
    r_all, r_pl = gc.ratios(c, got, gc.KAPPA_TIGHT, ref3)
    print("RATIO emulation", act, dtype, r_all, r_pl)
    assert r_all <= gc.BOUND16 and r_pl <= gc.BOUND16
    lin = gc.Gemm(c.name, c.a, c.w, c.dtype, gc.F32, c.bias)
    assert gc.lin_error(lin, gc.emulate(lin)) <= gc.KAPPA_EMU


def test_erf_act_term_covers_the_emulation():
    """ACT / 2 bounds the fp32 emulation of gelu_erf on exact fp32 inputs; the tanh and SiLU forms need no such term (0.01 u beside the fp32 underflow)"""
    x = torch.linspace(-14.0, 14.0, 400001)
    xd = x.double()
    err = (gc.emu_gelu_erf(x).double() - gc.gelu_erf64(xd)).abs()
    assert bool((err <= 0.5 * gc.erf_act_err(xd) + 2.0 ** -126).all())
    old = (gc.emu_gelu_erf(x, cancel=True).double() - gc.gelu_erf64(xd)).abs()
    assert bool((old <= 0.5 * gc.erf_act_err(xd, "cancel") + 2.0 ** -126).all())
    m = (x >= -6) & (x <= -5)
    assert (old[m] / gc.gelu_erf64(xd[m]).abs()).max().item() > 0.9          # the former form: twice the true value
    for emu, ref in ((gc.emu_gelu_tanh(x), gc.gelu_tanh64(xd)), (gc.emu_swiglu(x, torch.ones_like(x)), gc.swiglu64(xd, torch.ones_like(xd)))):
        for dt in DT:
            rel = (emu.double() - ref).abs() / (ref.abs() * gc.U[dt] + gc.FLOORS[dt] + xd.abs() * 2.0 ** -126)
            safe = ref.abs() >= xd.abs() * 2.0 ** -120                   # the sigmoid factor clear of the fp32 underflow
            assert rel[safe].max().item() <= 0.01 and rel.max().item() <= 0.5, (rel[safe].max().item(), rel.max().item())


def fold_pair(name, dtype, stream, D=192):
    """emulated producer -> (stream rows x16, the fp32 sums, partials, stats)"""
    p = gc.fold_producer(name, M, D, 128, dtype, stream)
    sums = gc.emulate(gc.Gemm(p.name, p.a, p.w, p.dtype, gc.F32, p.bias, p.res))
    part = gc.emu_slot_partials(sums)
    mean, rstd = gc.emu_finalize(part, gc.LN_EPS)
    return p, sums, part, torch.stack([mean, rstd], 1).contiguous()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", gc.FOLD_NAMES)
@pytest.mark.parametrize("D", [192, 448])
def test_fold_emulation(dtype, name, D):
    p, sums, part, stats = fold_pair(name, dtype, gc.F32, D)
    assert torch.isfinite(stats).all()
    mean64, rstd64, _ = gc.row_stats64(sums, gc.LN_EPS)
    mtol, rtol, _ = gc.stats_tol(sums, gc.LN_EPS)
    assert bool(((stats[:, 0].double() - mean64).abs() <= mtol).all())
    assert bool(((stats[:, 1].double() - rstd64).abs() / rstd64 <= rtol).all())
    p64 = gc.slot_partials64(sums)
    for s in range(part.shape[0]):
        smt, _, m2t = gc.stats_tol(sums[:, 64 * s:64 * s + 64], 0.0)
        assert bool(((part[s, :, 0].double() - p64[s, :, 0]).abs() <= smt).all())
        assert bool(((part[s, :, 1].double() - p64[s, :, 1]).abs() <= m2t).all())
    x16 = sums.to(dtype)
    wf, c1, c2, gamma, beta, w2, b2 = gc.fold_weights(D, 136, dtype)
    for act in (gc.NONE, gc.TANH, gc.SWIGLU):
        c = gc.fold_consumer(name, x16, stats, wf, c1, c2, act)
        r_all, _ = check(c)
        assert r_all <= gc.BOUND16, (name, act, r_all)
        if act == gc.NONE:
            c32 = gc.Gemm(name, x16, wf, dtype, gc.F32, c2, stats=stats, c1=c1)
            le = gc.lin_error(c32, gc.emulate(c32))
            print('LIN_ERROR', name, D, dtype, le)
            assert le <= gc.KAPPA_EMU
            if name == "fold_large_mean":
                assert check(c, "fold_mean_16bit")[0] >= 10 * gc.BOUND16
            if name != "fold_near_constant":     # and the fold IS LayerNorm(x) W^T + b: F.layer_norm in fp64 (well-conditioned rows)
                ref, _, S, _ = gc.reference(c)
                ln = F.layer_norm(x16.double(), (D,), gamma.double(), beta.double(), gc.LN_EPS) @ w2.double().t() + b2.double()
                # differences: W' = the 16-bit rounding of w2 gamma, and the emulated fp32 stats
                assert ((ref - ln).abs() / S).max().item() < 4 * gc.U[dtype]


def test_finalize_emulation_and_its_mutant():
    part = gc.slot_means_differ(M, 7)
    mean, rstd = gc.emu_finalize(part, gc.LN_EPS)
    m64, r64 = gc.finalize64(part, gc.LN_EPS)
    mtol, rtol = gc.finalize_tol(part, gc.LN_EPS)
    assert bool(((mean.double() - m64).abs() <= mtol).all()) and bool(((rstd.double() - r64).abs() / r64 <= rtol).all())
    _, bad = gc.emu_finalize(part, gc.LN_EPS, "chan_drops_between_slot_term")
    assert bool(((bad.double() - r64).abs() / r64 >= 10 * rtol).all())
    # the partial layout agrees with an independent path: partials of real rows, finalised, are the rows' own statistics
    x = gc.fold_rows("fold_large_mean", M, 448)
    mean2, rstd2 = gc.finalize64(gc.slot_partials64(x), gc.LN_EPS)
    m, r, _ = gc.row_stats64(x, gc.LN_EPS)
    assert torch.allclose(mean2, m, rtol=1e-12) and torch.allclose(rstd2, r, rtol=1e-10)


@pytest.mark.parametrize("dtype", DT)
def test_every_gemm_mutant_misses_on_its_case(dtype):
    N, K = 136, 192
    named = {"k_one_hot": gc.k_one_hot(M, N, K, dtype, dtype), "cancel": gc.cancel(M, N, K, dtype, dtype),
             "bias_fine": gc.bias_fine(M, N, K, dtype)}
    for mutant in ("acc16", "drop_last_k_tile", "dup_first_k_tile", "swap_k_chunk", "bias_16bit"):
        c = named[gc.CAUGHT_BY[mutant]]
        assert max(check(c)) <= gc.bound(c.out)
        r = max(check(c, mutant))
        assert r >= 10 * gc.bound(c.out), (mutant, r)
        if c.exact is not None:
            assert not torch.equal(gc.emulate(c, mutant), c.exact), mutant
    for fp8c in (gc.k_one_hot(M, N, 256, dtype, gc.F32, fp8=True, res_dtype=gc.F32),):
        for mutant in ("drop_last_k_tile", "dup_first_k_tile", "swap_k_chunk"):
            assert not torch.equal(gc.emulate(fp8c, mutant), fp8c.exact), mutant
    assert max(check(gc.cancel(M, N, K, dtype, gc.F32), "acc16")) >= 10 * gc.BOUND32
    for ct in DT:                                # double_round: see the module docstring
        c = gc.rmw_tie(M, N, K, dtype, ct)
        ref3 = gc.reference(c)
        den = gc.U[ct] * ref3[0].abs() + gc.KAPPA_TIGHT * gc.U32 * ref3[2] + gc.FLOORS[ct]
        good = (gc.emulate(c).double() - ref3[0]).abs() / den
        bad = (gc.emulate(c, "double_round").double() - ref3[0]).abs() / den
        assert good.max().item() <= 0.01 and bad.min().item() >= 1.95 > gc.BOUND16, (ct, good.max().item(), bad.min().item())
    # the activation defects, on the bf16 sweep (fp16's subnormal floor hides most of the tail: reported, not asserted)
    for mutant, act in (("erf_cancel", gc.ERF), ("tanh_naive", gc.TANH)):
        c = gc.act_sweep(M, N, dtype, act)
        r = check(c, mutant)
        print("MUTANT", mutant, dtype, r)
        if dtype == gc.BF16:
            assert r[1] >= 10 * gc.BOUND16, (mutant, r)


def test_references_agree_with_an_independent_path():
    x = torch.linspace(-4.0, 12.0, 20001, dtype=torch.float64)
    assert torch.allclose(gc.gelu_erf64(x), F.gelu(x), rtol=1e-12, atol=1e-300)
    assert torch.allclose(gc.gelu_tanh64(x), F.gelu(x, approximate="tanh"), rtol=1e-11, atol=1e-300)
    assert torch.allclose(gc.swiglu64(x, x + 1), F.silu(x) * (x + 1), rtol=1e-12, atol=1e-300)
    # the derivatives, against a central difference
    h = 1e-6
    for f, df in ((gc.gelu_erf64, gc.dgelu_erf64), (gc.gelu_tanh64, gc.dgelu_tanh64)):
        assert torch.allclose(df(x), (f(x + h) - f(x - h)) / (2 * h), rtol=1e-6, atol=1e-8)
    dg, du = gc.dswiglu64(x, x + 1)
    assert torch.allclose(dg, (gc.swiglu64(x + h, x + 1) - gc.swiglu64(x - h, x + 1)) / (2 * h), rtol=1e-6, atol=1e-8)
    assert torch.allclose(du, F.silu(x), rtol=1e-12)
    # and the tails where the naive fp64 forms die: still negative, still finite
    t = torch.tensor([-8.0, -8.5, -12.0], dtype=torch.float64)
    assert bool((gc.gelu_erf64(t) < 0).all()) and bool((gc.gelu_tanh64(t) < 0).all())
    assert (0.5 * t * (1.0 + torch.tanh(0.5 * gc._u2(t))))[0].item() == 0.0
    assert (0.5 * t * (1.0 + torch.erf(t * gc.SQRT1_2)))[1].item() == 0.0
    g, b = gc.ln_params(260)
    for name in ("outlier_channel", "two_level", "large_mean"):
        xr = gc.ln_rows(name, 9, 260, gc.F32)
        ref, _ = gc.ln_reference(xr, g, b)
        assert torch.allclose(ref, F.layer_norm(xr.double(), (260,), g.double(), b.double(), gc.LN_EPS), rtol=1e-9, atol=1e-9)
    _, rstd, var = gc.row_stats64(gc.ln_rows("two_level", 9, 260, gc.F32), 0.0)
    assert bool((var == 2.25).all())


LN_COLS = (4, 60, 256, 260, 768, 772, 1024, 1028, 1280, 1284, 1536, 1540, 4096)


@pytest.mark.parametrize("name", gc.LN_ROWS)
def test_layernorm_emulation(name):
    worst = 0.0
    for cols in LN_COLS:
        g, b = gc.ln_params(cols)
        for xdt in (gc.F32, gc.F16, gc.BF16):
            x = gc.ln_rows(name, 9, cols, xdt)
            ref, T = gc.ln_reference(x, g, b)
            o = gc.emu_layernorm(x, g, b)
            assert torch.isfinite(o).all()
            worst = max(worst, gc.ln_term_error(o, ref, T))
            for odt in (gc.F32, gc.F16, gc.BF16):
                assert gc.ln_ratio(o.to(odt), ref, T, odt, gc.KAPPA_LN) <= gc.bound(odt), (name, cols, xdt, odt)
            if name == "constant":               # the output is beta up to the honest term rstd |gamma| 2^-24 |c|
                c = x.double().abs().amax(1, keepdim=True)
                assert bool(((o.double() - b.double()[None, :]).abs() <= gc.KAPPA_LN * gc.U32 * 1e3 * g.double().abs()[None, :] * c).all())
    print("LN_TERM_ERROR", name, worst)
    assert worst <= gc.KAPPA_LN_EMU


def test_layernorm_mutant_var_one_pass():
    g, b = gc.ln_params(1028)
    x = gc.ln_rows("large_mean", 9, 1028, gc.F32)
    ref, T = gc.ln_reference(x, g, b)
    assert gc.ln_ratio(gc.emu_layernorm(x, g, b), ref, T, gc.F32, gc.KAPPA_LN) <= gc.BOUND32
    assert gc.ln_ratio(gc.emu_layernorm(x, g, b, mutant="var_one_pass"), ref, T, gc.F32, gc.KAPPA_LN) >= 10 * gc.BOUND32
