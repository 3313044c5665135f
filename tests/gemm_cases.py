"""Designed inputs for the GEMM epilogues and the LayerNorm kernels, their fp64 references, a per-element error metric, a CPU
emulation of the kernels' arithmetic and named defects of that emulation (plain torch, no GPU; modelled on softmax_cases.py).

Why: `randn` operands keep |lin| below about 5 and row means near 0, and max|got - ref| / max|ref| is blind to an error on a small
element, a wrong activation tail, a double rounding or a 16-bit bias.  The cases below plant exact integers behind every K
position, products that cancel to 2^-10 of their magnitude, a bias with fp32-only bits, ties that a second rounding breaks the
other way, a sweep of known fp32 pre-activation values down to -12 and up to the largest finite value of the type, and
residual-stream rows with a large mean, an outlier channel and a near-zero variance for the LayerNorm fold.

Metric (GEMM), for every output element:

    ratio = |got - ref| / (u_out |ref| + |f'(y)| KAPPA 2^-24 S + ACT(y) + FLOOR)

  ref    fp64 result of the operands as stored; y the fp64 pre-activation value;
  u_out  unit roundoff of the output type: 2^-11 fp16, 2^-8 bf16, 2^-24 fp32;
  S      sum_k |a_k w_k| + |bias| + |res| - for the LayerNorm-fold consumer rstd (sum_k |x_k W'_nk| + |mean c1_n|) + |bias_n|, for
         e4m3 operands s (sum_k |a_k w_k|) + |bias| + |res| with s the row's dequantisation scale;
  f'     fp64 derivative of the activation (1 without one; SwiGLU: |d/dgate| S_gate + |d/dup| S_up);
  FLOOR  2^-25 for fp16 (half the subnormal spacing), else 2^-126;
  ACT    the activation approximation's own error: for the tanh (sigmoid) and SiLU forms - emulated in fp32 with exact exp2 and
         reciprocal they stay within 0.01 u of fp64 beyond the fp32 term - only the fp32 underflow of the sigmoid factor
         (`sigmoid_act_err`: |y| 2^-126, 1e-37), `erf_act_err` for the erf form (below);
  BOUND  1.25 for 16-bit outputs (one rounding plus slack for the other terms' first-order nature), 1.0 for fp32 outputs.
         A double rounding reaches 2.

KAPPA.  DERIVED: any-order fp32 summation of K products and the bias, then one add of the residual: K + 2 (`kappa_derived`).
TIGHT: KAPPA_TIGHT = 4 x the worst |emulated lin - fp64 lin| / (2^-24 S) of the faithful emulation over every case at the test
shapes, M = 300: 5.4 measured, rounded up to 6 -> 24.  The worst is the fold consumer over `fold_outlier_channel` at K = 448 (one
product carries S, every later chunk's rounding costs 2^-24 of it); `act_sweep` reaches 1.0 (the single rounding of W + bias,
whose S is the result itself), the long sums of `cancel` 0.47.  tests/test_gemm_cases.py asserts that the emulation stays within
KAPPA_TIGHT / 4.  The factor 4 because the MFMA's internal summation of its 32 products (128 for e4m3) is not documented and
the emulation takes it as exact.  The GPU tests assert both.

erf.  gelu_erf (csrc/common.h) takes 1 + erf(z) as poly(t) exp(-z^2) for z < 0 and 2 - poly(t) exp(-z^2) otherwise (Abramowitz-
Stegun 7.1.26), both in one fma: -(0.5 |x| poly) e + max(x, 0).  Measured, fp32 emulation against 0.5 x erfc(-x / sqrt 2) in
fp64 on 4e6 points of [-14, 14]: absolute error <= 2.7e-7 |x| everywhere; on the negative side, RELATIVE to |gelu(x)|: 5.3e-5 on [-3, 0) (where the absolute term is the smaller
one anyway), 4.7e-4 on [-4, -3), 1.6e-3 on [-5, -4), 3.6e-3 on [-6, -5), 1.03e-2 on [-8, -6), 3.2e-2 on [-12, -8), 8.4e-2 below.
ACT(y) = 2 min(3e-7 |y|, rel(y) |gelu(y)|) (y < 0), 2 x 3e-7 |y| (y >= 0); the 2 for the hardware's 1-ulp v_exp_f32 / v_rcp_f32.
The former `1 + erf` form (mutant `erf_cancel`) has the absolute term alone: 257 u of a bf16 result on [-6, -5].

References use cancellation-free forms only: 0.5 x erfc(-x / sqrt 2), x sigmoid(2u), g sigmoid(g) u - the naive fp64
0.5 x (1 + tanh u) is -0.0 from x = -8 down (one ulp of 1 is all it has from -7.2) and 1 + erf dies below -8.3.

LayerNorm metric: |got - ref| / (u_out |ref| + KAPPA_LN 2^-24 (rstd |gamma| (|x| + |mean|) + |beta|) + FLOOR), BOUND as above.
KAPPA_LN = 4 x the worst ratio-to-that-term of a two-pass fp32 emulation over the designed rows at the test widths (5.3 measured on
`outlier_channel`, 3.6 on `tiny`; rounded up to 6 -> 24).  Its derived limit: the sum of `cols` values in any order errs by at
most (cols - 1) 2^-24 sum|x| / cols on the mean, so `cols + 4` bounds every first-order term (`kappa_ln_derived`).

Statistics of the fold (finalised (mean, rstd) and the per-slot partials), `stats_tol`: with n values of mean m, variance v,
largest magnitude X, each carrying an input error of at most E (0 when the values are an fp32 tensor as stored):
  |mean err| <= mean(E) + C 2^-24 mean|x|;  |var err| <= 2 sqrt(v) rms(E) + rms(E)^2 + C 2^-24 (v + sqrt(v) X),  C = log2(n) + 8:
a deviation x_i - mean inherits 2^-24 X from the rounded slot mean (a tree of depth log2 n), first order in the between-slot term of
Chan's combination, second order inside a slot.  rstd: |err| / rstd <= 0.5 |var err| / (v + eps) + 3 2^-24."""
import math

import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
E4M3 = torch.float8_e4m3fn
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: 2.0 ** -24}
FLOORS = {F16: 2.0 ** -25, BF16: 2.0 ** -126, F32: 2.0 ** -126}
U32 = 2.0 ** -24
BOUND16, BOUND32 = 1.25, 1.0
KAPPA_EMU = 6.0            # the faithful emulation's worst |lin - fp64| / (2^-24 S) stays below this (asserted on the CPU)
KAPPA_TIGHT = 4 * KAPPA_EMU
KAPPA_LN_EMU = 6.0
KAPPA_LN = 4 * KAPPA_LN_EMU
NONE, ERF, TANH, SWIGLU = 0, 1, 2, 3       # TDC_ACT_*

MUTANTS = ("acc16", "drop_last_k_tile", "dup_first_k_tile", "swap_k_chunk", "double_round", "bias_16bit", "erf_cancel",
           "tanh_naive", "fold_mean_16bit", "chan_drops_between_slot_term")
CAUGHT_BY = {"acc16": "cancel", "drop_last_k_tile": "k_one_hot", "dup_first_k_tile": "k_one_hot", "swap_k_chunk": "k_one_hot",
             "double_round": "rmw_tie", "bias_16bit": "bias_fine", "erf_cancel": "act_sweep", "tanh_naive": "act_sweep",
             "fold_mean_16bit": "fold_large_mean", "chan_drops_between_slot_term": "slot_means_differ"}


def bound(out_dtype):
    return BOUND32 if out_dtype == F32 else BOUND16


def kappa_derived(K):
    return K + 2.0


def kappa_ln_derived(cols):
    return cols + 4.0


# ------------------------------------------------------------------------------------------------------- activations, fp64
SQRT1_2 = 0.7071067811865476
C_TANH = 0.7978845608028654


def _phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_erf64(x):
    return 0.5 * x * torch.special.erfc(-x * SQRT1_2)


def dgelu_erf64(x):
    return 0.5 * torch.special.erfc(-x * SQRT1_2) + x * _phi(x)


def _u2(x):
    return 2.0 * C_TANH * (x + 0.044715 * x * x * x)


def gelu_tanh64(x):
    return x * torch.sigmoid(_u2(x))


def dgelu_tanh64(x):
    s = torch.sigmoid(_u2(x))
    return s + x * s * (1.0 - s) * 2.0 * C_TANH * (1.0 + 3.0 * 0.044715 * x * x)


def swiglu64(g, u):
    return g * torch.sigmoid(g) * u


def dswiglu64(g, u):
    s = torch.sigmoid(g)
    return u * (s + g * s * (1.0 - s)), g * s


_ERF_REL = ((-3.0, 5.3e-5), (-4.0, 4.7e-4), (-5.0, 1.6e-3), (-6.0, 3.6e-3), (-8.0, 1.03e-2), (-12.0, 3.2e-2))
_ERF_REL_BELOW = 8.4e-2
ERF_ABS = 3.0e-7


def erf_act_err(y, form="erfc"):
    """ACT(y) of the module docstring for the erf epilogues (y fp64).  form="cancel": the former 1 + erf formula, whose only
    bound is the absolute one."""
    a = ERF_ABS * y.abs()
    if form == "cancel":
        return 2.0 * a
    rel = torch.full_like(y, _ERF_REL_BELOW)
    for lo, r in reversed(_ERF_REL):
        rel = torch.where(y >= lo, torch.full_like(y, r), rel)
    return 2.0 * torch.where(y < 0, torch.minimum(a, rel * gelu_erf64(y).abs()), a)


def sigmoid_act_err(mag, y):
    """ACT of the tanh (sigmoid) and SiLU forms, x / (1 + 2^z) in fp32: the factor 1 / (1 + 2^z) is 0 once 2^z overflows (z >= 128)
    and an fp32 subnormal - flushed by v_rcp_f32, short of bits in the emulation - below 2^-126, so the result is lost where the
    sigmoid is below 2^-126: |gelu_tanh(y)| < |y| 2^-126 (y in (-10.07, -10.0): 3e-38, which bf16 and fp32 can hold).  The term is
    that threshold, mag 2^-126 on the negative side, mag = |y| (SwiGLU: |gate up|); nothing else is needed (0.01 u emulated)."""
    return torch.where(y < 0, mag * 2.0 ** -126, torch.zeros_like(y))


# -------------------------------------------------------------------------------------------------------------- the case
class Gemm:
    """Operands as stored.  a [M, K], w [N, K]: the 16-bit type `dtype` or e4m3; bias fp32 [N] or None; res [M, N] (fp32 or
    16-bit) or None; out: the output dtype; stats [M, 2] / c1 [N]: the fold operands ((mean, rstd); for e4m3 (*, s_a s_w));
    planted: bool mask [M, n_out] of the elements the plant acts on (None: all); exact: the exact expected output or None."""

    def __init__(self, name, a, w, dtype, out, bias=None, res=None, act=NONE, stats=None, c1=None, planted=None, exact=None):
        self.name, self.a, self.w, self.dtype, self.out, self.bias, self.res, self.act = name, a, w, dtype, out, bias, res, act
        self.stats, self.c1, self.planted, self.exact = stats, c1, planted, exact
        self.fp8 = a.dtype == E4M3
        self.M, self.K = a.shape
        self.N = w.shape[0]

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)
        c = Gemm(self.name, mv(self.a), mv(self.w), self.dtype, self.out, mv(self.bias), mv(self.res), self.act, mv(self.stats),
                 mv(self.c1), mv(self.planted), mv(self.exact))
        return c

    def rows(self, lo, hi):
        sl = lambda t: None if t is None else t[lo:hi].contiguous()
        return Gemm(self.name, sl(self.a), self.w, self.dtype, self.out, self.bias, sl(self.res), self.act, sl(self.stats), self.c1,
                    sl(self.planted), sl(self.exact))


def reference(c):
    """(ref, y, dS, mag) in fp64 on the device the operands live on: the result, the pre-activation value (the gate column's for
    SwiGLU), |f'| S of the metric and, for SwiGLU, |gate up| (sigmoid_act_err; None otherwise)."""
    a, w = c.a.double(), c.w.double()
    acc = a @ w.t()
    s_abs = a.abs() @ w.abs().t()
    zero = torch.zeros((), dtype=torch.float64, device=a.device)
    bias = c.bias.double()[None, :] if c.bias is not None else zero
    if c.stats is not None:
        mean, rstd = c.stats[:, 0:1].double(), c.stats[:, 1:2].double()
        if c.fp8:
            y, S = rstd * acc + bias, rstd.abs() * s_abs + bias.abs()
        else:
            c1 = c.c1.double()[None, :]
            y, S = rstd * (acc - mean * c1) + bias, rstd.abs() * (s_abs + (mean * c1).abs()) + bias.abs()
    else:
        y, S = acc + bias, s_abs + bias.abs()
    if c.res is not None:
        assert c.act == NONE
        y, S = y + c.res.double(), S + c.res.double().abs()
    if c.act == NONE:
        return y, y, S, None
    if c.act == ERF:
        return gelu_erf64(y), y, dgelu_erf64(y).abs() * S, None
    if c.act == TANH:
        return gelu_tanh64(y), y, dgelu_tanh64(y).abs() * S, None
    g, u = y[:, 0::2], y[:, 1::2]
    dg, du = dswiglu64(g, u)
    return swiglu64(g, u), g, dg.abs() * S[:, 0::2] + du.abs() * S[:, 1::2], (g * u).abs()


def ratios(c, got, kappa, ref3=None, erf_form="erfc"):
    """(ratio over all elements, ratio over the planted ones); a non-finite output counts as infinite"""
    ref, y, dS, mag = ref3 if ref3 is not None else reference(c)
    den = U[c.out] * ref.abs() + kappa * U32 * dS + FLOORS[c.out]
    if c.act == ERF:
        den = den + erf_act_err(y, erf_form)
    elif c.act == TANH:
        den = den + sigmoid_act_err(y.abs(), y)
    elif c.act == SWIGLU:
        den = den + sigmoid_act_err(mag, y)
    r = torch.nan_to_num((got.double() - ref).abs() / den, nan=float("inf"))
    pl = r[c.planted] if c.planted is not None else r
    return r.max().item(), (pl.max().item() if pl.numel() else 0.0)


def lin_error(c, lin32):
    """worst |lin32 - fp64 pre-activation| / (2^-24 S) - what KAPPA_TIGHT is measured from (act == NONE cases, fp32 `lin32`)"""
    assert c.act == NONE
    ref, _, S, _ = reference(c)
    return ((lin32.double() - ref).abs() / (U32 * S).clamp_min(1e-300)).max().item()


def sign_ok(got, ref):
    """every element is zero or has the reference's sign"""
    g = got.double()
    return bool(((g == 0) | (torch.sign(g) == torch.sign(ref)) | (ref == 0)).all())


# ---------------------------------------------------------------------------------------------------------------- inputs
def _ulp1(dtype):
    return {F16: 2.0 ** -10, BF16: 2.0 ** -7, E4M3: 2.0 ** -3}[dtype]


def _op(t, dtype, fp8):
    return t.to(E4M3) if fp8 else t.to(dtype)


def k_one_hot(M, N, K, dtype, out, fp8=False, res_dtype=None, with_bias=True):
    """Row m of A is one 1.0 at k = 7 m mod K; W small integers, asymmetric in n and k; integer bias and residual: the output is
    exactly W[n, k(m)] + b[n] + r[m, n] (|.| <= 16: exact in every type, e4m3 included).  res_dtype None: no residual."""
    m, n, k = torch.arange(M), torch.arange(N), torch.arange(K)
    km = (7 * m) % K
    a = torch.zeros(M, K)
    a[m, km] = 1.0
    w = ((5 * n[:, None] + 3 * k[None, :] + (n[:, None] * k[None, :]) % 7) % 15 - 7).float()
    bias = (n % 9 - 4).float() if with_bias else None
    res = ((3 * m[:, None] + n[None, :]) % 11 - 5).float().to(res_dtype) if res_dtype is not None else None
    exact = w[:, km].t() + (bias[None, :] if with_bias else 0.0) + (res.float() if res is not None else 0.0)
    stats = torch.stack([torch.zeros(M), torch.ones(M)], 1).contiguous() if fp8 else None
    return Gemm("k_one_hot", _op(a, dtype, fp8), _op(w, dtype, fp8), dtype, out, bias, res, stats=stats,
                c1=torch.zeros(N) if fp8 else None, exact=exact.to(out))


def cancel(M, N, K, dtype, out, fp8=False, res_dtype=None, seed=0):
    """The second half of K repeats the first with W negated but for one column pair: the partial sums grow to the magnitude of
    half a dot product and the whole cancels to about 2^-10 of S = sum |a w|.  e4m3: power-of-two scales through `stats`."""
    g = torch.Generator().manual_seed(seed + 31 * K + N)
    h = K // 2
    odt = E4M3 if fp8 else dtype
    a = torch.randn(M, h, generator=g).to(odt).float()
    w = torch.randn(N, h, generator=g).to(odt).float()
    a[:, 0] = 1.0
    w[:, 0] = 1.0
    S = 2.0 * (a.abs() @ w.abs().t()).mean().item()
    step = _ulp1(odt)
    r = torch.clamp(torch.round(S * 2.0 ** -10 * (1.0 + (torch.arange(N) % 3).float() / 2.0) / step), min=1.0) * step
    a2, w2 = torch.cat([a, a], 1), torch.cat([w, -w], 1)
    w2[:, 0] = 1.0 + r                           # the one pair that does not cancel: (1 + r) - 1
    stats = c1 = None
    if fp8:
        stats = torch.stack([torch.zeros(M), 2.0 ** -((torch.arange(M) % 5).float() + 1.0)], 1).contiguous()
        c1 = torch.zeros(N)
    res = None
    if res_dtype is not None:                    # a residual of the size of the cancelled sum: it does not hide the product's error
        res = (torch.randn(M, N, generator=g) * S * 2.0 ** -10).to(res_dtype)
    return Gemm("cancel", _op(a2, dtype, fp8), _op(w2, dtype, fp8), dtype, out, None, res, stats=stats, c1=c1)


def bias_fine(M, N, K, dtype):
    """A = 0; the fp32 bias 1 + j 2^-20 has bits no 16-bit type holds; fp32 output: exactly the bias"""
    g = torch.Generator().manual_seed(3)
    bias = 1.0 + torch.arange(N).float() * 2.0 ** -20
    w = torch.randn(N, K, generator=g).to(dtype)
    return Gemm("bias_fine", torch.zeros(M, K, dtype=dtype), w, dtype, F32, bias, exact=bias[None, :].expand(M, N).contiguous())


def rmw_tie(M, N, K, dtype, ctype):
    """16-bit residual update C = T(acc + bias + float(res)), T = `ctype` with spacing e at 1.  acc = 1 exactly (one-hot A, W = 1),
    d = 2^-22.  Even columns: bias = e/2 + d, res = +e/2: the sum 1 + e + d is exact in fp32 and rounds to 1 + e (error d); rounding
    acc + bias to T first gives 1 + e, and 1 + e + e/2 is a tie that goes to the even 1 + 2e: off by e = 2 u.  Odd columns, mirrored:
    bias = 3e/2 - d, res = -e/2: 1 + e against T(T(1 + 3e/2 - d) - e/2) = T(1 + e/2) = 1."""
    e, d = _ulp1(ctype), 2.0 ** -22
    m, n = torch.arange(M), torch.arange(N)
    a = torch.zeros(M, K)
    a[m, (7 * m) % K] = 1.0
    odd = (n % 2 == 1)
    bias = torch.where(odd, torch.tensor(1.5 * e - d), torch.tensor(0.5 * e + d)).float()
    res = torch.where(odd, torch.tensor(-0.5 * e), torch.tensor(0.5 * e)).float()[None, :].expand(M, N).to(ctype).contiguous()
    return Gemm("rmw_tie", a.to(dtype), torch.ones(N, K, dtype=dtype), dtype, ctype, bias, res)


def sweep_grid(dtype):
    """4096 points of [-12, 12] on the 16-bit grid, and the specials: +-0, +-2^-14, +-2^-24, +-100, +-the largest finite value"""
    grid = torch.linspace(-12.0, 12.0, 4096).to(dtype).float()
    big = torch.finfo(dtype).max
    special = torch.tensor([0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -24, -2.0 ** -24, 100.0, -100.0, big, -big])
    return grid, special.to(dtype).float()


def act_sweep(M, N, dtype, act, K=64):
    """A one-hot at k = m mod 64 of K tile (m / 64) mod (K / 64), W the same 64 columns in every K tile, so lin[m, n] =
    W[n, m mod 64] + bias[n]: a known fp32 number.  Activation column j (every column; the even, gate, columns for SwiGLU) holds
    grid point (64 (j - 1) + k) mod 4096 at W[., k] and an fp32 bias offset off the 16-bit grid; activation column 0 holds the
    specials with bias 0.  SwiGLU's up columns hold a second, asymmetric grid of quarters in [-1, 1.5] (0.5 beside the specials:
    the largest fp16 value times it stays finite).  planted: lin < -3."""
    grid, special = sweep_grid(dtype)
    m, k = torch.arange(M), torch.arange(64)
    a = torch.zeros(M, K)
    a[m, m % 64 + 64 * ((m // 64) % (K // 64))] = 1.0
    nj = N // 2 if act == SWIGLU else N
    assert 64 * (nj - 1) >= 4096 and M >= 64, "the sweep needs 64 rows and 65 activation columns"
    j = torch.arange(nj)
    wj = grid[(64 * (j[:, None] - 1) + k[None, :]) % 4096]
    wj[0] = special[k % special.numel()]
    bj = ((j % 5).float() - 2.0) * 2.0 ** -13 + (j % 3).float() * 2.0 ** -21
    bj[0] = 0.0
    if act == SWIGLU:
        w, bias = torch.zeros(N, 64), torch.zeros(N)
        w[0::2], bias[0::2] = wj, bj
        w[1::2] = (((7 * j[:, None] + 3 * k[None, :]) % 11).float() - 4.0) / 4.0
        w[1] = 0.5
        bias[1::2] = ((j % 4).float() - 1.0) * 2.0 ** -12
        bias[1] = 0.0
    else:
        w, bias = wj, bj
    c = Gemm("act_sweep", a.to(dtype), w.repeat(1, K // 64).to(dtype), dtype, dtype, bias, act=act)
    lin = c.w.double()[:, m % 64].t() + bias.double()[None, :]
    c.planted = (lin[:, 0::2] if act == SWIGLU else lin) < -3.0
    return c


FOLD_NAMES = ("fold_large_mean", "fold_outlier_channel", "fold_near_constant")


def fold_rows(name, M, D, seed=0):
    """fp32 residual-stream rows [M, D] of the producer / consumer pair"""
    g = torch.Generator().manual_seed(seed + sum(map(ord, name)))
    z = torch.randn(M, D, generator=g)
    if name == "fold_large_mean":
        return 64.0 + z
    if name == "fold_outlier_channel":
        z[:, 5] = 500.0 * (1.0 + 0.1 * z[:, 5])
        return z
    if name == "fold_near_constant":
        return 3.0 * (1.0 + 1e-3 * z)            # variance = 1e-6 mean^2
    raise ValueError(name)


def fold_producer(name, M, D, Kp, dtype, stream_dtype, seed=0):
    """the residual-stream GEMM over the designed rows: x <- a w^T + b + x0 with an update of order 0.1; stream_dtype fp32 (the
    x16 + ln_part producer) or a 16-bit type (the read-modify-write that emits only the partials)"""
    g = torch.Generator().manual_seed(seed + 1 + sum(map(ord, name)))
    a = (torch.randint(-4, 5, (M, Kp), generator=g).float() / 8.0).to(dtype)
    w = (torch.randn(D, Kp, generator=g) * 0.1 / math.sqrt(Kp)).to(dtype)
    b = 0.05 * torch.randn(D, generator=g)
    x0 = fold_rows(name, M, D, seed).to(stream_dtype)
    return Gemm(name, a, w, dtype, stream_dtype, b, x0)


def fold_weights(D, N2, dtype, seed=0):
    """(W', c1, bias, gamma, beta, W, b): the gamma-folded consumer weight W' = W diag(gamma) (16-bit), c1 = its row sums (fp32
    of the 16-bit values), bias = beta W^T + b, and the LayerNorm / Linear parameters they were folded from"""
    g = torch.Generator().manual_seed(seed + 77)
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    w2 = torch.randn(N2, D, generator=g) / math.sqrt(D)
    b2 = torch.randn(N2, generator=g)
    wf = (w2 * gamma[None, :]).to(dtype)
    return wf, wf.float().sum(1).contiguous(), (w2 @ beta + b2).contiguous(), gamma, beta, w2, b2


def fold_consumer(name, x, stats, wf, c1, c2, act):
    """the consumer over the stream rows x (16-bit, as the producer left them) and the finalised stats as stored"""
    return Gemm(name, x, wf, x.dtype, x.dtype, c2, act=act, stats=stats, c1=c1)


def row_stats64(x, eps):
    """fp64 (mean, rstd, var) of rows of any dtype"""
    xd = x.double()
    mean = xd.mean(1)
    var = ((xd - mean[:, None]) ** 2).mean(1)
    return mean, (var + eps).rsqrt(), var


def stats_tol(x, eps, E=None):
    """(tolerance of the mean, relative tolerance of rstd, tolerance of n var) per row of x [rows, n]: module docstring"""
    xd = x.double()
    n = xd.shape[1]
    C = math.log2(n) + 8.0
    mean, _, var = row_stats64(x, 0.0)
    meanE = E.double().mean(1) if E is not None else 0.0
    rmsE = (E.double() ** 2).mean(1).sqrt() if E is not None else 0.0
    mtol = meanE + C * U32 * xd.abs().mean(1)
    vtol = 2.0 * var.sqrt() * rmsE + rmsE ** 2 + C * U32 * (var + var.sqrt() * xd.abs().amax(1))
    return mtol, 0.5 * vtol / (var + eps) + 3.0 * U32, n * vtol


def slot_partials64(x):
    """fp64 per-slot (mean, M2) [slots, rows, 2] of x [rows, 64 slots]"""
    r, n = x.shape
    xs = x.double().view(r, n // 64, 64)
    mean = xs.mean(2)
    m2 = ((xs - mean[..., None]) ** 2).sum(2)
    return torch.stack([mean.t(), m2.t()], 2).contiguous()


def slot_means_differ(rows, slots, seed=0):
    """fp32 partials [slots, rows, 2] as a producer leaves them: every slot of a row has its own mean (of order 1, spread 2) and
    an M2 of order 64 x 0.01 - the between-slot term is most of the variance"""
    g = torch.Generator().manual_seed(seed + 5)
    mean = 1.0 + 2.0 * torch.rand(slots, rows, generator=g) + 0.25 * torch.arange(slots).float()[:, None]
    m2 = 64.0 * 0.01 * (0.5 + torch.rand(slots, rows, generator=g))
    return torch.stack([mean, m2], 2).contiguous()


def finalize64(part, eps):
    """fp64 Chan combination of the partials as stored -> (mean, rstd) [rows]"""
    p = part.double()
    slots = p.shape[0]
    mean = p[..., 0].mean(0)
    q = p[..., 1].sum(0) + 64.0 * ((p[..., 0] - mean[None, :]) ** 2).sum(0)
    return mean, (q / (64.0 * slots) + eps).rsqrt()


def finalize_tol(part, eps):
    """tdc_ln_finalize's own error on stored partials: sequential fp32 sums of `slots` terms.  mean: (slots + 1) 2^-24 mean|mean_s|;
    rstd, relative: 0.5 of the variance's (slots + 4) 2^-24 (1 + 2 D X / q') with D = rms |mean_s - mean|, X = max |mean_s|,
    q' = var + eps (the deviations inherit the mean's error), + 3 2^-24."""
    p = part.double()
    slots = p.shape[0]
    mean, rstd = finalize64(part, eps)
    D = ((p[..., 0] - mean[None, :]) ** 2).mean(0).sqrt()
    X = p[..., 0].abs().amax(0)
    mtol = (slots + 1) * U32 * p[..., 0].abs().mean(0)
    return mtol, 0.5 * (slots + 4) * U32 * (1.0 + 2.0 * D * X * rstd * rstd) + 3.0 * U32


# ------------------------------------------------------------------------------------------------------------- emulation
f32 = lambda v: torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    """fp32 fma of fp32 tensors: the product of two fp32 values is exact in fp64"""
    return (a.double() * b.double() + c.double()).float()


def _erfc_pe(x):
    z = (x * f32(0.70710678118654752)).abs()
    t = 1.0 / _fma(f32(0.3275911), z, f32(1.0))
    p = _fma(f32(1.061405429), t, f32(-1.453152027))
    p = _fma(p, t, f32(1.421413741))
    p = _fma(p, t, f32(-0.284496736))
    p = _fma(p, t, f32(0.254829592))
    p = p * t
    return p, torch.exp2(f32(-1.4426950408889634) * z * z)


def emu_gelu_erf(x, cancel=False):
    p, e = _erfc_pe(x)
    if cancel:                                   # the former form: erf = copysign(1 - poly e), then 1 + erf
        return f32(0.5) * x * (f32(1.0) + torch.copysign(_fma(-p, e, f32(1.0)), x))
    h = f32(0.5) * x                             # one fma: -(0.5 |x| poly) e + max(x, 0)
    return _fma(-(h.abs() * p), e, h + h.abs())


def emu_gelu_tanh(x, naive=False):
    if naive:
        u = f32(0.7978845608028654) * (x + f32(0.044715) * x * x * x)
        return f32(0.5) * x * (f32(1.0) + torch.tanh(u))
    c0 = f32(-2.0 * 0.7978845608028654 * 1.4426950408889634)
    c1 = c0 * f32(0.044715)
    z = x * _fma(x * x, c1, c0)
    return x * (1.0 / (torch.exp2(z) + 1.0))


def emu_swiglu(g, u):
    return g * (1.0 / (torch.exp2(g * f32(-1.4426950408889634)) + 1.0)) * u


def emulate_lin(c, mutant=None):
    """fp32 linear output: sums of 32-product chunks (128 for e4m3) in K order - each chunk summed exactly, one rounding per
    chunk -, from the bias; the fold by the two fmas of EpiOps::lin (one for e4m3's scale)"""
    a, w = c.a.double(), c.w.double()
    M, K = a.shape
    ch, tile, piece = (128, 128, 16) if c.fp8 else (32, 64, 8)
    if mutant == "swap_k_chunk":                 # the first two 16-byte pieces of A in every K tile trade places
        idx = torch.arange(K)
        in_t = idx % tile
        idx = torch.where(in_t < piece, idx + piece, torch.where(in_t < 2 * piece, idx - piece, idx))
        a = a[:, idx]
    bias = c.bias if c.bias is not None else torch.zeros(c.N)
    if mutant == "bias_16bit":
        bias = bias.to(c.dtype).float()
    fold = c.stats is not None
    acc = torch.zeros(M, c.N) if fold else bias[None, :].expand(M, c.N).clone()
    spans = [(k0, k0 + ch) for k0 in range(0, K, ch)]
    if mutant == "drop_last_k_tile":
        spans = [s for s in spans if s[0] < K - tile]
    if mutant == "dup_first_k_tile":
        spans = [s for s in spans if s[0] < tile] + spans
    for k0, k1 in spans:
        acc = (acc.double() + a[:, k0:k1] @ w[:, k0:k1].t()).float()
        if mutant == "acc16":
            acc = acc.to(c.dtype).float()
    if fold:
        mean, rstd = c.stats[:, 0:1], c.stats[:, 1:2]
        if mutant == "fold_mean_16bit":
            mean = mean.to(c.dtype).float()
        if c.fp8:
            acc = _fma(rstd, acc, bias[None, :])
        else:
            acc = _fma(rstd, _fma(-mean, c.c1[None, :], acc), bias[None, :])
    return acc


def emulate(c, mutant=None):
    """the kernels' arithmetic on a CPU: emulate_lin, the activation of csrc/common.h, the residual added in fp32, ONE rounding to
    the output type.  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    lin = emulate_lin(c, mutant)
    if c.act == ERF:
        lin = emu_gelu_erf(lin, cancel=mutant == "erf_cancel")
    elif c.act == TANH:
        lin = emu_gelu_tanh(lin, naive=mutant == "tanh_naive")
    elif c.act == SWIGLU:
        lin = emu_swiglu(lin[:, 0::2], lin[:, 1::2])
    if c.res is not None:
        if mutant == "double_round":
            lin = lin.to(c.out).float()
        lin = (lin.double() + c.res.double()).float()
    return lin.to(c.out)


def emu_finalize(part, eps, mutant=None):
    """tdc_ln_finalize: sequential fp32 sums over the slots in index order"""
    slots = part.shape[0]
    sm = torch.zeros(part.shape[1])
    for s in range(slots):
        sm = sm + part[s, :, 0]
    mean = sm / f32(float(slots))
    m2, dv = torch.zeros_like(sm), torch.zeros_like(sm)
    for s in range(slots):
        d = part[s, :, 0] - mean
        m2 = m2 + part[s, :, 1]
        dv = _fma(d, d, dv)
    q = m2 if mutant == "chan_drops_between_slot_term" else m2 + f32(64.0) * dv
    return mean, 1.0 / torch.sqrt(q / f32(float(slots * 64)) + f32(eps))


def emu_slot_partials(x32):
    """per-slot (mean, M2) of fp32 rows, fp32 arithmetic [slots, rows, 2]"""
    r, n = x32.shape
    xs = x32.view(r, n // 64, 64)
    mean = xs.sum(2) * f32(0.015625)
    d = xs - mean[..., None]
    return torch.stack([mean.t(), (d * d).sum(2).t()], 2).contiguous()


# ------------------------------------------------------------------------------------------------------------- LayerNorm
LN_ROWS = ("large_mean", "outlier_channel", "constant", "tiny", "two_level")
LN_EPS = 1e-6


def ln_rows(name, rows, cols, dtype, seed=0):
    """designed rows [rows, cols] of `dtype` (fp32 or 16-bit)"""
    g = torch.Generator().manual_seed(seed + sum(map(ord, name)) + cols)
    grid = F16 if dtype == F32 else dtype
    if name == "large_mean":                     # 64 +- a few spacings of the 16-bit type at 64
        x = 64.0 + torch.randint(-3, 4, (rows, cols), generator=g).float() * (64.0 * _ulp1(grid))
    elif name == "outlier_channel":
        x = torch.randn(rows, cols, generator=g)
        x[:, 1] = 500.0
    elif name == "constant":
        x = torch.full((rows, cols), 3.140625) * (1.0 + torch.arange(rows).float()[:, None])
    elif name == "tiny":                         # variance 4e-9, far below eps = 1e-6
        x = torch.randn(rows, cols, generator=g) * 2.0 ** -14
    elif name == "two_level":                    # +-1.5, as many of each: mean 0 and variance 2.25 exactly
        x = torch.where((torch.arange(cols)[None, :] + torch.arange(rows)[:, None]) % 2 == 0, 1.5, -1.5) * torch.ones(rows, cols)
    else:
        raise ValueError(name)
    return x.to(dtype)


def ln_params(cols, seed=0):
    g = torch.Generator().manual_seed(seed + 9)
    return (1.0 + 0.2 * torch.randn(cols, generator=g)).contiguous(), (0.3 * torch.randn(cols, generator=g)).contiguous()


def ln_reference(x, gamma, beta, eps=LN_EPS, add=None):
    """(ref, T) fp64: LayerNorm of the rows as stored (+ the additive table rows `add` [rows, cols], added in fp32 by the kernel:
    the reference takes the fp32 sum as the stored operand) and the metric's term rstd |gamma| (|x| + |mean|) + |beta|"""
    xd = (x.float() + add).double() if add is not None else x.double()
    gm, bt = gamma.double()[None, :], beta.double()[None, :]
    mean, rstd, _ = row_stats64(xd, eps)
    ref = (xd - mean[:, None]) * rstd[:, None] * gm + bt
    return ref, rstd[:, None] * gm.abs() * (xd.abs() + mean.abs()[:, None]) + bt.abs()


def ln_ratio(got, ref, T, out_dtype, kappa):
    den = U[out_dtype] * ref.abs() + kappa * U32 * T + FLOORS[out_dtype]
    return torch.nan_to_num((got.double() - ref).abs() / den, nan=float("inf")).max().item()


def ln_term_error(o32, ref, T):
    """worst |fp32 result - ref| / (2^-24 T): what KAPPA_LN is measured from"""
    return ((o32.double() - ref).abs() / (U32 * T)).max().item()


def emu_layernorm(x, gamma, beta, eps=LN_EPS, mutant=None, add=None):
    """two passes over the fp32 row: mean, then the squared deviations (fp32 result before the output rounding).
    mutant var_one_pass: variance as E[x^2] - mean^2"""
    v = x.float() + add if add is not None else x.float()
    n = f32(float(v.shape[1]))
    mean = v.sum(1) / n
    d = v - mean[:, None]
    if mutant == "var_one_pass":
        var = (v * v).sum(1) / n - mean * mean
    else:
        var = (d * d).sum(1) / n
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    return d * rstd[:, None] * gamma[None, :] + beta[None, :]
