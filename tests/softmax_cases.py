"""Adversarial softmax inputs for the attention kernels, their fp64 reference, the error metric and a CPU emulation of the
kernels' online softmax (plain torch, no GPU).

Why: `randn` q / k / v at S = 729 give a nearly uniform softmax - the output is a mean of V and the running maximum settles in
the first key tile or two -, so a kernel that rescales its accumulator wrongly when the maximum moves late, or mishandles the
one key that decides a row, passes a `randn` test.  The cases below move the maximum late, sit on both sides of the deferred
rescale's threshold, put the decisive key on the last valid key of a masked tile, behind a `k_len` or under a `key_mask`.

Metric.  With u the unit roundoff of the 16-bit type (2^-11 fp16, 2^-8 bf16) and A[row, col] = sum_k p_k |v_k[col]| the
softmax-weighted mean of |V|, a kernel that rounds P to the type once and its output once is, to first order, within 2 u A of
the exact result on every element.  ratio = max |got - ref| / (u A + 2^-24); the tests allow BOUND = 3 (one more u for the fp32
effects: score rounding, exp2, the order of the sums).  The faithful emulation below reaches about 1.75.
One explicit term is subtracted from the error first, in fp16 only: P = 2^(s - m) below 2^-14 is an fp16 SUBNORMAL, rounded to
a multiple of 2^-24 - an absolute error of up to 2^-25 per key instead of u p.  A stored P is never smaller than the key's final
weight p_k (the offset m only grows and the row sum is >= 1), so only keys with p_k < 2^-14 can be hit, each by at most 2^-25 of
weight: SUB[row, col] = 2^-25 sum over {k: p_k < 2^-14} of |v_k[col]|.  It is a few 1e-6 at these lengths and only shows where
the output itself is that small (one decisive key whose V element is ~1e-5: `winner_is_last_key` at head dim 80, 256 keys,
where the faithful emulation and the kernel both read 5.69 without the term).  bf16 has fp32's exponent range: no term.

Designed inputs start from `randn` with column 0 of every head reserved for the plant (q column 0 is QA on the planted queries
- every third - and 0 elsewhere, k column 0 is 0 but on the planted keys), so a plant of x base-2 units is a k value of
x / (QA scale log2 e).  |score log2 e| stays <= 256 (fp32 score rounding below 0.03 u) but for `all_far_negative`, which the
-250 natural units it is defined by put at 361 (half an ulp of the score there: 2^-16, 0.03 u in fp16)."""
import math

import torch

LOG2E = 1.4426950408889634
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
BOUND = 3.0            # see the module docstring: 2 u A first order + 1 u A for the fp32 effects
FLOOR = 2.0 ** -24
QA = 4.0               # q column 0 of a planted query
QUIET = 2.0 ** -6      # `quiet` planted queries: the other q columns scaled down, scores of unplanted keys within +-0.1 units

MUTANTS = ("never_rescale", "rescale_l_only", "drop_last_key", "double_last_key", "swap_pv", "mask_after_bias", "ignore_k_len")

# the designed input(s) that must expose each defect on their own, tenfold (tests/test_softmax_cases.py)
CAUGHT_BY = {"never_rescale": ("late_max", "threshold"), "rescale_l_only": ("late_max", "threshold"),
             "drop_last_key": ("winner_is_last_key",), "double_last_key": ("half_is_last_key",),
             "swap_pv": ("one_hot",), "mask_after_bias": ("masked_winner",), "ignore_k_len": ("k_len_edge",)}


class Case:
    """q [B, H, sq, d], k / v [B, H, sk, d] of the 16-bit type (CPU); scale; planted: LongTensor of the query rows the plant
    acts on (None: all); k_len: list of B ints or None; bias fp32 [H, sq, sk], gate fp32 [B, sq, H], key_mask bool [B, sk] (the
    biased form) or None; sel: LongTensor [sq] of the key each query of `one_hot` selects."""

    def __init__(self, name, q, k, v, scale, dtype, planted=None, k_len=None, bias=None, gate=None, key_mask=None, sel=None,
                 p16=True):
        self.name, self.scale, self.dtype = name, scale, dtype
        self.p16 = p16         # the kernel under test rounds P to the 16-bit type (False: fp32 softmax and PV, tdc_sva_attention)
        self.q, self.k, self.v = q.to(dtype), k.to(dtype), v.to(dtype)
        self.planted, self.k_len, self.bias, self.gate, self.key_mask, self.sel = planted, k_len, bias, gate, key_mask, sel
        self._ref = None

    def reference(self):
        if self._ref is None:
            self._ref = reference(self.q, self.k, self.v, self.scale, self.bias, self.gate, self.key_mask, self.k_len)
        return self._ref

    def one_hot_error(self, got):
        """`one_hot`: max |got - the selected V row|.  The integers of V are exact in both types and the other keys weigh 2^-34,
        so a correct kernel returns the row itself; only where V is 0 may a residue below 2^-24 remain (bf16 does not underflow)."""
        return (got.double() - self.v[:, :, self.sel].double()).abs().max().item()

    def ratios(self, got):
        """(ratio over all rows, ratio over the planted rows) of got [B, H, sq, d]"""
        ref, A, _, sub = self.reference()
        if not self.p16:
            sub = None         # no P is rounded to fp16: the plain bound
        return ratio(got, ref, A, self.dtype, sub=sub), ratio(got, ref, A, self.dtype, self.planted, sub=sub)


def _valid(B, sk, key_mask, k_len):
    ok = torch.ones(B, sk, dtype=torch.bool)
    if k_len is not None:
        ok &= torch.arange(sk)[None, :] < torch.tensor(k_len)[:, None]
    if key_mask is not None:
        ok &= ~key_mask.bool()
    return ok


def reference(q, k, v, scale, bias=None, gate=None, key_mask=None, k_len=None):
    """fp64 softmax attention of the operands as stored.  Returns ref [B, H, sq, d], A = softmax @ |v| (same shape), the
    row-wise largest |score log2 e| over the valid keys [B, H, sq] and the sum of |v| over the keys with p < 2^-14 (the fp16
    subnormal term of the module docstring, before its factor 2^-25).  Keys at and beyond k_len[b] and keys under key_mask are
    excluded whatever they hold (NaN included)."""
    B, _, _, _ = q.shape
    sk = k.shape[2]
    ok = _valid(B, sk, key_mask, k_len)[:, None, None, :]
    kd = torch.where(ok.transpose(-1, -2), k.double(), torch.zeros((), dtype=torch.float64))
    vd = torch.where(ok.transpose(-1, -2), v.double(), torch.zeros((), dtype=torch.float64))
    s = (q.double() @ kd.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + gate.double().permute(0, 2, 1)[..., None] * bias.double()[None]
    smax = torch.where(ok, s.abs(), torch.zeros((), dtype=torch.float64)).amax(-1) * LOG2E
    p = torch.softmax(s.masked_fill(~ok, float("-inf")), -1)
    return p @ vd, p @ vd.abs(), smax, (p < 2.0 ** -14).double() @ vd.abs()


def ratio(got, ref, A, dtype, rows=None, sub=None):
    """max (|got - ref| - SUB) / (u A + 2^-24), SUB = 2^-25 sub in fp16 (module docstring); a non-finite output counts as infinite"""
    err = (got.double() - ref).abs()
    if sub is not None and dtype == torch.float16:
        err = (err - 2.0 ** -25 * sub).clamp_min(0.0)
    err = err / (U[dtype] * A + FLOOR)
    err = torch.nan_to_num(err, nan=float("inf"))
    if rows is not None:
        err = err[:, :, rows]
    return err.max().item()


# ---------------------------------------------------------------------------------------------------------------- inputs
def _base(B, H, sq, sk, d, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, s, d, generator=g) for s in (sq, sk, sk))
    q[..., 0] = 0
    k[..., 0] = 0
    return q, k, v, g


def _kval(units, scale):
    return units / (QA * scale * LOG2E)


def _plant_rows(q, quiet=False, every=3):
    rows = torch.arange(0, q.shape[2], every)
    if quiet:
        q[:, :, rows] *= QUIET
    q[:, :, rows, 0] = QA
    return rows


def _key(t, tile, sk):
    return min(t * tile + 2 + t % 7, sk - 1)


def make(name, B, H, sq, sk, d, dtype, tile=64, seed=0, k_len=None):
    """the case `name` for the non-biased kernels; tile: the key-tile width the plants are placed by (64, or 32 for the key blocks
    inside the 32x32x16 form)"""
    scale = 1.0 / math.sqrt(d)
    q, k, v, g = _base(B, H, sq, sk, d, seed + 1000 * sum(map(ord, name)))
    nt = (sk + tile - 1) // tile
    planted = None
    sel = None
    if name == "randn":
        pass
    elif name == "late_max":
        # a key in tile 2 beats all before it by ~20 units, one in tile 5 beats that one by ~9.5 (fewer tiles: the last two)
        planted = _plant_rows(q)
        t1, t2 = min(2, nt - 2), min(5, nt - 1)
        assert 0 <= t1 < t2
        k[:, :, _key(t1, tile, sk), 0] = _kval(20.4, scale)
        k[:, :, _key(t2, tile, sk), 0] = _kval(29.9, scale)
    elif name == "threshold":
        # quiet rows; M = 20 units, then M + 7.5 (the deferred rule stays at M: P up to 2^7.5) and M + 8.5 (it follows)
        planted = _plant_rows(q, quiet=True)
        assert nt >= 3
        ta = 2 if nt >= 6 else nt - 3
        for t, units in ((ta, 20.0), (ta + 1, 27.5), (ta + 2, 28.5)):
            k[:, :, _key(t, tile, sk), 0] = _kval(units, scale)
    elif name == "winner_is_last_key":
        planted = _plant_rows(q)
        k[:, :, sk - 1, 0] = _kval(25.0, scale)
    elif name == "one_hot":
        # +-1 code of the key index, query i selects key (37 i + 11) mod sk by 24 natural units; integer V
        scale = 1.0
        bits = max(1, (sk - 1).bit_length())
        assert bits <= d
        code = torch.zeros(sk, d)
        for bit in range(bits):
            code[:, bit] = ((torch.arange(sk) >> bit) & 1).float() * 2 - 1
        sel = (torch.arange(sq) * 37 + 11) % sk
        q = (code[sel] * 12.0).expand(B, H, sq, d).clone()
        k = code.expand(B, H, sk, d).clone()
        rows = torch.arange(sk).view(1, 1, sk, 1) + 5 * torch.arange(B).view(B, 1, 1, 1) + 3 * torch.arange(H).view(1, H, 1, 1)
        v = ((rows * 7 + torch.arange(d).view(1, 1, 1, d) * 3) % 13).float()
    elif name == "half_and_half":
        # quiet rows: the other keys share a near-uniform half, the planted key holds the other half
        planted = _plant_rows(q, quiet=True)
        k[:, :, _key(nt // 2, tile, sk), 0] = _kval(math.log2(sk - 1), scale)
    elif name == "half_is_last_key":
        # the same with the heavy key on key sk - 1: a last key dropped or counted twice moves half of the weight
        planted = _plant_rows(q, quiet=True)
        k[:, :, sk - 1, 0] = _kval(math.log2(sk - 1), scale)
    elif name == "all_far_negative":
        q[..., 0] = 16.0
        k[..., 0] = -250.0 / (16.0 * scale)
    elif name == "k_len_edge":
        # winner at k_len[b] - 1; a far larger key at k_len[b], NaN behind it (K and V): neither may matter
        assert k_len is not None and len(k_len) == B
        planted = _plant_rows(q)
        for b, n in enumerate(k_len):
            k[b, :, n - 1, 0] = _kval(25.0, scale)
            if n < sk:
                k[b, :, n, 0] = _kval(60.0, scale)
                v[b, :, n] = 1000.0
            k[b, :, n + 1:] = float("nan")
            v[b, :, n + 1:] = float("nan")
    else:
        raise ValueError(name)
    return Case(name, q, k, v, scale, dtype, planted=planted, k_len=k_len, sel=sel)


NAMES = ("late_max", "threshold", "winner_is_last_key", "one_hot", "half_and_half", "half_is_last_key", "all_far_negative")


def make_biased(name, B, H, sq, sk, d, dtype, tile=64, seed=0, masked=False):
    """cases for the biased form (score = scale q.k + gate * bias, key_mask): the plant goes through `bias`; the gate of the
    planted queries is 1 so that one bias table plants the same units in every batch item.
    late_max: as above, through the bias (masked: a quarter of the other keys under key_mask);
    masked_winner: key 3 has the largest raw score (+70 units through column 0) AND the largest bias (+130) and is masked; a key in
    the last tile wins through a bias of +25 units alone."""
    assert sk % 4 == 0
    scale = 1.0 / math.sqrt(d)
    q, k, v, g = _base(B, H, sq, sk, d, seed + 1000 * sum(map(ord, name)) + 7)
    nt = (sk + tile - 1) // tile
    bias = torch.randn(H, sq, sk, generator=g)
    gate = 0.5 + torch.rand(B, sq, H, generator=g)
    planted = torch.arange(0, sq, 3)
    gate[:, planted] = 1.0
    key_mask = None
    if name == "late_max":
        k1, k2 = _key(min(2, nt - 2), tile, sk), _key(min(5, nt - 1), tile, sk)
        bias[:, planted, k1] = 20.4 / LOG2E
        bias[:, planted, k2] = 29.9 / LOG2E
        if masked:
            key_mask = torch.rand(B, sk, generator=g) < 0.25
            key_mask[:, k1] = key_mask[:, k2] = False
    elif name == "masked_winner":
        km, kw = 3, _key(nt - 1, tile, sk)
        q[:, :, planted, 0] = QA
        k[:, :, km, 0] = _kval(70.0, scale)
        bias[:, planted, km] = 130.0 / LOG2E
        bias[:, planted, kw] = 25.0 / LOG2E
        key_mask = torch.rand(B, sk, generator=g) < 0.25
        key_mask[:, km] = True
        key_mask[:, kw] = False
    else:
        raise ValueError(name)
    return Case(name, q, k, v, scale, dtype, planted=planted, bias=bias, gate=gate, key_mask=key_mask)


# ------------------------------------------------------------------------------------------------------------- emulation
def emulate(case, tile=64, thr=0.0, mutant=None, p_ftz=False):
    """The kernels' online softmax on a CPU: fp32 raw scores, base-2 exponent arguments fma(s, scale log2 e, -m), P rounded to
    the 16-bit type for the PV product while the row sum adds the unrounded fp32 values, O and l in fp32, one rounding of O / l.
    thr = 0 models the 16x16x32 kernels (the running maximum follows every rise), thr = 8 the deferred rescale of the 32x32x16
    form (it follows a tile's maximum only when that exceeds it by more than thr base-2 units).
    mutant: one of MUTANTS - the defects the designed inputs must expose (tests/test_softmax_cases.py).
    p_ftz: fp16 P below 2^-14 becomes 0 instead of a subnormal (a diagnostic model, not what the kernels were found to do)."""
    assert mutant is None or mutant in MUTANTS
    q, k, v, dtype = case.q, case.k, case.v, case.dtype
    B, H, sq, d = q.shape
    sk = k.shape[2]
    c = torch.tensor(case.scale * LOG2E, dtype=torch.float32)
    k_len = None if mutant == "ignore_k_len" else case.k_len
    n_b = torch.tensor(k_len if k_len is not None else [sk] * B)
    valid = torch.arange(sk)[None, :] < n_b[:, None]                          # [B, sk]
    if mutant == "drop_last_key":
        valid = valid & (torch.arange(sk)[None, :] != (n_b - 1)[:, None])
    km = case.key_mask.bool() if case.key_mask is not None else torch.zeros(B, sk, dtype=torch.bool)
    o = torch.zeros(B, H, sq, d)
    l = torch.zeros(B, H, sq)
    m = torch.full((B, H, sq), float("-inf"))
    for t0 in range(0, sk, tile):
        t1 = min(t0 + tile, sk)
        ok = valid[:, None, None, t0:t1]
        kt = torch.where(ok.transpose(-1, -2), k[:, :, t0:t1].float(), torch.zeros(()))      # rows never loaded: any finite stand-in
        vt = torch.where(ok.transpose(-1, -2), v[:, :, t0:t1].float(), torch.zeros(()))
        s = (q.float() @ kt.transpose(-1, -2)) * c
        if case.bias is not None:
            s = s + (case.gate.permute(0, 2, 1)[..., None] * LOG2E) * case.bias[None, :, :, t0:t1]
        gone = ~ok | km[:, None, None, t0:t1]
        if mutant == "mask_after_bias":                                       # the statistics see the masked keys' biased scores
            s_stat = s.masked_fill(~ok, float("-inf"))
        else:
            s_stat = s = s.masked_fill(gone, float("-inf"))
        m_cand = s_stat.amax(-1)
        m_new = torch.where(m_cand > m + thr, m_cand, m)
        m_use = torch.where(m_new == float("-inf"), torch.zeros(()), m_new)
        alpha = torch.exp2(m - m_use)
        m = m_new
        p = torch.exp2(s - m_use[..., None])
        if mutant == "mask_after_bias":
            p = p.masked_fill(gone, 0.0)
        p16 = p.to(dtype).float()
        if p_ftz and dtype == torch.float16:
            p16 = torch.where(p16 < 2.0 ** -14, torch.zeros(()), p16)
        if mutant == "swap_pv" and t1 - t0 > 6:
            p16[..., [5, 6]] = p16[..., [6, 5]]
        a_l = a_o = alpha
        if t0 > 0 and mutant == "never_rescale":
            a_l = a_o = torch.ones(())
        if t0 > 0 and mutant == "rescale_l_only":
            a_o = torch.ones(())
        l = l * a_l + p.sum(-1)
        o = o * a_o[..., None] + p16 @ vt
        if mutant == "double_last_key":
            for b in range(B):
                j = int(n_b[b]) - 1
                if t0 <= j < t1:
                    l[b] += p[b, :, :, j - t0]
                    o[b] += p16[b, :, :, j - t0, None] * vt[b, :, j - t0, None, :]
    return (o / l[..., None]).to(dtype)
