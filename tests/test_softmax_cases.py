"""The adversarial softmax cases themselves, on a CPU (tests/softmax_cases.py): a faithful emulation of the kernels' online
softmax stays within the bound the GPU tests assert on every case, and each modelled defect exceeds it tenfold on at least one
- so the inputs discriminate, and the bound is derived from the arithmetic, not read off the kernels."""
import pytest
import torch

import softmax_cases as sc

DT = [torch.float16, torch.bfloat16]
B, H = 1, 2
KLEN = {"k_len": [200]}


def all_cases(dtype, d, S, tile):
    cases = [sc.make(n, B, H, S, S, d, dtype, tile=tile) for n in sc.NAMES]
    cases += [sc.make("winner_is_last_key", B, H, 70, sk, d, dtype) for sk in (193, 225, 256)]      # last tiles of 1, 33, 64 keys
    cases.append(sc.make("k_len_edge", B, H, 70, S, d, dtype, k_len=[S - 129]))
    cases.append(sc.make_biased("late_max", B, H, 70, 196, d, dtype))
    cases.append(sc.make_biased("late_max", B, H, 70, 196, d, dtype, masked=True))
    cases.append(sc.make_biased("masked_winner", B, H, 70, 196, d, dtype))
    return cases


@pytest.fixture(scope="module")
def cases():
    return {(dtype, tile): all_cases(dtype, 64, 330, tile) for dtype in DT for tile in (64, 32)}


def worst(case, **kw):
    return max(case.ratios(sc.emulate(case, **kw)))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("thr", [0.0, 8.0])
def test_faithful_emulation_stays_within_the_bound(cases, dtype, thr):
    for tile in (64, 32):
        for case in cases[dtype, tile]:
            _, _, smax, _ = case.reference()
            assert smax.max().item() <= (256 if case.name != "all_far_negative" else 380), case.name
            r = worst(case, thr=thr)
            print("%-20s tile %d thr %g %s ratio %.2f" % (case.name, tile, thr, dtype, r))
            assert r <= sc.BOUND, (case.name, tile, r)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("S,d", [(729, 64), (729, 72)])
def test_faithful_emulation_at_the_tower_shapes(dtype, S, d):
    for name in ("randn", "late_max", "threshold"):
        case = sc.make(name, 1, 1, S, S, d, dtype)
        for thr in (0.0, 8.0):
            r = worst(case, thr=thr)
            print("%-10s S %d d %d thr %g %s ratio %.2f" % (name, S, d, thr, dtype, r))
            assert r <= sc.BOUND, (name, thr, r)


def test_fp16_subnormal_p_is_the_explicit_term():
    """one decisive key in the last tile pushes the P of its 63 tile mates to ~2^-22, an fp16 subnormal: where the winner's V
    element is ~1e-5 their absolute rounding error shows (5.69 without the term - measured alike on the GPU); bf16 is untouched"""
    case = sc.make("winner_is_last_key", 2, 2, 256, 256, 80, torch.float16)
    got = sc.emulate(case, thr=8.0)
    ref, A, _, sub = case.reference()
    assert sc.ratio(got, ref, A, torch.float16) > sc.BOUND
    assert sc.ratio(got, ref, A, torch.float16, sub=sub) <= sc.BOUND
    assert (2.0 ** -25 * sub).max().item() < 1e-5
    bf = sc.make("winner_is_last_key", 2, 2, 256, 256, 80, torch.bfloat16)
    ref, A, _, _ = bf.reference()
    assert sc.ratio(sc.emulate(bf, thr=8.0), ref, A, torch.bfloat16) <= sc.BOUND


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("thr", [0.0, 8.0])
@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_every_mutant_exceeds_the_bound_tenfold_on_the_input_designed_for_it(cases, dtype, thr, mutant):
    """not only somewhere (`one_hot` exposes five of the seven at ~1e8): each defect on the designed input(s) named for it in
    softmax_cases.CAUGHT_BY, every one of them on its own"""
    for name in sc.CAUGHT_BY[mutant]:
        hit = [c for c in cases[dtype, 64] if c.name == name]
        assert hit, name
        for case in hit:
            r = worst(case, thr=thr, mutant=mutant)
            print("%s thr %g %s: ratio %.3g on %s (%d keys)" % (mutant, thr, dtype, r, name, case.k.shape[2]))
            assert r >= 10 * sc.BOUND, (mutant, name, r)


@pytest.mark.parametrize("dtype", DT)
def test_one_hot_selects_the_row_exactly(cases, dtype):
    case = next(c for c in cases[dtype, 64] if c.name == "one_hot")
    for thr in (0.0, 8.0):
        assert case.one_hot_error(sc.emulate(case, thr=thr)) <= sc.FLOOR
    assert case.one_hot_error(sc.emulate(case, mutant="swap_pv")) >= 1


@pytest.mark.parametrize("dtype", DT)
def test_never_rescaling_is_invisible_on_randn_under_the_deferred_rule(dtype):
    """the reason for this module: at S = 729 bounded random scores never move the deferred running maximum after the first
    tile, so a kernel that never rescales again computes exactly what the faithful one does - and is far off once the maximum is
    planted late"""
    case = sc.make("randn", 1, 2, 729, 729, 64, dtype)
    good, bad = sc.emulate(case, thr=8.0), sc.emulate(case, thr=8.0, mutant="never_rescale")
    assert max(case.ratios(bad)) <= sc.BOUND
    assert max(case.ratios(bad)) == max(case.ratios(good))
    late = sc.make("late_max", 1, 2, 729, 729, 64, dtype)
    assert late.ratios(sc.emulate(late, thr=8.0, mutant="never_rescale"))[1] >= 1e3
