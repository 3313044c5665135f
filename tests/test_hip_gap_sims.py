"""GPU (-m gpu): the gap table of a compact feature set.

  1. VideoEncoder.gap_sims_tensor - tdc_pair_cossim over every pair (i, i + g), g = 1 .. G, in calls of at most 65535 pairs -
     against tdc_frame_cossim on the pairs' frames copied adjacent (bit for bit: what the lossless path computes behind its a1
     gather) and against an fp64 cosine;
  2. the three export routes give one set, table included;
  3. encode_features at 30 of 40 frames from a set with the table: the lossless path's selection without an a5 launch, the
     tokens within the section-14 contract (the bounds of tests/test_hip_feature_store.py; measured at 30 of 40 frames:
     2.4e-4 / 4.7e-4, profiles/feature_store.json) - also through encode_features_prompts and from a saved, loaded, pinned set;
  4. a set without the table behaves as it did: "decoded", one a5 launch."""
import sys

import pytest
import torch

from test_hip_feature_store import _load, parity, planted_video
from test_hip_frame_inputs import frames_of, reference_pixels, towers
from test_hip_pipeline import make_encoder
from util import pipeline_cfg

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
TOL_COMP, TOL_STATIC = 6.1e-4, 8.2e-4           # the section-14 test bounds


@pytest.fixture(scope="module")
def fx():
    """the T = 40 fixture and its fp16 engine (refinement off, 126-px frame towers), the planted 30-of-40 video's lossless set,
    its compact set and its compact set with the table - made once"""
    f = _load()
    f["enc"] = enc = make_encoder(f["W"], pipeline_cfg(f["o"]), torch.float16)
    assert enc.selection_eps is None
    enc.frame_towers = towers()
    vid, f["idx"] = planted_video(f["o"], enc)
    f["px"] = vid.cuda(), (vid + 0.01).cuda()
    f["fs"] = enc.export_features(*f["px"], f["size"])
    f["plain"] = enc.compact_features(f["fs"])
    f["cs"] = enc.compact_features(f["fs"], gaps="auto")
    return f


def count_sims(enc):
    """-> (the list every sims_tensor launch appends its frame count to, a function that puts the method back)"""
    launches = []
    sims_tensor = enc.sims_tensor
    enc.sims_tensor = lambda d, T: launches.append(T) or sims_tensor(d, T)
    return launches, lambda: setattr(enc, "sims_tensor", sims_tensor)


# ------------------------------------------------------------------------------------------------ 1. the table launch
@pytest.mark.parametrize("dtype", DT)
def test_gap_sims_tensor_is_the_frame_kernel_on_adjacent_copies(dtype):
    f = _load()
    enc = make_encoder(f["W"], pipeline_cfg(f["o"]), dtype)
    ops = sys.modules[type(enc).__module__].ops                   # the module object the engine's launches go through
    T0, P, Dp, G = 800, 2, 64, 100
    n = P * Dp
    g = torch.Generator().manual_seed(31)
    # frames that share a direction to a varying degree: similarities from about 0 to about 1
    x = torch.randn(T0, n, generator=g) + torch.randn(1, n, generator=g) * (torch.rand(T0, 1, generator=g) * 4.0)
    rows = x.to(dtype).reshape(T0 * P, Dp).cuda()
    pairs = [(i, i + k) for k in range(1, G + 1) for i in range(T0 - k)]
    assert len(pairs) == 74950 > ops.PAIR_COSSIM_MAX                          # two tdc_pair_cossim calls
    calls = []
    pair_cossim = ops.pair_cossim
    ops.pair_cossim = lambda slab, prs, nn, **kw: calls.append((len(prs), kw.get("scratch"))) or pair_cossim(slab, prs, nn, **kw)
    try:
        table = enc.gap_sims_tensor(rows, T0, G)
    finally:
        ops.pair_cossim = pair_cossim
    assert [c[0] for c in calls] == [65535, 74950 - 65535] and calls[0][1] is not None and calls[0][1] is calls[1][1]
    assert tuple(table.shape) == (G, T0 - 1) and table.dtype == torch.float32 and table.is_cuda
    # every entry: the frame kernel on one buffer where the pair's two frames lie adjacent - one launch, every second value
    flat = torch.tensor(pairs).reshape(-1).cuda()
    buf = rows.view(T0, n)[flat].contiguous()
    want = ops.frame_cossim(buf, 2 * len(pairs), n)[0::2]
    at = torch.tensor([(j - i - 1) * (T0 - 1) + i for i, j in pairs]).cuda()
    assert torch.equal(table.view(-1)[at], want), "an entry is not the frame kernel's value for the two frames laid adjacent"
    # ... and an fp64 cosine: three fp32 sums of n = 128 terms (about 2.5e-5), doubled
    a, b = buf.view(len(pairs), 2, n)[:, 0].double(), buf.view(len(pairs), 2, n)[:, 1].double()
    cos = (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1)).clamp_min(1e-8)
    err = float((table.view(-1)[at].double() - cos).abs().max())
    print("gap table %s: max |entry - fp64 cosine| = %.3e over %d pairs, values %.3f .. %.3f" %
          (dtype, err, len(pairs), float(cos.min()), float(cos.max())))
    assert err <= 5e-5
    # the entries that reach past the last frame are 0.0, and only those were left unwritten
    out_of_range = torch.ones(G * (T0 - 1), dtype=torch.bool, device="cuda")
    out_of_range[at] = False
    assert int(out_of_range.sum()) == G * (T0 - 1) - len(pairs) == sum(range(G))
    assert torch.count_nonzero(table.view(-1)[out_of_range]) == 0
    for k in (2, G):
        assert torch.count_nonzero(table[k - 1, T0 - k:]) == 0 and table[k - 1, T0 - k:].numel() == k - 1
    # row 0 is the a5 launch of the lossless path over all frames
    assert torch.equal(table[0], enc.sims_tensor(rows, T0))
    with pytest.raises(ValueError):
        enc.gap_sims_tensor(rows, T0, T0)
    with pytest.raises(ValueError):
        enc.gap_sims_tensor(rows, T0, 0)


# ------------------------------------------------------------------------------------------------ 2. export routes
def test_export_routes_give_one_set(fx):
    enc = fx["enc"]
    H, W = 90, 160
    frames = frames_of(H, W)
    ps, pd = reference_pixels(frames)
    a = enc.export_features(ps, pd, (H, W), store="e4m3", gaps="auto")
    b = enc.compact_features(enc.export_features(ps, pd, (H, W)), gaps="auto")
    c = enc.export_features_from_frames(frames, store="e4m3", slab=16, gaps="auto")
    assert a.gaps == 2 and tuple(a.gap_sims.shape) == (2, 39) and a.gap_sims.is_cuda and a.gap_sims.dtype == torch.float32
    assert sorted(a.tensors()) == ["dino", "dino_scale", "gap_sims", "siglip", "siglip_scale", "sims"]
    for other in (b, c):
        assert sorted(other.tensors()) == sorted(a.tensors()) and other.signature == a.signature
        for k, t in a.tensors().items():
            assert torch.equal(getattr(other, k), t), k
    assert torch.equal(a.gap_sims[0], a.sims) and float(a.gap_sims[1, 38]) == 0.0
    plain = enc.export_features(ps, pd, (H, W), store="e4m3")
    assert a.nbytes == plain.nbytes + 4 * 2 * 39 and plain.gap_sims is None
    for k, t in plain.tensors().items():
        assert torch.equal(getattr(a, k), t), k
    with pytest.raises(ValueError, match="gaps"):
        enc.export_features(ps[:2], pd[:2], (H, W), gaps="auto")
    with pytest.raises(ValueError, match="gap"):
        enc.compact_features(plain, gaps=2)


# ------------------------------------------------------------------------------------------------ 3. the fix
def check_tokens(enc, want, got, info):
    c, s = parity(enc, want, got, info)
    print("table set vs lossless, 30 of 40 frames: compressed rows max abs %.3e, static rows max rel %.3e" % (c, s))
    assert c <= TOL_COMP and s <= TOL_STATIC


def test_sub_sampled_selection_comes_from_the_table(fx, tmp_path):
    enc, fs, cs, pid = fx["enc"], fx["fs"], fx["cs"], fx["pid"]
    assert cs.gaps == 2
    wi, gi = {}, {}
    want = enc.encode_features(fs, 9, 8, pid, frame_cap=30, info=wi)
    launches, restore = count_sims(enc)
    try:
        got = enc.encode_features(cs, 9, 8, pid, frame_cap=30, info=gi)
        assert launches == [], "a5 was launched on a set that holds the similarities"
        assert gi.pop("selection_sims") == "stored" and "selection_sims" not in wi
        assert gi["seg_indices"] == wi["seg_indices"] and len(gi["seg_indices"]) == 24
        assert gi["frame_indices"] == wi["frame_indices"] == fx["idx"] and gi == wi
        assert got.shape == want.shape and got.dtype == want.dtype
        check_tokens(enc, want, got, gi)
        # the table's entries ARE the lossless path's similarities of the kept frames
        from tdc_video_amd import encode, features
        lossless = enc.sims_tensor(encode.feature_rows(enc, fs, fx["idx"])[1], 30).tolist()
        del launches[:]
        assert features.stored_sims(cs, fx["idx"]) == lossless
        # three prompts share the one front
        qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid),
              dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:]),
              dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid[1:4] + pid[-1:])]
        infos = [{} for _ in qs]
        many = enc.encode_features_prompts(cs, qs, frame_cap=30, infos=infos, pad_fraction=1.0)
        assert torch.equal(many[0], got)
        for p, q in enumerate(qs):
            li, si = {}, {}
            ref = enc.encode_features(fs, q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"], frame_cap=30, info=li)
            one = enc.encode_features(cs, q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"], frame_cap=30, info=si)
            assert torch.equal(many[p], one), p
            assert {k: v for k, v in infos[p].items() if k != "prompts"} == si and si.pop("selection_sims") == "stored"
            assert si == li and many[p].shape == ref.shape
            c, s = parity(enc, ref, many[p], si, q["n_text_tokens"])
            assert c <= TOL_COMP and s <= TOL_STATIC
        assert launches == [30] * 3, "only the lossless reference calls launch a5"
        # saved as format 3, loaded, pinned, uploaded by the call
        del launches[:]
        path = str(tmp_path / "v.tdcfeat")
        cs.save(path)
        assert torch.load(path, weights_only=True)["format"] == 3
        host = type(cs).load(path).cpu()
        assert host.gaps == 2 and all(t.is_pinned() for t in host.tensors().values()) and host.nbytes == cs.nbytes
        hi = {}
        assert torch.equal(enc.encode_features(host, 9, 8, pid, frame_cap=30, info=hi), got)
        assert hi.pop("selection_sims") == "stored" and hi == wi and launches == []
        back = host.to(enc.dev)
        for k, t in cs.tensors().items():
            assert torch.equal(getattr(back, k), t) and getattr(back, k).is_cuda, k
    finally:
        restore()


# ------------------------------------------------------------------------------------------------ 4. without the table
def test_default_compact_set_still_selects_on_the_decoded_rows(fx):
    enc, plain, pid = fx["enc"], fx["plain"], fx["pid"]
    assert plain.gap_sims is None and plain.gaps == 1
    launches, restore = count_sims(enc)
    try:
        gi = {}
        enc.encode_features(plain, 9, 8, pid, frame_cap=30, info=gi)
        assert launches == [30] and gi["selection_sims"] == "decoded"
        del launches[:]
        ai = {}
        enc.encode_features(plain, 9, 8, pid, info=ai)                 # every frame kept: the stored similarities, as before
        assert launches == [] and ai["selection_sims"] == "stored"
    finally:
        restore()
