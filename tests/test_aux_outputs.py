"""CPU: the reference's three aux outputs of the 10-tuple - segment.aux_window_map against the fixture
recorded from the reference (tests/golden/aux_outputs.npz, make_golden_aux.py) and against the oracle's own geometry,
`config.tdc_return_aux` at the boundary on an engine double, the ctypes mirror of the three new fields, and the launch trace
of tdc_connector_fwd with them set (tests/aux_trace/aux_trace.cpp, compared with the plain trace of the same case)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import encode, lib as L, pipeline, segment as seg
from test_dist_gloo import make_video
from test_features import FeatureMixinEngine, feature_lm
from util import GOLDEN, oracle

CASES = ("T40", "T10_land", "T10_480x640")
SIDE, R = 4, 2                                    # the reduced fixtures' grid: 16 queries over 8 x 8 aux tokens


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "aux_outputs.npz"), allow_pickle=False)
    return {c: {k.split("::", 1)[1]: z[k] for k in z.files if k.startswith(c + "::")} for c in CASES}


# ------------------------------------------------------------------------------------------------- host geometry
@pytest.mark.parametrize("case", CASES)
def test_window_map_equals_the_reference(fixture, case):
    f = fixture[case]
    size = tuple(int(v) for v in f["image_size"])
    src, mask, hw = seg.aux_window_map(SIDE, R, size)
    T, P = f["final_size"].shape[0], (SIDE * R) ** 2
    n = hw[0] * hw[1]
    assert src.shape == mask.shape == (n, R * R) and mask.dtype == np.bool_
    assert [tuple(v) for v in f["final_size"].tolist()] == [hw] * T
    want_src = np.concatenate([src + t * P for t in range(T)], 0)
    for i in range(2):
        assert np.array_equal(f["feat_src%d" % i], want_src), i
        assert np.array_equal(f["mask%d" % i], np.concatenate([mask] * T, 0)), i
    assert np.array_equal(f["ctx_src"], np.repeat(np.arange(T), n))
    if case == "T10_480x640":                     # the case the masks are there for
        assert (~mask.all(-1)).sum() == 8 and mask.any(-1).all()


def oracle_composition(side, r, size):
    """the oracle's rearrange_windows, window_masks and unpad_bounds as they are, composed as the reference composes its own
    (cambrian_arch.py:624-669): windows, cut of the window grid, masks of the kept windows"""
    P = (side * r) ** 2
    win = oracle.rearrange_windows(torch.arange(P).view(1, P, 1), side)[:, :, 0].view(side, side, r * r)
    masks = oracle.window_masks(side, r, size).view(side, side, r * r)
    r0, r1, c0, c1 = oracle.unpad_bounds(side, side, size)
    return (win[r0:r1, c0:c1].reshape(-1, r * r).numpy(), masks[r0:r1, c0:c1].reshape(-1, r * r).numpy(),
            (max(r1 - r0, 0), max(c1 - c0, 0)))


SWEEP = [(s, s) for s in (1, 126, 384, 1000)] + [(480, 640), (300, 400), (360, 640), (200, 640), (90, 640), (378, 384), (100, 101)]
SWEEP += [(w, h) for h, w in SWEEP if h != w]


@pytest.mark.parametrize("side,r", [(4, 2), (12, 2)])
def test_window_map_equals_the_oracle_composition(side, r):
    ran, masked = 0, 0
    for size in SWEEP:
        want_src, want_mask, want_hw = oracle_composition(side, r, size)
        if want_hw[0] * want_hw[1] == 0:          # un-padding keeps no window: out of scope (behaves as final_size does)
            continue
        src, mask, hw = seg.aux_window_map(side, r, size)
        assert hw == want_hw, size
        assert np.array_equal(src, want_src) and np.array_equal(mask, want_mask), size
        assert src.min() >= 0 and src.max() < (side * r) ** 2
        ran += 1
        masked += int((~mask.all(-1)).any())
    assert ran >= 16 and masked >= 2
    counts = {(4, 2): (16, 8), (12, 2): (120, 24)}[(side, r)]      # (480, 640): windows kept, windows with masked entries
    src, mask, hw = seg.aux_window_map(side, r, (480, 640))
    assert (src.shape[0], int((~mask.all(-1)).sum())) == counts


# ------------------------------------------------------------------------------------------------- the boundary
class AuxEngine(FeatureMixinEngine):
    """the double with the aux= argument: its three outputs are arithmetic of the frames' rows and sizes, so sample order and
    the frames of a sample can be read off them; records how `connector` was called"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.connector_kw = []

    def connector(self, sig, dino, T, sizes, keep=None, **kw):
        self.connector_kw.append(sorted(kw))
        X, fsz = super().connector(sig, dino, T, sizes, keep)
        if "aux" in kw:
            n = [int(s[0]) // 100 for s in sizes]                 # "windows" of a frame: a function of its size
            rows = torch.cat([sig.reshape(T, self.P, self.H)[t, :1].expand(n[t], -1) for t in range(T)], 0)
            tag = torch.cat([torch.full((n[t],), float(sizes[t][1])) for t in range(T)], 0)
            kw["aux"].update(features=[rows[:, None, :].expand(-1, 4, -1).contiguous(), (rows * 2)[:, None, :].expand(-1, 4, -1).contiguous()],
                             masks=[tag[:, None].expand(-1, 4) > 500, tag[:, None].expand(-1, 4) > 0],
                             global_context=tag[:, None, None] + rows[:, None, :])
        return X, fsz

    def encode_video(self, *a, **kw):
        return pipeline.encode_video_with(self, *a, **kw)


def call(lm, images, sizes, prompts=None):
    n = len(sizes)
    ids = torch.tensor([[11, 12, -200, 13, 14, 15]] * n)
    with torch.inference_mode():
        return lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, images, image_sizes=list(sizes),
                                                       video_indices=[None] * n, prompts=prompts or [[1, 2]] * n,
                                                       audios=[None] * n)


def same_but_aux(on, off):
    assert len(on) == len(off) == 10
    for i, (x, y) in enumerate(zip(on, off)):
        if i in (6, 7, 9):
            continue
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y), i
        else:
            assert x == y, i


def test_key_off_leaves_the_slots_none_and_passes_no_aux():
    for cfg in ({}, {"tdc_return_aux": False}, {"tdc_return_aux": None}):
        lm = feature_lm(**cfg)
        eng = lm.get_model()._tdc_encoder = AuxEngine(K=3, H=8)
        ims = make_video(2)
        out = call(lm, [ims, ims], [(384, 384), (360, 640)])
        assert out[6] is None and out[7] is None and out[9] is None
        out = call(lm, [[make_video(30)], [make_video(30)]], [(384, 384)])
        assert out[6] is None and out[7] is None and out[9] is None
        assert eng.connector_kw == [[], [], []]
    # ... so an engine whose connector predates the argument serves the key-off call
    lm = feature_lm()
    lm.get_model()._tdc_encoder = FeatureMixinEngine(K=3, H=8)
    assert call(lm, [[make_video(30)], [make_video(30)]], [(384, 384)])[9] is None


def test_key_on_fills_the_slots_in_sample_order():
    ims = make_video(2)
    sizes = [(300, 640), (200, 384)]              # 3 and 2 "windows": the samples can be told apart
    lm = feature_lm()
    eng = lm.get_model()._tdc_encoder = AuxEngine(K=3, H=8)
    off = call(lm, [ims, ims], sizes)
    lm.get_model().config.tdc_return_aux = True
    on = call(lm, [ims, ims], sizes)
    same_but_aux(on, off)
    assert eng.connector_kw == [[], [], ["aux"], ["aux"]]
    feats, masks, ctx = on[6], on[7], on[9]
    assert isinstance(feats, list) and isinstance(masks, list) and len(feats) == len(masks) == 2
    assert tuple(feats[0].shape) == (5, 4, 8) and tuple(masks[0].shape) == (5, 4) and tuple(ctx.shape) == (5, 1, 8)
    assert masks[0].dtype == torch.bool and masks[1].dtype == torch.bool
    rows = [eng.tower("siglip", ims[i:i + 1])[0] for i in range(2)]
    want = torch.stack([rows[0]] * 3 + [rows[1]] * 2)
    assert torch.equal(feats[0][:, 0], want) and torch.equal(feats[1][:, 2], want * 2)
    assert masks[0][:, 0].tolist() == [True] * 3 + [False] * 2 and bool(masks[1].all())
    assert torch.equal(ctx[:, 0], want + torch.tensor([640.0] * 3 + [384.0] * 2)[:, None])
    # a video: the frames a1 keeps, in order; two videos: sample order
    vids = [make_video(30), make_video(26) + 1.0]
    lm.get_model().config.tdc_return_aux = False
    off = call(lm, [vids, vids], [(300, 300), (200, 200)], [[1, 2], [3, 4, 5]])
    lm.get_model().config.tdc_return_aux = True
    on = call(lm, [vids, vids], [(300, 300), (200, 200)], [[1, 2], [3, 4, 5]])
    same_but_aux(on, off)
    want = torch.cat([eng.tower("siglip", vids[0]).reshape(30, eng.P, 8)[:, 0].repeat_interleave(3, 0),
                      eng.tower("siglip", vids[1]).reshape(26, eng.P, 8)[:, 0].repeat_interleave(2, 0)], 0)
    assert torch.equal(on[6][0][:, 0], want) and tuple(on[9].shape) == (30 * 3 + 26 * 2, 1, 8)


def test_key_on_composes_with_feature_inputs():
    vid = make_video(30)
    lm = feature_lm(tdc_return_aux=True)
    eng = lm.get_model()._tdc_encoder = AuxEngine(K=3, H=8)
    want = call(lm, [[vid], [vid]], [(300, 300)])
    fs = encode.export_features_with(eng, vid, vid, (300, 300))
    lm.get_model().config.tdc_feature_inputs = True
    got = call(lm, [[fs], [None]], [(300, 300)])
    same_but_aux(got, want)
    for i in range(2):
        assert torch.equal(got[6][i], want[6][i]) and torch.equal(got[7][i], want[7][i])
    assert torch.equal(got[9], want[9])


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the engine was touched: %s" % name)


@pytest.mark.parametrize("other,v", [("tdc_video_cache_bytes", 1 << 30), ("tdc_kv_cache_bytes", 1 << 20), ("tdc_shard_frames", True),
                                     ("tdc_shard_cache_bytes", 1 << 30), ("tdc_batch_frames", 512), ("tdc_batch_prompts", 4)])
def test_refused_key_pairs_name_both_keys(other, v):
    cfg = {other: v}
    if other == "tdc_kv_cache_bytes":             # that key alone already needs the frame cache: give it, the pair still raises
        cfg["tdc_video_cache_bytes"] = 1 << 30
    lm = feature_lm(tdc_return_aux=True, **cfg)
    with pytest.raises(ValueError) as ei:
        lm.get_model().tdc_return_aux()
    assert "tdc_return_aux" in str(ei.value) and ("tdc_video_cache_bytes" if other == "tdc_kv_cache_bytes" else other) in str(ei.value)
    lm = feature_lm(tdc_return_aux=True, **{other: v})
    lm.get_model()._tdc_encoder = Untouchable()
    with pytest.raises(ValueError) as ei:
        call(lm, [[make_video(30)], [make_video(30)]], [(384, 384)])
    assert "tdc_return_aux" in str(ei.value) and other in str(ei.value)
    # the other key alone, and the pair with the key off, are what they were
    assert feature_lm(tdc_return_aux=False, **{other: v}).get_model().tdc_return_aux() is False


def test_non_bool_value_names_the_key():
    for bad in (1, 0, "yes", 2.5, [True]):
        lm = feature_lm(tdc_return_aux=bad)
        lm.get_model()._tdc_encoder = Untouchable()
        with pytest.raises(ValueError, match="tdc_return_aux"):
            call(lm, [[make_video(30)], [make_video(30)]], [(384, 384)])
    assert feature_lm(tdc_return_aux=True).get_model().tdc_return_aux() is True


def test_early_return_is_unchanged():
    lm = feature_lm(tdc_return_aux=True)
    lm.get_model()._tdc_encoder = Untouchable()
    ids = torch.tensor([[11]])
    out = lm.prepare_inputs_labels_for_multimodal(ids, None, None, "pkv", None, [make_video(2), make_video(2)], image_sizes=[(1, 1)])
    assert out == (ids, None, None, "pkv", None, None, None, None, None, None)


def test_engine_entries_refuse_aux_with_a_cache():
    eng = AuxEngine(K=3, H=8)
    vid = make_video(30)
    with pytest.raises(ValueError, match="aux=.*cache="):
        pipeline.encode_video_with(eng, vid, vid, (300, 300), 4, 4, [1], cache=object(), aux={})
    with pytest.raises(ValueError, match="aux=.*cache="):
        encode.encode_source(eng, encode.PixelSource(vid[:1], vid[:1], (300, 300), object()), None, 4, None, image=True, aux={})
    with pytest.raises(ValueError, match="dict"):
        pipeline.encode_video_with(eng, vid, vid, (300, 300), 4, 4, [1], aux=[])
    assert eng.connector_kw == []
    d = {}
    a = pipeline.encode_video_with(eng, vid, vid, (300, 300), 4, 4, [1], aux=d)
    assert sorted(d) == ["features", "global_context", "masks"] and eng.connector_kw == [["aux"]]
    assert torch.equal(a, pipeline.encode_video_with(eng, vid, vid, (300, 300), 4, 4, [1]))
    for entry in ("encode_video_prompts", "encode_batch", "encode_features_prompts", "encode_frames_prompts"):
        assert "aux" not in inspect.signature(getattr(pipeline.VideoEncoder, entry)).parameters, entry
    for entry in ("encode_video", "encode_frames", "encode_features", "connector"):
        assert inspect.signature(getattr(pipeline.VideoEncoder, entry)).parameters["aux"].default is None, entry


# ------------------------------------------------------------------------------------------------- the C ABI
def test_ctypes_mirror_ends_with_the_three_fields():
    names = [f[0] for f in L.ConnectorModel._fields_]
    assert names[-3:] == ["mm2", "aux_keep", "ctx_keep"]
    fields = dict(L.ConnectorModel._fields_)
    assert fields["ctx_keep"] is C.c_void_p and C.sizeof(fields["aux_keep"]) == 2 * C.sizeof(C.c_void_p)
    m = L.ConnectorModel()
    assert not m.aux_keep[0] and not m.aux_keep[1] and not m.ctx_keep            # zero: the behaviour before
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "tdc_hip.h")).read()
    body = hdr[:hdr.index("} tdc_connector_model;")]
    assert re.search(r"void\*\s*aux_keep\[2\];\s*void\*\s*ctx_keep;\s*$", body)  # appended behind everything else
    assert not any("aux" in k for k in L.SIGNATURES)                             # no new symbol


def _aux_traces(workdir):
    """builds tests/aux_trace/aux_trace.cpp with api.cpp by the host compiler (as test_api_trace does) -> {case: trace lines}"""
    from test_api_trace import ROOT, _toolchain
    cxx, inc = _toolchain()
    assert cxx, "no host C++ compiler ($CXX, else g++)"
    assert inc, "no ROCm headers (hip/hip_runtime.h declares the one runtime call api.cpp makes)"
    exe = os.path.join(str(workdir), "aux_trace")
    src = [os.path.join(ROOT, "tdc-video_amd", "csrc", "api.cpp"), os.path.join(ROOT, "tests", "aux_trace", "aux_trace.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O0", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-o", exe] + src, capture_output=True,
                       text=True)
    assert r.returncode == 0, "the trace program did not build:\n" + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, timeout=60)
    assert r.returncode == 0, "the trace program failed (%d):\n%s" % (r.returncode, r.stderr.decode()[-2000:])
    cases, cur = {}, None
    for line in r.stdout.decode().splitlines():
        if line.startswith("== "):
            cur = cases.setdefault(line[3:], [])
        else:
            cur.append(line)
    return cases


def _fields(line):
    return dict(t.split("=", 1) for t in line.split()[1:] if "=" in t)


def test_composite_trace_moves_exactly_the_aux_and_ctx_pointers(tmp_path):
    from test_api_trace import _toolchain
    if _toolchain() == (None, None):
        pytest.skip("neither a host C++ compiler nor the ROCm headers")
    cases = _aux_traces(tmp_path)
    for C_ in (96, 128):
        plain, keep = cases["aux C%d plain" % C_], cases["aux C%d keep" % C_]
        assert plain[-1].startswith("-> rc=0") and plain[-1] == keep[-1]         # the same workspace bytes
        assert len(plain) == len(keep)
        # the workspace regions, from the plain trace: the aux LayerNorms' outputs and the token mean's output
        aux_ln = [i for i, l in enumerate(plain) if l.startswith("tdc_layernorm ") and _fields(l)["gamma"].startswith("aux")]
        assert [_fields(plain[i])["gamma"] for i in aux_ln] == ["aux0.ln_g", "aux1.ln_g"]
        ws_aux = [_fields(plain[i])["y16"] for i in aux_ln]
        mean = [i for i, l in enumerate(plain) if l.startswith("tdc_token_mean ")]
        assert len(mean) == 1 and _fields(plain[mean[0]])["x"] == ws_aux[0]
        ws_ctx = _fields(plain[mean[0]])["y"]
        assert ws_aux[0].startswith("ws+") and ws_aux[1].startswith("ws+") and ws_ctx.startswith("ws+") and len({ws_aux[0], ws_aux[1], ws_ctx}) == 3
        moved = {"aux_ln": 0, "mean": 0, "layer_ln": 0, "proj_context": 0}
        for i, (a, b) in enumerate(zip(plain, keep)):
            fa, fb = _fields(a), _fields(b)
            if i in aux_ln:
                assert fb.pop("y16") == "aux_keep%d" % aux_ln.index(i) and fa.pop("y16")
                moved["aux_ln"] += 1
            elif i == mean[0]:
                assert (fb.pop("x"), fb.pop("y")) == ("aux_keep0", "ctx_keep") and fa.pop("x") and fa.pop("y")
                moved["mean"] += 1
            elif a.startswith("tdc_layernorm ") and fa.get("x") in ws_aux:
                assert fb.pop("x") == "aux_keep%d" % ws_aux.index(fa.pop("x")) and fa["gamma"] == "ones_C"
                moved["layer_ln"] += 1
            elif a.startswith("tdc_gemm ") and fa.get("A") == ws_ctx:
                assert fb.pop("A") == "ctx_keep" and fa.pop("A") and fa["W"].endswith("proj_context.w")
                moved["proj_context"] += 1
            assert a.split()[0] == b.split()[0] and fa == fb, (C_, i, a, b)
        assert moved == {"aux_ln": 2, "mean": 1, "layer_ln": 4, "proj_context": 2}   # 2 towers, 2 layers in the tiny model
        # nothing of the kept form names the workspace regions any more, and nothing else names the buffers
        for l in keep[:-1]:
            vals = list(_fields(l).values())
            assert not any(v in (ws_aux[0], ws_aux[1], ws_ctx) for v in vals), l
        assert sum("aux_keep" in l or "ctx_keep" in l for l in keep) == 9
        assert not any("_keep" in l for l in plain)
    refused = [n for n in cases if n.startswith("refused")]
    assert len(refused) == 7
    for name in refused:
        assert cases[name] == ["-> rc=-2 " + cases[name][-1].split(" ", 2)[2]], name      # TDC_E_BADARG, before any launch
