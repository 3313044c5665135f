"""GPU (-m gpu): encode from stored tower features (features.FeatureSet) on the tiny reference-fixture
model (towers 48 / 64 wide: the SigLIP rows carry padding columns the stored form drops and the encode restores).  Every
comparison is torch.equal against the pixel path: the feature path launches the pixel path's a5, connector and Q-Former
kernels on the same operands.  The engine runs fp16 DINOv2 operands, so the pixel path refines nothing."""
import numpy as np
import pytest
import torch

import synth
from test_hip_boundary import loaded_lm
from test_hip_pipeline import make_encoder
from util import load_fixture, pipeline_cfg

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y)
        else:
            assert x == y


def _load(name):
    W, o = load_fixture(name)
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    return dict(W=W, o=o, vs=vid.cuda(), vd=(vid + 0.01).cuda(), vid=vid, pid=[int(i) for i in o["prompt_ids"]],
                size=tuple(int(v) for v in o["image_size"]))


@pytest.fixture(scope="module")
def fx():
    """the T = 40 fixture, its engine (refinement off) and the video's exported feature set - made once, never changed"""
    f = _load("pipeline_T40.npz")
    f["enc"] = enc = make_encoder(f["W"], pipeline_cfg(f["o"]), torch.float16)
    assert enc.selection_eps is None
    f["fs"] = enc.export_features(f["vs"], f["vd"], f["size"])
    return f


def test_stored_form(fx):
    enc, fs = fx["enc"], fx["fs"]
    assert tuple(fs.siglip.shape) == (40, 64, 48) and tuple(fs.dino.shape) == (40, 64, 64) and fs.siglip.dtype == enc.dtype
    assert fs.image_size == fx["size"] and fs.signature == enc.feature_signature()
    rows = enc.tower("siglip", fx["vs"])                          # [40 * 64, 64]: 16 padding columns, zeros
    assert torch.equal(fs.siglip, rows[:, :48].reshape(40, 64, 48)) and torch.equal(enc.feature_rows(fs.siglip), rows)
    assert torch.equal(enc.feature_rows(fs.dino), enc.tower("dino", fx["vd"]))


@pytest.mark.parametrize("T0,cap,kept", [(40, 224, 40), (40, 30, 30), (20, 224, 20)])
def test_encode_features_equals_encode_video(fx, T0, cap, kept):
    enc = fx["enc"]
    vs, vd = fx["vs"][:T0], fx["vd"][:T0]
    fs = fx["fs"] if T0 == 40 else enc.export_features(vs, vd, fx["size"])
    wi, gi = {}, {}
    want = enc.encode_video(vs, vd, fx["size"], 9, 8, fx["pid"], frame_cap=cap, info=wi)
    got = enc.encode_features(fs, 9, 8, fx["pid"], frame_cap=cap, info=gi)
    assert torch.equal(got, want) and gi == wi
    assert len(gi["frame_indices"]) == kept and gi["final_size"] == wi["final_size"] and gi["seg_indices"] == wi["seg_indices"]
    assert gi["seg_indices"] == list(range(20)) if T0 == 20 else len(gi["seg_indices"]) == 24


def test_one_image(fx):
    enc = fx["enc"]
    im_s, im_d = fx["vs"][7:8], fx["vd"][7:8]
    size = (360, 640)
    X, sizes = enc.connector(enc.tower("siglip", im_s), enc.tower("dino", im_d), 1, [size])
    info = {}
    got = enc.encode_features(enc.export_features(im_s, im_d, size), None, 8, None, image=True, info=info)
    assert torch.equal(got, X[:, :enc.H]) and info == {"final_size": sizes}


def test_audio():
    f = _load("pipeline_T40_audio.npz")
    enc = make_encoder(f["W"], pipeline_cfg(f["o"]), torch.float16)
    wins = synth.beats_windows(torch.from_numpy(f["o"]["audio_wav"].astype(np.float32)))
    fs = enc.export_features(f["vs"], f["vd"], f["size"])
    for cap in (224, 33):
        wi, gi = {}, {}
        want = enc.encode_video(f["vs"], f["vd"], f["size"], 9, 8, f["pid"], audio={"beats_windows": wins}, frame_cap=cap, info=wi)
        got = enc.encode_features(fs, 9, 8, f["pid"], audio={"beats_windows": wins}, frame_cap=cap, info=gi)
        assert torch.equal(got, want) and gi == wi


def test_pinned_host_and_back(fx, tmp_path):
    enc, fs = fx["enc"], fx["fs"]
    want = enc.encode_features(fs, 9, 8, fx["pid"], frame_cap=30)
    host = fs.cpu()
    assert host.siglip.is_pinned() and host.dino.is_pinned() and not host.siglip.is_cuda and host.nbytes == fs.nbytes
    assert torch.equal(enc.encode_features(host, 9, 8, fx["pid"], frame_cap=30), want)         # uploaded by the call
    back = host.to(enc.dev)
    assert back.siglip.is_cuda and torch.equal(back.siglip, fs.siglip) and torch.equal(back.dino, fs.dino)
    assert torch.equal(enc.encode_features(back, 9, 8, fx["pid"], frame_cap=30), want)
    path = str(tmp_path / "v.tdcfeat")
    fs.save(path)
    assert torch.equal(enc.encode_features(type(fs).load(path), 9, 8, fx["pid"], frame_cap=30), want)


def test_encode_features_prompts_equals_per_prompt_calls(fx):
    enc, fs, pid = fx["enc"], fx["fs"], fx["pid"]
    qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid),
          dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:]),
          dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid[1:4] + pid[-1:])]
    infos = [{} for _ in qs]
    got = enc.encode_features_prompts(fs, qs, infos=infos, pad_fraction=1.0)
    assert [i["prompts"]["group_size"] for i in infos] == [3, 3, 3]
    for p, q in enumerate(qs):
        wi = {}
        want = enc.encode_features(fs, q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"], info=wi)
        assert torch.equal(got[p], want), p
        assert {k: v for k, v in infos[p].items() if k != "prompts"} == wi
        assert torch.equal(want, enc.encode_video(fx["vs"], fx["vd"], fx["size"], 9, q["n_text_tokens"], q["prompt_ids"]))


def test_export_on_two_streams_gives_the_same_bits(fx):
    enc, fs = fx["enc"], fx["fs"]
    old = enc.two_streams
    try:
        for two in (True, False):
            enc.two_streams = two
            again = enc.export_features(fx["vs"], fx["vd"], fx["size"])
            torch.cuda.synchronize()
            assert torch.equal(again.siglip, fs.siglip) and torch.equal(again.dino, fs.dino) and again.signature == fs.signature
    finally:
        enc.two_streams = old


def test_signature_refuses_other_towers(fx):
    """one element of one tower weight changed: another signature, and the set is refused before any launch"""
    W = dict(fx["W"])
    k = "vision_tower_aux_list.1.vision_tower.encoder.layer.0.mlp.weights_out.bias"
    W[k] = W[k].clone()
    W[k][3] += 0.25
    other = make_encoder(W, pipeline_cfg(fx["o"]), torch.float16)
    assert other.feature_signature() != fx["fs"].signature
    with pytest.raises(ValueError) as ei:
        other.encode_features(fx["fs"], 9, 8, fx["pid"])
    assert fx["fs"].signature in str(ei.value) and other.feature_signature() in str(ei.value)
    got = other.encode_features(fx["fs"], 9, 8, fx["pid"], check_signature=False)
    assert torch.equal(got, fx["enc"].encode_features(fx["fs"], 9, 8, fx["pid"]))          # behind the towers they are equal


# ------------------------------------------------------------------------------------------------------------- the mixin
def _call(lm, ids, images, size, prompts, n=1):
    ids = ids.repeat(n, 1)
    pos = torch.arange(ids.shape[1])[None].repeat(n, 1)
    return lm.prepare_inputs_labels_for_multimodal(ids, pos, torch.ones_like(ids), None, ids.clone(), images,
                                                   image_sizes=[size] * n, video_indices=[None] * n, prompts=prompts,
                                                   audios=[None] * n)


def test_mixin_feature_inputs_equal_the_pixel_call(fx):
    lm = loaded_lm(fx["W"], fx["o"])
    ids = torch.from_numpy(fx["o"]["input_ids"])
    vid = fx["vid"]
    want = _call(lm, ids, [[vid], [vid + 0.01]], fx["size"], [fx["pid"]])
    eng = lm.get_model().tdc_engine()
    assert eng.selection_eps is None
    fs = eng.export_features(vid, vid + 0.01, fx["size"])
    lm.get_model().config.tdc_feature_inputs = True
    towers = []
    tower = eng.tower
    eng.tower = lambda name, px: towers.append(name) or tower(name, px)
    _same(_call(lm, ids, [[fs.siglip], [fs.dino]], fx["size"], [fx["pid"]]), want)               # the tensor-pair form
    _same(_call(lm, ids, [[fs], [None]], fx["size"], [fx["pid"]]), want)                         # the FeatureSet form
    _same(_call(lm, ids, [[fs.cpu()], [None]], fx["size"], [fx["pid"]]), want)                   # from pinned host memory
    assert towers == []
    with pytest.raises(ValueError, match="tdc_feature_inputs"):
        _call(lm, ids, [[fs.dino], [fs.dino]], fx["size"], [fx["pid"]])                          # 64 wide where SigLIP is 48


def test_mixin_batch_prompts_over_one_feature_set(fx):
    lm = loaded_lm(fx["W"], fx["o"], tdc_feature_inputs=True)
    ids = torch.from_numpy(fx["o"]["input_ids"])
    eng = lm.get_model().tdc_engine()
    fs = eng.export_features(fx["vid"], fx["vid"] + 0.01, fx["size"])
    pid = fx["pid"]
    prompts = [pid, pid[:5] + pid[-1:], pid[1:4] + pid[-1:]]
    # the same video as the same set, as equal tensors in another allocation, and as the bare tensor pair
    images = [[fs, type(fs)(fs.siglip.clone(), fs.dino.clone(), fs.image_size, fs.signature), fs.siglip], [None, None, fs.dino]]
    off = _call(lm, ids, images, fx["size"], prompts, 3)
    for i in range(3):                                                                           # each row: its single call
        one = _call(lm, ids, [[fs], [None]], fx["size"], [prompts[i]])
        assert torch.equal(off[4][i, :one[4].shape[1]], one[4][0])
    lm.get_model().config.tdc_batch_prompts = 4
    lm.get_model().config.tdc_prompt_pad_fraction = 1.0
    seen = []
    multi = eng.encode_features_prompts
    eng.encode_features_prompts = lambda fs_, qs, **kw: seen.append(len(qs)) or multi(fs_, qs, **kw)
    _same(_call(lm, ids, images, fx["size"], prompts, 3), off)
    assert seen == [3]
