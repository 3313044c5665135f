"""Pins oracle/tdc_oracle.py to the reference: every stage against fixtures produced by running the reference
(tests/golden/make_golden.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

import synth
from util import GOLDEN, oracle, load_fixture, embed_fn, pipeline_cfg

ATOL = 2e-5


def close(a, b, atol=ATOL):
    a = torch.as_tensor(a, dtype=torch.float32)
    b = torch.as_tensor(b, dtype=torch.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())  # fp32 round-off grows with magnitude
    assert err <= atol * scale, (err, scale)


def test_bilinear_bicubic_matrices_match_torch():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    for n_in, n_out in [(27, 24), (9, 8), (6, 8), (37, 27), (5, 9)]:
        x = torch.randn(2, 3, n_in, n_in, generator=g)
        tok = x.permute(0, 2, 3, 1).reshape(2, n_in * n_in, 3)
        ref = F.interpolate(x, size=(n_out, n_out), mode="bilinear", align_corners=False)
        close(oracle.resize_tokens(tok, n_out), ref.permute(0, 2, 3, 1).reshape(2, -1, 3), 3e-5)
        ref = F.interpolate(x, size=(n_out, n_out), mode="bicubic", align_corners=False)
        close(oracle.resize_tokens(tok, n_out, oracle.bicubic_matrix), ref.permute(0, 2, 3, 1).reshape(2, -1, 3), 3e-5)


def test_adaptive_pool_matches_torch():
    import torch.nn.functional as F
    x = torch.randn(156, 7)
    for K in (16, 144, 5):
        ref = F.adaptive_avg_pool1d(x.t()[None], K)[0].t()
        close(oracle.adaptive_avg_pool_tokens(x, K), ref, 1e-6)


def test_siglip_tower():
    W, o = load_fixture("siglip_small.npz")
    out, pre = oracle.siglip_tower(torch.from_numpy(o["pixels"]), W, heads=4, interp_tokens=64)
    close(pre, o["out_pre_interp"])
    close(out, o["out"])


def test_dino_tower():
    W, o = load_fixture("dino_small.npz")
    out, pre = oracle.dino_tower(torch.from_numpy(o["pixels"]), W, heads=4, interp_tokens=64)
    close(pre, o["out_pre_interp"])
    close(out, o["out"])


def test_sva_and_masks():
    W, o = load_fixture("sva_small.npz")
    aux = [torch.from_numpy(o["aux0"]), torch.from_numpy(o["aux1"])]
    sizes = [tuple(int(v) for v in s) for s in o["image_sizes"]]
    out, masks = oracle.sva(aux, torch.from_numpy(o["vision_query"])[0], sizes, W, side=4)
    assert np.array_equal(masks[0].numpy(), o["out_mask0"])
    assert np.array_equal(masks[1].numpy(), o["out_mask1"])
    assert not o["out_mask0"].all()  # the fixture really exercises padding masks
    close(out, o["out"])


def test_qformer_chunk():
    W, o = load_fixture("qformer_small.npz")
    chunk = torch.from_numpy(o["chunk"])
    K = int(o["K"])
    ids = torch.from_numpy(o["prompt_ids"])
    q = oracle._lin(oracle.adaptive_avg_pool_tokens(chunk[0], K), W, "query_proj")
    close(q, o["out_query_tokens"])
    L = chunk.shape[0] - 1
    last = oracle.qformer_bert(q[None].expand(L, -1, -1), chunk[1:], ids, W, heads=4)
    close(last, o["out_last_hidden"])
    close(oracle.qformer_bert(q[None].expand(L, -1, -1), chunk[1:], None, W, heads=4), o["out_last_hidden_notext"])
    comp, _ = oracle.compress_chunk(chunk, ids, W, K, heads=4)
    close(comp, o["out_compressed"])


def _run_pipeline(name):
    W, o = load_fixture(name)
    cfg = pipeline_cfg(o)
    W["embed_tokens_fn"] = embed_fn(o)
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    r = oracle.encode_video(W, cfg, vid, vid + 0.01, tuple(int(v) for v in o["image_size"]),
                            torch.from_numpy(o["input_ids"]), torch.from_numpy(o["prompt_ids"]))
    return r, o


@pytest.mark.parametrize("name,stride", [("pipeline_T40.npz", 1), ("pipeline_T10_land.npz", 1),
                                         ("pipeline_T260.npz", 16)])
def test_full_pipeline(name, stride):
    r, o = _run_pipeline(name)
    # integers: bit-exact
    assert np.array_equal(r["seg_indices"].numpy(), o["out_seg_indices"])
    assert np.array_equal(r["selected"].numpy(), o["out_selected"])
    assert [list(s) for s in r["final_size"]] == o["out_final_size"].tolist()
    # stages
    close(r["siglip_feat"][::stride], o["out_siglip_feat"])
    close(r["dino_feat"][::stride], o["out_dino_feat"])
    close(r["aux0"][::stride], o["out_aux0"])
    close(r["aux1"][::stride], o["out_aux1"])
    nq = r["sva"].shape[1]
    close(r["sva"][::stride], torch.from_numpy(o["out_sva"]).reshape(-1, nq, r["sva"].shape[2]))
    close(r["mm_proj"][::stride], o["out_mm_proj"])
    close(r["inputs_embeds"], o["out_inputs_embeds"])


@pytest.mark.parametrize("name", ["pipeline_T40_nostatic.npz", "pipeline_T40_learned.npz"])
def test_pipeline_config_ablations(name):
    """add_static=False (every frame compressed, no static tokens) and query_type='learned' (query_tokens), generated
    from the reference with those config values (tdc/cambrian_arch.py:1509-1511,1625-1640,1668-1692)."""
    r, o = _run_pipeline(name)
    assert np.array_equal(r["seg_indices"].numpy(), o["out_seg_indices"])
    close(r["inputs_embeds"], o["out_inputs_embeds"])
    if "nostatic" in name:
        n_text = o["input_ids"].shape[1] - 1
        assert r["inputs_embeds"].shape[1] == n_text + 40 * (4 + 1)


def test_pipeline_token_accounting():
    """T=40 -> static frames emit N+1 tokens, compressed frames K+1."""
    r, o = _run_pipeline("pipeline_T40.npz")
    chunks = oracle.chunk_table(40, r["seg_indices"])
    n_static = len(chunks)
    n_comp = 40 - n_static
    N = 4 * 5  # 4x4 tokens + newline column
    assert r["visual_tokens"].shape[0] == n_static * (N + 1) + n_comp * (4 + 1)
    assert int(o["n_qformer_calls"]) == sum(1 for s, e in chunks if e - s > 1)


def test_full_pipeline_audio():
    """a20: audio tokens interleaved into the Q-Former KV (N+50) and into the static frames (fake BEATs features)."""
    W, o = load_fixture("pipeline_T40_audio.npz")
    cfg = pipeline_cfg(o)
    assert cfg["audio_input"]
    W["embed_tokens_fn"] = embed_fn(o)
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    wins = synth.beats_windows(torch.from_numpy(o["audio_wav"].astype(np.float32)))
    assert [w.shape[1] for w in wins] == [496] * 4
    r = oracle.encode_video(W, cfg, vid, vid + 0.01, tuple(int(v) for v in o["image_size"]),
                            torch.from_numpy(o["input_ids"]), torch.from_numpy(o["prompt_ids"]), beats_windows=wins)
    assert np.array_equal(r["seg_indices"].numpy(), o["out_seg_indices"])
    close(r["inputs_embeds"], o["out_inputs_embeds"])
    # static frames carry N + 50 + 1 tokens, compressed ones K + 1
    chunks = oracle.chunk_table(40, r["seg_indices"])
    assert r["visual_tokens"].shape[0] == len(chunks) * (20 + 50 + 1) + (40 - len(chunks)) * 5


def test_audio_tokens_with_dropped_frames():
    """seconds dropped by the frame cap are pooled into the preceding kept second (cambrian_arch.py:1570-1589)."""
    g = torch.Generator().manual_seed(0)
    wins = [torch.randn(1, 496, 8, generator=g), torch.randn(1, 300, 8, generator=g)]   # 10 s + 6 s
    samp = torch.tensor([1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 1, 0, 1, 1])
    out = oracle.audio_tokens(wins, samp, int(samp.sum()))
    assert out.shape == (int(samp.sum()), 50, 8)
    close(out[0], wins[0][0, :50])                                              # kept, next kept -> verbatim
    close(out[1], torch.nn.functional.adaptive_avg_pool2d(wins[0][:, 50:200], (50, 8))[0])   # 1 kept + 2 dropped
    close(out[2], torch.nn.functional.adaptive_avg_pool2d(wins[0][:, 200:300], (50, 8))[0])


# ---- full model dimensions: the oracle against digests of the reference's outputs (tests/golden/make_golden_fulldim.py) -----
# Weights and inputs are rebuilt from synth.fill's hash; the fixtures hold only digests (synth.digest).  Each fixture also has
# a sensitivity test: one host-side perturbation of the weights or arguments, of the kind of bug the digests are meant for,
# must fail the same comparison.
FULLDIM_TOL = 2e-5
FULLDIM_LAYERS = (4, 4)


def test_synth_fill_literal_values():
    """synth.fill is integer hashing only; these bits must not move with a numpy upgrade (the fixtures depend on them)."""
    assert synth.name_hash("probe") == 17975714548341171953
    assert synth.fill("probe", (8,), "pixels").tolist() == [
        -0.5088361501693726, -0.959699273109436, 0.4637244939804077, 0.5194743871688843, -0.9659587144851685,
        0.4994715452194214, -0.7230956554412842, -0.28796398639678955]
    u = synth.fill("vision_tower_aux_list.0.vision_tower.encoder.layers.0.mlp.fc1.weight", (4304, 1152))    # linear
    assert u[0, :3].tolist() == [-0.04016349837183952, 0.004593810997903347, -0.04890754446387291]
    assert u[-1, -2:].tolist() == [0.02125607430934906, 0.023045578971505165]
    assert u.reshape(-1)[(1 << 22) + 5] == np.float32(-0.03494581952691078)          # second chunk of the hash
    assert synth.fill("vision_tower_aux_list.1.vision_tower.encoder.layer.3.layer_scale2.lambda1", (1536,))[:2].tolist() == [
        0.729943573474884, 0.8447016477584839]


@pytest.fixture(scope="module")
def fulldim_sd():
    sd = synth.synth_state_dict(*FULLDIM_LAYERS, prefixes=("vision_tower_aux_list.", "vision_sampler_0.", "vision_query",
                                                             "Qformer.", "query_proj.", "vision_proj."))
    return sd, oracle.sub(sd, "vision_tower_aux_list.0.vision_tower."), oracle.sub(sd, "vision_tower_aux_list.1.vision_tower.")


def fulldim_errors(name, key, x):
    z = np.load(os.path.join(GOLDEN, name))
    return synth.digest_errors(synth.load_digest(z, key), torch.as_tensor(x).double().numpy())


def assert_fulldim(name, key, x, tol=FULLDIM_TOL):
    e = fulldim_errors(name, key, x)
    print("%s %s: %s" % (name, key, " ".join("%s %.2e" % kv for kv in e.items())))
    assert max(e.values()) <= tol, e
    return e


def assert_fulldim_fails(name, key, x, tol=FULLDIM_TOL):
    e = fulldim_errors(name, key, x)
    worst = max(e, key=e.get)
    print("%s %s perturbed: fails by %.0fx on %s (%s)" % (name, key, e[worst] / tol, worst,
                                                          " ".join("%s %.2e" % kv for kv in e.items())))
    assert e[worst] > 10 * tol, e


def fulldim_siglip(Ws):
    return oracle.siglip_tower(synth.synth_input("pixels/siglip", (2, 3, 384, 384)), Ws, heads=16)


def test_fulldim_siglip(fulldim_sd):
    """1152 wide, 16 heads of 72, MLP 4304, 27^2 patches -> 24^2 (4 layers, 2 frames)."""
    out, pre = fulldim_siglip(fulldim_sd[1])
    assert_fulldim("fulldim_siglip.npz", "out_pre_interp", pre)
    assert_fulldim("fulldim_siglip.npz", "out", out)


def test_fulldim_siglip_sensitivity(fulldim_sd):
    """heads 3 and 11 of the last layer's V projection swapped"""
    W = dict(fulldim_sd[1])
    for n in ("weight", "bias"):
        k = "encoder.layers.3.self_attn.v_proj." + n
        w = W[k].clone()
        w[3 * 72:4 * 72], w[11 * 72:12 * 72] = W[k][11 * 72:12 * 72], W[k][3 * 72:4 * 72]
        W[k] = w
    assert_fulldim_fails("fulldim_siglip.npz", "out", fulldim_siglip(W)[0])


def fulldim_dino(Wd):
    return oracle.dino_tower(synth.synth_input("pixels/dino", (2, 3, 378, 378)), Wd, heads=24)


def test_fulldim_dino(fulldim_sd):
    """1536 wide, 24 heads, SwiGLU 4096, LayerScale, position table 37^2 -> 27^2 (bicubic), tokens 27^2 -> 24^2 (4 layers)."""
    out, pre = fulldim_dino(fulldim_sd[2])
    assert_fulldim("fulldim_dino.npz", "out_pre_interp", pre)
    assert_fulldim("fulldim_dino.npz", "out", out)


def test_fulldim_dino_sensitivity(fulldim_sd):
    """the 37 x 37 position grid shifted by one column"""
    W = dict(fulldim_sd[2])
    pos = W["embeddings.position_embeddings"]
    grid = pos[:, 1:].reshape(1, 37, 37, -1)
    W["embeddings.position_embeddings"] = torch.cat([pos[:, :1], torch.roll(grid, 1, dims=2).reshape(1, 37 * 37, -1)], 1)
    assert_fulldim_fails("fulldim_dino.npz", "out", fulldim_dino(W)[0])


def fulldim_sva(sd, size):
    aux = [synth.synth_input("features/sva_aux%d" % i, (3, 576, 1024)) for i in range(2)]
    return oracle.sva(aux, sd["vision_query"][0], [size] * 3, sd, side=12)


@pytest.mark.parametrize("tag,size", [("square", (384, 384)), ("wide", (360, 640))])
def test_fulldim_sva(fulldim_sd, tag, size):
    """C = 1024, 3 layers, 12 x 12 windows of 2 x 2 keys per tower; (360, 640): the window masks of a 16:9 frame."""
    out, masks = fulldim_sva(fulldim_sd[0], size)
    z = np.load(os.path.join(GOLDEN, "fulldim_sva.npz"))
    for i in range(2):
        assert np.array_equal(masks[i].numpy(), z["mask%d_%s" % (i, tag)])
    assert z["mask0_" + tag].all() == (tag == "square")
    assert_fulldim("fulldim_sva.npz", "out_" + tag, out)


def test_fulldim_sva_sensitivity(fulldim_sd, monkeypatch):
    """the last valid key of every partly masked window of the 16:9 frame dropped"""
    wm = oracle.window_masks

    def short(side, reduce, image_size):
        m = wm(side, reduce, image_size)
        for row in m:
            if not row.all():
                row[int(torch.nonzero(row)[-1])] = False
        return m
    monkeypatch.setattr(oracle, "window_masks", short)
    assert_fulldim_fails("fulldim_sva.npz", "out_wide", fulldim_sva(fulldim_sd[0], (360, 640))[0])


def fulldim_qformer(sd, K, N, queries=None):
    z = np.load(os.path.join(GOLDEN, "fulldim_qformer.npz"))
    chunk = synth.synth_input("features/qformer_N%d" % N, (8, N, 3584))
    ids = torch.from_numpy(z["prompt_ids"])
    if queries is None:
        return oracle.compress_chunk(chunk, ids, sd, K, heads=12)[0]
    last = oracle.qformer_bert(queries(chunk[0])[None].expand(7, -1, -1), chunk[1:], ids, sd, heads=12)
    return torch.nn.functional.normalize(oracle._lin(last[:, :K], sd, "vision_proj"), dim=-1)


@pytest.mark.parametrize("K,N", [(144, 156), (16, 156), (16, 84)])
def test_fulldim_qformer(fulldim_sd, K, N):
    """one 8-frame chunk: bert-base Q-Former (12 layers, cross-attention to H = 3584 in the even ones), Lt = 12 prompt ids,
    K = 144 / 16 pooling windows over N = 156 (square) or 84 (16:9) tokens of the key frame."""
    assert len(np.load(os.path.join(GOLDEN, "fulldim_qformer.npz"))["prompt_ids"]) == 12
    assert_fulldim("fulldim_qformer.npz", "out_K%d_N%d" % (K, N), fulldim_qformer(fulldim_sd[0], K, N))


def test_fulldim_qformer_sensitivity(fulldim_sd):
    """K = 16 pooling windows (each query repeated 9 times) where K = 144 is expected"""
    sd = fulldim_sd[0]
    q = lambda key: oracle._lin(oracle.adaptive_avg_pool_tokens(key, 16).repeat_interleave(9, 0), sd, "query_proj")
    assert_fulldim_fails("fulldim_qformer.npz", "out_K144_N156", fulldim_qformer(sd, 144, 156, q))
