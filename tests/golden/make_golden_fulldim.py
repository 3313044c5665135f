"""Generate tests/golden/fulldim_*.npz: digests of the REFERENCE's outputs at the model's real dimensions.

Run by hand in the build container only:   python tests/golden/make_golden_fulldim.py
The reference is imported (ref_shims.install) and built from configs at full width - SigLIP-so400m (1152, 16 heads of 72,
MLP 4304), DINOv2-giant (1536, 24 heads of 64, SwiGLU 4096, LayerScale, 37^2 position table), the SVA at C = 1024 and the
bert-base Q-Former with H = 3584 projections - with fewer tower layers (4 of 27 / 40) so that fp32 on the host stays cheap.
Weights and inputs are synth.fill's hash values (synth.synth_state_dict: the key set of bench.random_state_dict), loaded with
load_state_dict(strict=True); everything runs in fp32.  Only digests (synth.digest) of the outputs are stored; the tests
rebuild the weights and inputs from the same hash.

Fixtures written:
  fulldim_siglip.npz    SiglipVisionTower._forward, 2 frames of 384 px: 27^2 patch tokens -> 24^2
  fulldim_dino.npz      DinoVisionTower._forward, 2 frames of 378 px: position table 37^2 -> 27^2 (bicubic), tokens 27^2 -> 24^2
  fulldim_sva.npz       VisionTokenSampler (3 layers) after the reference's window rearrange, frames (384, 384) and (360, 640)
  fulldim_qformer.npz   one 8-frame chunk through query_proj / Qformer.bert / vision_proj: K = 144 and 16 at N = 156, K = 16 at N = 84
  manifest_fulldim.json seeds (tensor names), shapes, versions
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402
import synth  # noqa: E402

LAYERS = dict(siglip=4, dino=4)
H, C, DQ = 3584, 1024, 768
BERT_KW = dict(hidden_size=DQ, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=30522,
               max_position_embeddings=512)
PROMPT = "what does the person in the video do next ?"          # [CLS] + 10 words + [SEP]: Lt = 12
QFORMER_CASES = [(144, 156), (16, 156), (16, 84)]                # (K, N): square frames 12 x 13, 16:9 frames 12 x 7
SVA_SIZES = {"square": (384, 384), "wide": (360, 640)}
SVA_T = 3

from transformers import Dinov2Config, SiglipVisionConfig  # noqa: E402

DINO_CFG = Dinov2Config(hidden_size=1536, num_hidden_layers=LAYERS["dino"], num_attention_heads=24, image_size=518,
                        patch_size=14, mlp_ratio=4, use_swiglu_ffn=True, layerscale_value=1.0)
SIGLIP_CFG = SiglipVisionConfig(hidden_size=1152, intermediate_size=4304, num_hidden_layers=LAYERS["siglip"],
                                num_attention_heads=16, image_size=384, patch_size=14)

arch, Q, vs = ref_shims.install(bert_cfg_kwargs=BERT_KW, dino_cfg=DINO_CFG)
from transformers import Dinov2Model, SiglipVisionModel  # noqa: E402

SD = synth.synth_state_dict(LAYERS["siglip"], LAYERS["dino"])


def load_exact(module, prefix, rename=lambda k: k):
    """module.load_state_dict(strict=True) from SD[prefix + rename(k)]; keys the path never reads and SD does not hold
    (SigLIP's post-LN / pooling head, DINOv2's mask_token) get hash values of their own.  Then every parameter and
    persistent buffer is checked to hold exactly what was loaded: none is left at HF init."""
    want = {}
    for k, v in module.state_dict().items():
        if k.endswith("position_ids"):
            want[k] = v                                  # an index buffer, not a weight
            continue
        name = prefix + rename(k)
        want[k] = SD[name] if name in SD else torch.from_numpy(synth.fill(name, v.shape))
        assert tuple(want[k].shape) == tuple(v.shape), (k, want[k].shape, v.shape)
    module.load_state_dict(want, strict=True)
    for k, v in module.state_dict().items():
        assert torch.equal(v, want[k]), k
    return sorted(prefix + rename(k) for k in want if prefix + rename(k) not in SD and not k.endswith("position_ids"))


def save(name, arrs):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrs)
    print("wrote", name, "%.1f KB" % (os.path.getsize(path) / 1024))


def tower_config():
    return types.SimpleNamespace(
        mm_vision_tower_aux_list=["siglip/CLIP-ViT-SO400M-14-384", "facebook/dinov2-giant-res378"],
        mm_vision_tower_aux_token_len_list=[576, 576], mm_vision_select_layer=-2, mm_vision_select_feature="patch",
        unfreeze_mm_vision_tower=False)


def make_towers(man):
    from tdc.multimodal_encoder.builder import build_vision_tower_aux_list
    sig, dino = build_vision_tower_aux_list(tower_config(), delay_load=True)
    sig.vision_tower = SiglipVisionModel(SIGLIP_CFG).eval()
    sig.is_loaded = True
    dino.vision_tower = Dinov2Model(DINO_CFG).eval()
    dino.is_loaded = True
    assert (sig._interp_size, dino._interp_size, dino._image_size) == (576, 576, 378)
    extra = load_exact(sig.vision_tower, "vision_tower_aux_list.0.vision_tower.", lambda k: k.replace("vision_model.", "", 1))
    extra += load_exact(dino.vision_tower, "vision_tower_aux_list.1.vision_tower.")
    px_s = synth.synth_input("pixels/siglip", (2, 3, 384, 384))
    px_d = synth.synth_input("pixels/dino", (2, 3, 378, 378))
    with torch.no_grad():
        s_out = sig._forward(px_s)
        s_pre = sig.vision_tower(px_s, output_hidden_states=True).hidden_states[-1]
        d_out = dino._forward(px_d)
        d_pre = dino.vision_tower(px_d).last_hidden_state
    assert s_out.shape == (2, 576, 1152) and s_pre.shape == (2, 729, 1152)
    assert d_out.shape == (2, 576, 1536) and d_pre.shape == (2, 730, 1536)
    a = {}
    synth.save_digest(a, "out", s_out.numpy())
    synth.save_digest(a, "out_pre_interp", s_pre.numpy())
    save("fulldim_siglip.npz", a)
    a = {}
    synth.save_digest(a, "out", d_out.numpy())
    synth.save_digest(a, "out_pre_interp", d_pre.numpy())
    save("fulldim_dino.npz", a)
    man["siglip"] = dict(layers=LAYERS["siglip"], pixels="pixels/siglip", pixel_shape=[2, 3, 384, 384],
                         out=list(s_out.shape), out_pre_interp=list(s_pre.shape))
    man["dino"] = dict(layers=LAYERS["dino"], pixels="pixels/dino", pixel_shape=[2, 3, 378, 378], out=list(d_out.shape),
                       out_pre_interp=list(d_pre.shape), position_grid="37x37 -> 27x27 (bicubic, transformers %s: "
                       "interpolate(size=...))" % __import__("transformers").__version__)
    man["unused_keys_filled"] = extra


def make_sva(man):
    sampler = vs.VisionTokenSampler(C, C, [C, C], [2, 2], C, 3).eval()
    load_exact(sampler, "vision_sampler_0.")
    side = 12
    vq = SD["vision_query"]
    a, m = {}, {}
    for tag, size in SVA_SIZES.items():
        aux0 = synth.synth_input("features/sva_aux0", (SVA_T, 576, C))
        aux1 = synth.synth_input("features/sva_aux1", (SVA_T, 576, C))
        ctx = aux0.mean(1).view(SVA_T, 1, 1, -1)
        # the reference's own rearrange + window masks on a stub `self` (cambrian_arch.py:601-695)
        feats, masks = arch.CambrianMetaForCausalLM.rearrange_vision_tower_features_inference(
            types.SimpleNamespace(), [aux0, aux1], side, [size] * SVA_T)
        q = vq[0].view(1, 1, 1, -1).expand(SVA_T, side * side, -1, -1).flatten(0, 1)
        c = ctx.expand(-1, side * side, 1, -1).flatten(0, 1)
        with torch.no_grad():
            out = sampler(q, c, *feats, *masks).view(SVA_T, side * side, C)
        synth.save_digest(a, "out_" + tag, out.numpy())
        a["mask0_" + tag] = masks[0].numpy()
        a["mask1_" + tag] = masks[1].numpy()
        m[tag] = dict(image_size=list(size), out=list(out.shape), masked_keys=int((~masks[0]).sum()))
    save("fulldim_sva.npz", a)
    man["sva"] = dict(T=SVA_T, inputs=["features/sva_aux0", "features/sva_aux1"], cases=m)


def make_qformer(man):
    from transformers import BertConfig
    ids = torch.tensor([ref_shims.prompt_to_ids(PROMPT, BERT_KW["vocab_size"])])
    a, m = {"prompt_ids": ids[0].numpy()}, {}
    query_proj, vision_proj = nn.Linear(H, DQ), nn.Linear(DQ, H)
    load_exact(query_proj, "query_proj.")
    load_exact(vision_proj, "vision_proj.")
    for K, N in QFORMER_CASES:
        cfg = BertConfig(**BERT_KW)
        cfg.encoder_width = H
        cfg.add_cross_attention = True
        cfg.cross_attention_freq = 2
        cfg.query_length = K
        qf = Q.BertLMHeadModel(cfg).eval()
        load_exact(qf.bert, "Qformer.bert.")
        chunk = synth.synth_input("features/qformer_N%d" % N, (8, N, H))
        with torch.no_grad():
            # tdc/cambrian_arch.py:1603-1667 in call structure: key frame = chunk[0], the other 7 frames are compressed
            other = chunk[1:]
            L = other.shape[0]
            key_frame = chunk[0].unsqueeze(0).repeat_interleave(L, dim=0)
            qt = torch.nn.functional.adaptive_avg_pool1d(key_frame.permute(2, 0, 1), K).permute(1, 2, 0)
            qt = query_proj(qt).expand(L, -1, -1)
            out = qf.bert(input_ids=ids.expand(L, -1), query_embeds=qt, encoder_hidden_states=other,
                          encoder_attention_mask=torch.ones(other.size()[:-1], dtype=torch.long), use_cache=False,
                          return_dict=True)
            comp = torch.nn.functional.normalize(vision_proj(out.last_hidden_state[:, :K]), dim=-1)
        tag = "K%d_N%d" % (K, N)
        synth.save_digest(a, "out_" + tag, comp.numpy())
        synth.save_digest(a, "last_hidden_" + tag, out.last_hidden_state.numpy())
        m[tag] = dict(chunk="features/qformer_N%d" % N, out=list(comp.shape),
                      last_hidden=list(out.last_hidden_state.shape))
    save("fulldim_qformer.npz", a)
    man["qformer"] = dict(prompt=PROMPT, prompt_ids=ids[0].tolist(), bert=BERT_KW, cases=m)


if __name__ == "__main__":
    import transformers
    man = dict(torch=torch.__version__, transformers=transformers.__version__, numpy=np.__version__,
               reference="Hoar012/TDC-Video @ 2025-08-29",
               weights="synth.synth_state_dict(%d, %d): synth.fill(name, shape), seed = fnv1a64(name)" % (
                   LAYERS["siglip"], LAYERS["dino"]),
               H=H, C=C, dtype="float32")
    make_towers(man)
    make_sva(man)
    make_qformer(man)
    with open(os.path.join(HERE, "manifest_fulldim.json"), "w") as f:
        json.dump(man, f, indent=1)
    print(json.dumps(man, indent=1))
