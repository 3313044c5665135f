"""Host-side mirror of the reference's operator interface for the video-encoding path (the drop-in boundary):

    CambrianMetaModel            tdc/cambrian_arch.py:47-484   (owns the parameters, same names / state-dict keys)
    CambrianMetaForCausalLM      tdc/cambrian_arch.py:546-1898 (encode_images, adapt_segment,
                                                                prepare_inputs_labels_for_multimodal -> 10-tuple)

Same class / method / argument names, config keys and error behaviour, so `CambrianQwenForCausalLM.forward/.generate`
(tdc/language_model/cambrian_qwen.py:260-284, :415-438) and the eval drivers call it unchanged.  All tensor math runs
in libtdc_hip.so through `pipeline.VideoEncoder`; this file only holds parameters (nn.Parameter containers whose
names reproduce the reference state dict), does the host integer logic and the text/visual splice (a21).

Deliberate differences (documented in DESIGN.md): the dead `Qformer.cls` LM head is not allocated; a sample with
several <image> tokens raises IndexError as the reference does (it indexes past its one-entry-per-sample feature list,
tdc/cambrian_arch.py:1716), it is not given a meaning of its own; the three aux
return values used only by in-LLM samplers (`connector_only=False`) are returned as None; `video_indices=[None]`
(what generate() passes) is treated as "not given" instead of raising TypeError when the frame cap triggers
(tdc/cambrian_arch.py:919); training-only entry points raise NotImplementedError.
"""
from abc import ABC, abstractmethod

import torch
import torch.nn as nn

from . import lib as L
from . import segment as seg
from .encode import (FeatureSource, FrameSource, PixelSource, batch_groups, encode_source, frame_indices, normalize_audio,
                     same_source_key)
from .features import FeatureSet, is_feature_set
from .pipeline import VideoEncoder

IGNORE_INDEX = -100        # tdc/constants.py
IMAGE_TOKEN_INDEX = -200


class ParamTree(nn.Module):
    """Container whose nested attribute names reproduce dotted state-dict keys ('0.weight', 'bert.encoder.layer.3...')."""

    def __init__(self, spec=None, init=None):
        super().__init__()
        for name, shape in (spec or {}).items():
            self.add(name, shape, init)

    def add(self, name, shape, init=None):
        head, _, rest = name.partition(".")
        if rest:
            if head not in self._modules:
                self.add_module(head, ParamTree())
            self._modules[head].add(rest, shape, init)
        else:
            p = nn.Parameter(torch.empty(*shape), requires_grad=False)
            (init or _default_init)(name, p)
            self.register_parameter(head, p)


def _default_init(name, p):
    with torch.no_grad():
        if p.ndim >= 2:
            p.normal_(0.0, 0.02)
        elif "weight" in name or "lambda1" in name:
            p.fill_(1.0)
        else:
            p.zero_()


def _randn_init(name, p):
    with torch.no_grad():
        p.normal_(0.0, 1.0)


# ------------------------------------------------------------------------------------------------ parameter specs
def _linear(spec, name, n, k, bias=True):
    spec[name + ".weight"] = (n, k)
    if bias:
        spec[name + ".bias"] = (n,)


def _ln(spec, name, n):
    spec[name + ".weight"] = (n,)
    spec[name + ".bias"] = (n,)


def qformer_spec(dq, layers, ffn, enc_width, vocab, max_pos, cross_freq=2):
    s = {}
    p = "bert."
    s[p + "embeddings.word_embeddings.weight"] = (vocab, dq)
    s[p + "embeddings.position_embeddings.weight"] = (max_pos, dq)
    _ln(s, p + "embeddings.LayerNorm", dq)
    for i in range(layers):
        l = p + "encoder.layer.%d." % i
        for n in ("query", "key", "value"):
            _linear(s, l + "attention.self." + n, dq, dq)
        _linear(s, l + "attention.output.dense", dq, dq)
        _ln(s, l + "attention.output.LayerNorm", dq)
        if i % cross_freq == 0:
            _linear(s, l + "crossattention.self.query", dq, dq)
            _linear(s, l + "crossattention.self.key", dq, enc_width)
            _linear(s, l + "crossattention.self.value", dq, enc_width)
            _linear(s, l + "crossattention.output.dense", dq, dq)
            _ln(s, l + "crossattention.output.LayerNorm", dq)
        for a, b in (("intermediate", "output"), ("intermediate_query", "output_query")):
            _linear(s, l + a + ".dense", ffn, dq)
            _linear(s, l + b + ".dense", dq, ffn)
            _ln(s, l + b + ".LayerNorm", dq)
    return s


def sva_spec(C, depth, n_towers=2, r=2):
    s = {}
    for i in range(depth):
        l = "layers.%d." % i
        for t in range(n_towers):
            s[l + "pos_embed_%d" % t] = (r * r, C)
        _linear(s, l + "proj_context", C, C, False)
        _linear(s, l + "proj_in", C, 2 * C, False)
        _linear(s, l + "proj_out.linear_1", C, C, False)
        _linear(s, l + "proj_out.linear_2", C, C, False)
        _ln(s, l + "norm", C)
        _ln(s, l + "cross_attn.q_proj.0", C)
        _linear(s, l + "cross_attn.q_proj.1", C, C, False)
        for t in range(n_towers):
            for kv in "kv":
                _ln(s, l + "cross_attn.%s_proj_%d.0" % (kv, t), C)
                _linear(s, l + "cross_attn.%s_proj_%d.1" % (kv, t), C, C, False)
        _linear(s, l + "cross_attn.o_proj", C, C, False)
    return s


def siglip_spec(D=1152, layers=27, mlp=4304, n_pos=729, patch=14):
    s = {"embeddings.patch_embedding.weight": (D, 3, patch, patch), "embeddings.patch_embedding.bias": (D,),
         "embeddings.position_embedding.weight": (n_pos, D)}
    for i in range(layers):
        l = "encoder.layers.%d." % i
        _ln(s, l + "layer_norm1", D)
        _ln(s, l + "layer_norm2", D)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            _linear(s, l + "self_attn." + n, D, D)
        _linear(s, l + "mlp.fc1", mlp, D)
        _linear(s, l + "mlp.fc2", D, mlp)
    return s


def dino_spec(D=1536, layers=40, hidden=4096, n_pos=37 * 37, patch=14):
    s = {"embeddings.cls_token": (1, 1, D), "embeddings.position_embeddings": (1, 1 + n_pos, D),
         "embeddings.patch_embeddings.projection.weight": (D, 3, patch, patch),
         "embeddings.patch_embeddings.projection.bias": (D,)}
    for i in range(layers):
        l = "encoder.layer.%d." % i
        _ln(s, l + "norm1", D)
        _ln(s, l + "norm2", D)
        for n in ("query", "key", "value"):
            _linear(s, l + "attention.attention." + n, D, D)
        _linear(s, l + "attention.output.dense", D, D)
        s[l + "layer_scale1.lambda1"] = (D,)
        s[l + "layer_scale2.lambda1"] = (D,)
        _linear(s, l + "mlp.weights_in", 2 * hidden, D)
        _linear(s, l + "mlp.weights_out", D, hidden)
    _ln(s, "layernorm", D)
    return s


class VisionTowerHandle:
    """Stands where the reference keeps SiglipVisionTower / DinoVisionTower objects (a plain python list,
    tdc/cambrian_arch.py:62; tdc/multimodal_encoder/builder.py:8-37).  `vision_tower` holds the HF-named parameters."""

    def __init__(self, kind, name, arch):
        self.kind, self.vision_tower_name = kind, name
        self.arch = dict(arch)
        self.hidden_size = arch["D"]
        self.heads = arch["heads"]
        self.is_loaded = False
        self.vision_tower = None
        self._interp_size = 576
        self.image_size = 384 if kind == "siglip" else 378

    def load_model(self, device_map=None, state_dict=None):
        """Allocates the tower parameters (random init); pass `state_dict` (HF names) to load released weights - the
        reference pulls them from the hub (siglip_encoder.py:28, dino_encoder.py:28), which this image cannot reach."""
        a = self.arch
        if self.kind == "siglip":
            spec = siglip_spec(a["D"], a["layers"], a["mlp"], a["n_pos"])
        else:
            spec = dino_spec(a["D"], a["layers"], a["mlp"], a["n_pos"])
        self.vision_tower = ParamTree(spec)
        if state_dict is not None:
            sd = {k.replace("vision_model.", ""): v for k, v in state_dict.items()}
            self.vision_tower.load_state_dict(sd, strict=False)
        self.is_loaded = True


SIGLIP_SO400M = dict(D=1152, layers=27, mlp=4304, n_pos=729, heads=16)
DINOV2_GIANT = dict(D=1536, layers=40, mlp=4096, n_pos=37 * 37, heads=24)


def build_vision_tower_aux_list(config, tower_archs=None, **kwargs):
    """tdc/multimodal_encoder/builder.py:8-37: tower picked by name ('siglip' / 'dinov2')."""
    names = getattr(config, "mm_vision_tower_aux_list", getattr(config, "vision_tower_aux_list", None))
    out = []
    for i, n in enumerate(names):
        if "siglip" in n.lower():
            out.append(VisionTowerHandle("siglip", n, (tower_archs or {}).get("siglip", SIGLIP_SO400M)))
        elif "dinov2" in n.lower():
            out.append(VisionTowerHandle("dino", n, (tower_archs or {}).get("dino", DINOV2_GIANT)))
        else:
            raise ValueError(f"Unknown vision tower: {n}")
    return out


class BeatsHandle:
    """stands where the reference keeps `audio_encoder.beats` (a BEATs nn.Module): checkpoint cfg + state dict; the
    compute lives in beats.BeatsEncoder."""

    def __init__(self, cfg, state):
        self.cfg = dict(cfg) if not hasattr(cfg, "__dict__") or isinstance(cfg, dict) else dict(cfg.__dict__)
        self.state = state
        self._enc = None

    def state_dict(self):
        return self.state

    def extract_features(self, source, padding_mask=None, feature_only=True, device=None, dtype=torch.float16):
        """BEATs.extract_features(..., feature_only=True) (BEATs.py:131-178) -> (features, padding_mask)."""
        if not feature_only:
            raise NotImplementedError("the AS2M classifier head is not on the path")
        if self._enc is None:
            from .beats import BeatsEncoder
            self._enc = BeatsEncoder(self.state, self.cfg, dtype=dtype,
                                     device=device or ("cuda:%d" % torch.cuda.current_device()))
        feats = self._enc.extract_features(source, padding_mask)
        if padding_mask is not None:         # the reference hands back the mask reduced to one flag per token (BEATs.py:142-153)
            pm = torch.as_tensor(padding_mask).bool()
            frames = int(L.load().tdc_fbank_frames(int(pm.shape[1])))
            padding_mask = self._enc.forward_padding_mask(feats.shape[1], self._enc.forward_padding_mask(frames, pm))
        return feats, padding_mask


class AudioEncoderHandle:
    """tdc/audio_models/audio_encoder.py:20-70 reduced to what the path uses: `.beats_path`, `.beats`."""

    def __init__(self, beats_path="", beats_ckpt=None):
        self.beats_path = beats_path
        self.beats = None
        if beats_ckpt is None and beats_path:
            import os
            if os.path.exists(beats_path):
                beats_ckpt = torch.load(beats_path, map_location="cpu")
        if beats_ckpt is not None:
            self.beats = BeatsHandle(beats_ckpt["cfg"], beats_ckpt["model"])


class CambrianMetaModel:
    """Mixin placed before the HF base model in the MRO (tdc/cambrian_arch.py:47-181)."""

    def __init__(self, config):
        super(CambrianMetaModel, self).__init__(config)
        if hasattr(config, "mm_vision_tower_aux_list"):
            projector_type = getattr(config, "mm_projector_type", "linear")
            if projector_type != "sva":
                raise NotImplementedError("only mm_projector_type='sva' is on the accelerated path "
                                          "(tdc/cambrian_arch.py:55-161)")
            C = config.vision_hidden_size
            H = config.hidden_size
            self.vision_tower_aux_list = build_vision_tower_aux_list(
                config, tower_archs=getattr(config, "tdc_tower_archs", None), delay_load=True)
            self.mm_projector = ParamTree({"0.weight": (H, C * config.num_query_group), "0.bias": (H,),
                                           "2.weight": (H, H), "2.bias": (H,)})
            for i, t in enumerate(self.vision_tower_aux_list):
                setattr(self, "mm_projector_aux_%d" % i, ParamTree({
                    "0.weight": (C, t.hidden_size), "0.bias": (C,), "2.weight": (C, C), "2.bias": (C,),
                    "3.weight": (C,), "3.bias": (C,)}))
            tok = config.mm_vision_tower_aux_token_len_list
            for g in range(config.num_query_group):
                r = int(tok[0] ** 0.5) // int(config.query_num_list[g] ** 0.5)
                setattr(self, "vision_sampler_%d" % g, ParamTree(
                    sva_spec(C, config.connector_depth, len(self.vision_tower_aux_list), r),
                    init=lambda n, p: (_randn_init if n.startswith("pos_embed") else _default_init)(n, p)))
            if not getattr(config, "connector_only", True):
                raise NotImplementedError("connector_only=False (in-LLM vision samplers) is outside the hot path")
            self.vision_query = nn.Parameter(torch.randn(config.num_query_group, C), requires_grad=False)
            self.image_newline = nn.Parameter(torch.randn(H) * 0.02, requires_grad=False)
            self.frame_seg = nn.Parameter(torch.randn(H), requires_grad=False)
        self.initialize_compressor(config=config, pretrained_qformer=None,
                                   context_token_num=getattr(config, "context_token_num", 16))
        if getattr(config, "audio_input", False):
            self.audio_proj = ParamTree({"weight": (config.hidden_size, 768), "bias": (config.hidden_size,)})
        self._tdc_encoder = None

    def get_vision_tower_aux_list(self):
        return getattr(self, "vision_tower_aux_list", None)

    def get_frame_pos(self, time_range):
        raise NotImplementedError("frame_pos=True is not used by the released configs (tdc/cambrian_arch.py:183-190)")

    def initialize_vision_modules(self, model_args, fsdp=None):
        raise NotImplementedError("training-time module initialisation (tdc/cambrian_arch.py:206-401) is out of scope")

    def initialize_audio(self, model_args=None, beats_path="./checkpoints/audio_encoder/BEATs/"
                         "BEATs_iter3_plus_AS2M_finetuned_on_AS2M_cpt2.pt", beats_ckpt=None):
        """tdc/cambrian_arch.py:451-467: `audio_proj` + the BEATs half of AudioEncoder (audio_encoder.py:60-70; the
        Whisper / speech-Q-Former half is commented out in the reference).  `beats_ckpt` = {'cfg': ..., 'model': state
        dict} (what torch.load(beats_path) returns) may be passed directly."""
        if not hasattr(self, "audio_proj"):
            self.audio_proj = ParamTree({"weight": (self.config.hidden_size, 768), "bias": (self.config.hidden_size,)})
        self.audio_encoder = AudioEncoderHandle(beats_path, beats_ckpt)
        self._tdc_beats = None
        return self.audio_encoder

    def tdc_beats(self, device=None, dtype=None):
        """BeatsEncoder built (once) from audio_encoder.beats' checkpoint; None when no audio encoder is attached."""
        ae = getattr(self, "audio_encoder", None)
        if ae is None or ae.beats is None:
            return None
        if getattr(self, "_tdc_beats", None) is None:
            from .beats import BeatsEncoder
            eng = self.tdc_engine()
            self._tdc_beats = BeatsEncoder(ae.beats.state, ae.beats.cfg, dtype=dtype or eng.dtype, device=device or eng.dev)
        return self._tdc_beats

    def initialize_compressor(self, config, pretrained_qformer=None, context_token_num=16):
        """tdc/cambrian_arch.py:469-484 (+ init_Qformer :403-424): bert-base Q-Former with cross-attention to the LLM
        embedding width every other layer; query_proj / vision_proj."""
        H = config.hidden_size
        qc = getattr(config, "tdc_qformer_arch", None) or dict(hidden=768, layers=12, heads=12, ffn=3072, vocab=30522,
                                                               max_pos=512)
        self._qformer_arch = dict(qc)
        self.Qformer = ParamTree(qformer_spec(qc["hidden"], qc["layers"], qc["ffn"], H, qc["vocab"], qc["max_pos"]))
        self.query_tokens = nn.Parameter(torch.zeros(1, context_token_num, qc["hidden"]).normal_(0, 0.02),
                                         requires_grad=False)
        self.vision_proj = ParamTree({"weight": (H, qc["hidden"]), "bias": (H,)})
        self.query_proj = ParamTree({"weight": (qc["hidden"], H), "bias": (qc["hidden"],)})
        self.bert_tokenizer = None
        try:  # the reference loads ./checkpoints/bert-base-uncased (tdc/cambrian_arch.py:405)
            from transformers import BertTokenizer
            self.bert_tokenizer = BertTokenizer.from_pretrained("./checkpoints/bert-base-uncased",
                                                                truncation_side="right")
        except Exception:
            self.bert_tokenizer = None

    # ---- HIP engine -------------------------------------------------------------------------------------------
    def tdc_state_dict(self):
        """reference-named state dict (without 'model.') of everything on the path, towers included."""
        sd = {}
        for k, v in self.state_dict().items():
            if k.startswith(("mm_projector", "vision_sampler_", "vision_query", "image_newline", "frame_seg",
                             "Qformer.", "vision_proj", "query_proj", "audio_proj", "query_tokens")):
                sd[k] = v
        for i, t in enumerate(self.vision_tower_aux_list):
            if not t.is_loaded:
                t.load_model()
            for k, v in t.vision_tower.state_dict().items():
                sd["vision_tower_aux_list.%d.vision_tower.%s" % (i, k)] = v
        return sd

    def tdc_engine(self, device=None, dtype=None, refresh=False):
        """Build (once) the VideoEncoder from the current parameters: pads / fuses / uploads the weights.
        Keys that are not reference keys (all optional; INTEGRATION.md lists them):
        `config.tdc_fp8_towers = True` / 2 / 3 selects e4m3 operands for the towers' qkv / fc1 GEMMs (2: out-proj / fc2 as
        well; 3: fc1 also writes the e4m3 MLP hidden itself) - a throughput mode, not a parity mode;
        `config.tdc_tower_dtype = "bfloat16" | "float16"`: GEMM operand type of the two ViT towers under a connector / Q-Former
        in `dtype`; `config.tdc_dino_dtype`: the same for the DINOv2 tower alone (it alone drives the a5 segment selection,
        tdc/cambrian_arch.py:832-849: "float16" there keeps the similarities at the reference's own precision under a bf16
        SigLIP tower);
        `config.tdc_selection_refine` (default: automatic - on when the DINOv2 operands are bf16) / `config.tdc_selection_eps`
        (default 1e-3): the a5 segment selection at the reference's precision under bf16 DINOv2 operands - the pairs whose
        similarities decide the selection and lie closer than the operand type's error are re-encoded by an fp16-operand copy of
        the DINOv2 tower, as long as their frames number at most max(8, `config.tdc_selection_max_fraction` (default 1/8) x frames)
        (VideoEncoder.selection_refine);
        `config.tdc_tower_res_dtype = "float16" | "bfloat16" | "float32"`: the towers' residual stream in HBM.  Default:
        "float16" when the towers' operands are fp16 - the reference's own arithmetic, its HF towers run under
        torch_dtype=float16 (tdc/builder.py:69) -, "float32" otherwise (bf16 operands reach 3e38, an fp16 stream ends at 65504:
        that combination - what bench.py measures - is opt-in; fp8 towers follow the same rule);
        `config.tdc_tower_batch`: frames per tower batch; default: every frame of the call up to 512, bounded by the free HBM
        (VideoEncoder.auto_tower_batch; the result does not depend on it bit for bit, the reference's own chunk is 64,
        tdc/cambrian_arch.py:698-745);
        `config.tdc_frame_cap` (default 224 = the reference's "in case of OOM" constant, tdc/cambrian_arch.py:907-916,813-822):
        the cap of both frame sub-samplings; `config.tdc_shard_frames`: see prepare_inputs_labels_for_multimodal;
        `config.tdc_video_cache_bytes`: see tdc_video_cache; `config.tdc_shard_cache_bytes`: see tdc_shard_cache;
        `config.tdc_batch_frames`: see tdc_batch_frames; `config.tdc_feature_inputs`: see tdc_feature_inputs;
        `config.tdc_frame_inputs`: see tdc_frame_inputs; `config.tdc_kv_cache_bytes`: see tdc_kv_cache_bytes.
        bench.py's line is reproduced by dtype=float16, tdc_tower_dtype="bfloat16", tdc_tower_res_dtype="float16",
        tdc_frame_cap=T (its `product_setting` field says so; `bench.py --via-mixin` runs exactly that)."""
        if self._tdc_encoder is None or refresh:
            cfg = {k: getattr(self.config, k) for k in dir(self.config)
                   if not k.startswith("_") and (isinstance(getattr(self.config, k, None), (int, float, str, bool, list)) or
                                                 (k.startswith("tdc_") and isinstance(getattr(self.config, k, None), torch.dtype)))}
            device = device or ("cuda:%d" % torch.cuda.current_device())
            dtype = dtype or (self.dtype if self.dtype in (torch.float16, torch.bfloat16) else torch.float16)
            towers = self.vision_tower_aux_list
            fp8 = int(cfg.get("tdc_fp8_towers", 0) or 0)
            tower_dtype = _dtype_key(cfg, "tdc_tower_dtype", allow32=False)
            dino_dtype = _dtype_key(cfg, "tdc_dino_dtype", allow32=False)
            if "tdc_tower_res_dtype" in cfg:
                res = _dtype_key(cfg, "tdc_tower_res_dtype")
            else:
                res = torch.float16 if (tower_dtype or dtype) == torch.float16 and (dino_dtype or tower_dtype or dtype) == \
                    torch.float16 else None
            sel_refine = cfg.get("tdc_selection_refine")            # None = automatic (on under bf16 DINOv2 operands)
            if sel_refine is not None and not isinstance(sel_refine, bool):
                raise ValueError("config.tdc_selection_refine must be True / False (or absent for the automatic choice), got %r"
                                 % (sel_refine,))
            sel_eps = cfg.get("tdc_selection_eps", 1e-3)
            if isinstance(sel_eps, bool) or not isinstance(sel_eps, (int, float)) or not (0 < sel_eps < 1):
                raise ValueError("config.tdc_selection_eps must be a similarity error bound in (0, 1), got %r" % (sel_eps,))
            sel_frac = cfg.get("tdc_selection_max_fraction", 0.125)
            if isinstance(sel_frac, bool) or not isinstance(sel_frac, (int, float)) or not (0 <= sel_frac <= 1):
                raise ValueError("config.tdc_selection_max_fraction must be a fraction of the frames in [0, 1], got %r" % (sel_frac,))
            tb = cfg.get("tdc_tower_batch")
            if tb is not None and (isinstance(tb, bool) or not isinstance(tb, int) or tb < 0):
                raise ValueError("config.tdc_tower_batch must be a positive frame count (or 0 / absent for the automatic "
                                 "choice), got %r" % (tb,))
            self._tdc_encoder = VideoEncoder(self.tdc_state_dict(), cfg, dtype=dtype, device=device,
                                             siglip_heads=towers[0].heads, dino_heads=towers[1].heads,
                                             qformer_heads=self._qformer_arch["heads"], fp8_towers=fp8,
                                             tower_batch=tb or None, tower_dtype=tower_dtype, dino_dtype=dino_dtype,
                                             ln_fuse=bool(cfg.get("tdc_ln_fuse", False)),
                                             selection_refine=sel_refine, selection_eps=sel_eps,
                                             selection_max_fraction=sel_frac,
                                             tower_res_dtype=res)
        return self._tdc_encoder

    def tdc_frame_cap(self):
        """`config.tdc_frame_cap`: the reference's constant 224 of both frame caps (tdc/cambrian_arch.py:907-916,813-822; SURVEY
        D3) as a config key.  224 (the default) is the parity setting."""
        cap = getattr(self.config, "tdc_frame_cap", 224)
        if cap is None:
            return 224
        if isinstance(cap, bool) or not isinstance(cap, int) or cap < 1:
            raise ValueError("config.tdc_frame_cap must be a positive frame count, got %r" % (cap,))
        return cap

    def tdc_video_cache(self):
        """the engine's FrameCache (cache.py) when `config.tdc_video_cache_bytes` is a positive byte budget; None when the key
        is absent or 0.  Videos and single images then skip the towers and the connector for frames whose content the
        cache holds - the results are bit for bit those without it.  Ignored (None) under `config.tdc_shard_frames`:
        the frame-sharded path has a per-rank cache of its own (tdc_shard_cache).  A new engine (tdc_engine(refresh=True))
        gets a new, empty cache.  `config.tdc_kv_cache_bytes` (tdc_kv_cache_bytes) gives it a K/V budget."""
        n = getattr(self.config, "tdc_video_cache_bytes", None)
        if isinstance(n, bool) or not (n is None or isinstance(n, int)) or (n or 0) < 0:
            raise ValueError("config.tdc_video_cache_bytes must be a byte budget (a non-negative int; 0 / absent = off), "
                             "got %r" % (n,))
        kv = self.tdc_kv_cache_bytes()
        if not n or getattr(self.config, "tdc_shard_frames", False):
            return None
        eng = self.tdc_engine()
        c = getattr(self, "_tdc_video_cache", None)
        if c is None or getattr(self, "_tdc_video_cache_engine", None) is not eng or c.max_bytes != n or \
                getattr(c, "kv_max_bytes", 0) != kv:
            c = self._tdc_video_cache = eng.new_cache(n, kv) if kv else eng.new_cache(n)
            self._tdc_video_cache_engine = eng
        return c

    def tdc_kv_cache_bytes(self):
        """`config.tdc_kv_cache_bytes`: a byte budget of its own inside the frame cache for the Q-Former's cross-attention K/V
        (DESIGN.md section 17): one entry per (video, a1 selection), so a later question about a cached video skips the stacked
        K/V projection and the row gather in front of it - the 10-tuple is bit for bit the key-off call's.  0 / absent: off.
        It lives in the frame cache, so it needs `config.tdc_video_cache_bytes`, and composes with `config.tdc_batch_prompts`
        and `tdc_frame_inputs`, which go through that cache; set together with `config.tdc_shard_frames`,
        `tdc_shard_cache_bytes`, `tdc_batch_frames` or `tdc_feature_inputs` it raises: those paths keep no K/V."""
        n = getattr(self.config, "tdc_kv_cache_bytes", None)
        if isinstance(n, bool) or not (n is None or isinstance(n, int)) or (n or 0) < 0:
            raise ValueError("config.tdc_kv_cache_bytes must be a byte budget (a non-negative int; 0 / absent = off), "
                             "got %r" % (n,))
        if not n:
            return 0
        if not getattr(self.config, "tdc_video_cache_bytes", None):
            raise ValueError("config.tdc_kv_cache_bytes needs config.tdc_video_cache_bytes: the K/V entries live in the "
                             "frame cache and are keyed by its fingerprints")
        for other in ("tdc_shard_frames", "tdc_shard_cache_bytes", "tdc_batch_frames", "tdc_feature_inputs"):
            if getattr(self.config, other, None):
                raise ValueError("config.tdc_kv_cache_bytes and config.%s cannot be set together" % other)
        return n

    def tdc_video_cache_clear(self):
        """empty the frame cache (and release its device memory); no-op when it is off"""
        c = getattr(self, "_tdc_video_cache", None)
        if c is not None:
            c.clear()

    def tdc_shard_cache(self):
        """this rank's FrameCache of the frame-sharded path (dist.ShardedVideoEncoder.encode_video(cache=...)) when
        `config.tdc_shard_cache_bytes` is a positive per-rank byte budget and `config.tdc_shard_frames` is set; None when the
        key is absent or 0.  Each rank caches its own frames; a second question on a video skips the towers and the
        connector on every rank whose frames the cache holds - the results are bit for bit those without it.  A new engine
        (tdc_engine(refresh=True)) gets a new, empty cache."""
        n = getattr(self.config, "tdc_shard_cache_bytes", None)
        if isinstance(n, bool) or not (n is None or isinstance(n, int)) or (n or 0) < 0:
            raise ValueError("config.tdc_shard_cache_bytes must be a per-rank byte budget (a non-negative int; 0 / absent = "
                             "off), got %r" % (n,))
        if not n or not getattr(self.config, "tdc_shard_frames", False):
            return None
        eng = self.tdc_engine()
        c = getattr(self, "_tdc_shard_cache", None)
        if c is None or getattr(self, "_tdc_shard_cache_engine", None) is not eng or c.max_bytes != n:
            c = self._tdc_shard_cache = eng.new_cache(n)
            self._tdc_shard_cache_engine = eng
        return c

    def tdc_shard_cache_clear(self):
        """empty this rank's frame cache of the sharded path (and release its device memory); no-op when it is off"""
        c = getattr(self, "_tdc_shard_cache", None)
        if c is not None:
            c.clear()

    def tdc_batch_frames(self):
        """`config.tdc_batch_frames`: the frame ceiling of a batched encode - the samples of one call are grouped greedily in
        batch order, up to that many a1-selected frames per group (images: 1), and each group of two or more runs through
        one tower and connector pass (VideoEncoder.encode_batch), bit for bit the per-sample results.  0 / absent: off, every
        sample is encoded on its own (the default: a group holds its samples' pixels, tower features and connector rows on
        the device at once).  Ignored (0) under `config.tdc_shard_frames` and with `config.tdc_video_cache_bytes` on."""
        n = getattr(self.config, "tdc_batch_frames", None)
        if n is None:
            return 0
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError("config.tdc_batch_frames must be a frame ceiling (a non-negative int; 0 / absent = off), got %r"
                             % (n,))
        if getattr(self.config, "tdc_shard_frames", False) or getattr(self.config, "tdc_video_cache_bytes", None):
            return 0
        return n

    def tdc_batch_prompts(self):
        """`config.tdc_batch_prompts`: the most prompts of one compressor pass - the samples of one call (bsz > 1) that carry the
        same video (equal engine.fingerprint of their a1-selected pixels, equal image_size, equal audio) run through
        VideoEncoder.encode_video_prompts, bit for bit the per-sample results.  0 / absent: off, every sample on its own.  Set
        together with `config.tdc_shard_frames` or `config.tdc_batch_frames` it raises: the paths do not compose."""
        n = getattr(self.config, "tdc_batch_prompts", None)
        if n is None:
            return 0
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError("config.tdc_batch_prompts must be a prompt count (a non-negative int; 0 / absent = off), got %r"
                             % (n,))
        if n:
            for other in ("tdc_shard_frames", "tdc_batch_frames"):
                if getattr(self.config, other, None):
                    raise ValueError("config.tdc_batch_prompts and config.%s cannot be set together" % other)
        return n

    def tdc_feature_inputs(self):
        """`config.tdc_feature_inputs`: True = `images` carries stored tower features instead of pixels (features.FeatureSet,
        VideoEncoder.export_features): images[0][i] / images[1][i] are the SigLIP / DINOv2 rows of sample i, [T, tokens,
        hidden_size of that tower], or images[0][i] is a FeatureSet - lossless or compact (store="e4m3"; raw tensors are
        always lossless) - and images[1][i] None; every sample runs through
        VideoEncoder.encode_features (images: its connector-only form).  Absent / False: pixels.  Set together with
        `config.tdc_shard_frames`, `tdc_batch_frames`, `tdc_video_cache_bytes` or `tdc_shard_cache_bytes` it raises: those need
        pixels, or key on them.  `config.tdc_batch_prompts` composes with it."""
        v = getattr(self.config, "tdc_feature_inputs", None)
        if v is None:
            return False
        if not isinstance(v, bool):
            raise ValueError("config.tdc_feature_inputs must be True / False (absent = off), got %r" % (v,))
        if v:
            for other in ("tdc_shard_frames", "tdc_batch_frames", "tdc_video_cache_bytes", "tdc_shard_cache_bytes"):
                if getattr(self.config, other, None):
                    raise ValueError("config.tdc_feature_inputs and config.%s cannot be set together" % other)
        return v

    def tdc_frame_inputs(self):
        """`config.tdc_frame_inputs`: True = `images` carries decoded uint8 frames instead of pixels.  Videos: images[0][i] is the
        uint8 [T, H, W, 3] tensor (or numpy array) of sample i, on the host or the device, and images[1] is ignored (None);
        single images: images[0] is uint8 [bsz, H, W, 3].  An entry images[0][i] (videos), or images[0] itself (single images),
        may be a preprocess.YuvFrames - NV12 / I420 planes as the decoder wrote them - or a
        preprocess.Oriented over either kind: stored frames plus their display rotation / mirror (image_sizes
        is then the upright frames') - or a preprocess.RgbFrames: channel-first [T, 3, H, W], B G R, RGBA / BGRA / ARGB or gray
        pictures as their source wrote them, bare or inside an Oriented - or a preprocess.Interlaced over
        any of these kinds (interlaced video, one field kept and rebuilt to full height), bare or inside an
        Oriented.  Every sample runs through VideoEncoder.encode_frames: a1 first, then
        only the kept frames are uploaded and resized - the 10-tuple is bit for bit the pixel call's on
        preprocess.process_images of the same frames.  Absent / False: pixels.  Composes with `config.tdc_video_cache_bytes`;
        set together with `config.tdc_feature_inputs`, `tdc_shard_frames`, `tdc_batch_frames`, `tdc_shard_cache_bytes` or
        `tdc_batch_prompts` it raises: those paths take pixels or features."""
        v = getattr(self.config, "tdc_frame_inputs", None)
        if v is None:
            return False
        if not isinstance(v, bool):
            raise ValueError("config.tdc_frame_inputs must be True / False (absent = off), got %r" % (v,))
        if v:
            for other in ("tdc_feature_inputs", "tdc_shard_frames", "tdc_batch_frames", "tdc_shard_cache_bytes",
                          "tdc_batch_prompts"):
                if getattr(self.config, other, None):
                    raise ValueError("config.tdc_frame_inputs and config.%s cannot be set together" % other)
        return v

    def tdc_return_aux(self):
        """`config.tdc_return_aux`: True = prepare_inputs_labels_for_multimodal fills slots 6, 7 and 9 of its 10-tuple with the
        reference's vision_tower_aux_feature_list_final, vision_tower_aux_attention_masks_list_final and
        global_context_feature_final (tdc/cambrian_arch.py:1187-1193, 1295-1303, 1833-1844), concatenated
        over the samples of the call in sample order, on the engine device; everything else of the tuple is the key-off
        call's.  Absent / False: the three slots are None.  Composes with `tdc_frame_inputs` and `tdc_feature_inputs`; set
        together with `config.tdc_video_cache_bytes`, `tdc_kv_cache_bytes`, `tdc_shard_frames`, `tdc_shard_cache_bytes`,
        `tdc_batch_frames` or `tdc_batch_prompts` it raises: those paths keep or move connector rows, not aux rows."""
        v = getattr(self.config, "tdc_return_aux", None)
        if v is None:
            return False
        if not isinstance(v, bool):
            raise ValueError("config.tdc_return_aux must be True / False (absent = off), got %r" % (v,))
        if v:
            for other in ("tdc_video_cache_bytes", "tdc_kv_cache_bytes", "tdc_shard_frames", "tdc_shard_cache_bytes",
                          "tdc_batch_frames", "tdc_batch_prompts"):
                if getattr(self.config, other, None):
                    raise ValueError("config.tdc_return_aux and config.%s cannot be set together" % other)
        return v

    def tdc_prompt_pad_fraction(self):
        """`config.tdc_prompt_pad_fraction`: the share of a prompt group's rows that may be padding (encode.prompt_groups);
        absent: 1/4."""
        v = getattr(self.config, "tdc_prompt_pad_fraction", None)
        if v is None:
            return 0.25
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
            raise ValueError("config.tdc_prompt_pad_fraction must be a fraction in [0, 1] (absent = 0.25), got %r" % (v,))
        return float(v)

    def tdc_side_stream(self, frames_per_rank):
        """engine.two_streams (encode.start_side_tower): the config's choice, by default on at <= 128 frames per rank"""
        ts = getattr(self.config, "tdc_two_streams", None)
        return bool(ts) if ts is not None else frames_per_rank <= 128

    def tdc_sharded_engine(self):
        """dist.ShardedVideoEncoder over the default process group when `config.tdc_shard_frames` is set and
        torch.distributed runs with more than one rank (one process per GPU, RCCL); None otherwise."""
        if not getattr(self.config, "tdc_shard_frames", False):
            return None
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
            return None
        sh = getattr(self, "_tdc_sharded", None)
        if sh is None or sh.e is not self.tdc_engine():
            from .dist import ShardedVideoEncoder
            sh = self._tdc_sharded = ShardedVideoEncoder(self.tdc_engine(), dist.get_rank(), dist.get_world_size())
        return sh


_DT16 = {"bfloat16": torch.bfloat16, "bf16": torch.bfloat16, "float16": torch.float16, "fp16": torch.float16,
         "half": torch.float16, "float32": None, "fp32": None, "float": None, None: None}


def _dtype_key(cfg, key, allow32=True):
    """config string -> torch dtype (None = fp32 / not given), with an error that names the key and the accepted values."""
    v = cfg.get(key)
    if isinstance(v, torch.dtype):
        v = str(v).replace("torch.", "")
    if v not in _DT16 or (not allow32 and v is not None and _DT16[v] is None):
        ok = sorted(k for k in _DT16 if k is not None and (allow32 or _DT16[k] is not None))
        raise ValueError("config.%s = %r is not one of %s" % (key, v, ok))
    return _DT16[v]


class CambrianMetaForCausalLM(ABC):
    """tdc/cambrian_arch.py:546-1898."""

    @abstractmethod
    def get_model(self):
        pass

    def get_vision_tower_aux_list(self):
        return self.get_model().get_vision_tower_aux_list()

    # ---- a2 -----------------------------------------------------------------------------------------------------
    def encode_images(self, image_aux_list, encode_type=None):
        """tdc/cambrian_arch.py:698-745: run a tower ('dino' -> last entry, 'siglip' -> first, None -> all) in 64-frame
        batches; returns [B, 576, D] tensors (list for encode_type None)."""
        eng = self.get_model().tdc_engine()
        towers = self.get_model().get_vision_tower_aux_list()

        def run(kind, px, D):
            out = eng.tower(kind, px.to(eng.dev))
            return out[:, :D].reshape(px.shape[0], -1, D)
        if encode_type == "dino":
            return run("dino", image_aux_list[-1], towers[-1].hidden_size)
        if encode_type == "siglip":
            return run("siglip", image_aux_list[0], towers[0].hidden_size)
        return [run(t.kind, px, t.hidden_size) for px, t in zip(image_aux_list, towers)]

    # ---- a1 -----------------------------------------------------------------------------------------------------
    def _budget_text_len(self, cur_input_ids):
        pad_id = 128002 if "llama" in getattr(self.get_model().config, "model_type", "") else 151643
        pos = torch.where(cur_input_ids == pad_id)[-1]
        return int(pos[0]) if len(pos) > 0 else len(cur_input_ids)

    def _cfg(self):
        c = self.get_model().config
        keys = ("context_token_num", "audio_input", "add_static", "tokenizer_model_max_length", "inference_max_length",
                "max_num_segments", "text_input", "query_type")
        d = {k: getattr(c, k) for k in keys if hasattr(c, k)}
        return d

    def get_max_num_frames(self, cur_input_ids):
        """tdc/cambrian_arch.py:748-780."""
        return seg.get_max_num_frames(self._budget_text_len(cur_input_ids), self._cfg())

    def adapt_segment(self, feature_list, split_sizes, new_image_aux_list, window_size=64, threshold=0.9,
                      max_num_segments=24):
        """tdc/cambrian_arch.py:783-861 (same 5-tuple).  feature_list: DINO features [sum T, 576, D]."""
        eng = self.get_model().tdc_engine()
        feats = torch.split(feature_list, split_sizes, dim=0)
        a0 = torch.split(new_image_aux_list[0], split_sizes, dim=0)
        a1 = torch.split(new_image_aux_list[1], split_sizes, dim=0)
        out_f, out_0, out_1, new_sizes, sel_all, seg_all = [], [], [], [], [], []
        for i, f in enumerate(feats):
            T = len(f)
            if T <= max_num_segments + 1:
                idx, segi = list(range(T)), list(range(T))
            else:
                idx = seg.uniform_indices(T, self.get_model().tdc_frame_cap())     # :813-822 (config.tdc_frame_cap)
                ff = f[idx] if len(idx) != T else f
                P, D = ff.shape[1], ff.shape[2]
                flat = ff.reshape(len(idx) * P, D).contiguous()
                if D % 8:
                    raise ValueError("feature width must be a multiple of 8")
                segi = seg.select_segments(eng.frame_sims(flat.to(eng.dtype), len(idx)), max_num_segments)
            sel = torch.tensor(idx)
            out_f.append(f[idx] if len(idx) != T else f)
            out_0.append(a0[i][idx] if len(idx) != T else a0[i])
            out_1.append(a1[i][idx] if len(idx) != T else a1[i])
            new_sizes.append(len(idx))
            sel_all.append(sel)
            seg_all.append(torch.tensor(segi))
        return torch.cat(out_f, 0), new_sizes, [torch.cat(out_0, 0), torch.cat(out_1, 0)], sel_all, seg_all

    # ---- config.tdc_feature_inputs ----------------------------------------------------------------------------------
    def _feature_sets(self, images, image_sizes, bsz):
        """`images` under config.tdc_feature_inputs -> one features.FeatureSet per sample.  Videos: images[0] / images[1] are
        lists, entry i the [T, tokens, width] rows of sample i (or a FeatureSet in images[0][i], images[1][i] None); single
        images: two [bsz, tokens, width] tensors.  A width that is not the tower's raises ValueError here, before any launch."""
        towers = self.get_model().get_vision_tower_aux_list()
        widths = (towers[0].hidden_size, towers[-1].hidden_size)
        out = []
        for i in range(bsz):
            s = images[0][i]
            d = images[1][i] if len(images) > 1 and images[1] is not None else None
            if is_feature_set(s):
                if d is not None:
                    raise ValueError("config.tdc_feature_inputs: images[0][%d] is a FeatureSet, images[1][%d] must be None" % (i, i))
                fs = s
            else:
                if not (torch.is_tensor(s) and torch.is_tensor(d)):
                    raise ValueError("config.tdc_feature_inputs: sample %d needs a FeatureSet or the two towers' feature tensors" % i)
                if s.dim() == 2:
                    s, d = s.unsqueeze(0), d.unsqueeze(0)
                fs = FeatureSet(s, d, image_sizes[i])
            for name, x, w in (("SigLIP", fs.siglip, widths[0]), ("DINOv2", fs.dino, widths[1])):
                if x.shape[-1] != w:
                    raise ValueError("config.tdc_feature_inputs: the %s features of sample %d are %d wide, the tower's "
                                     "hidden_size is %d" % (name, i, x.shape[-1], w))
            out.append(fs)
        return out

    # ---- the hot path ---------------------------------------------------------------------------------------------
    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels,
                                             images, image_aux_attention_masks_list=None, image_sizes=None,
                                             video_indices=None, prompts=None, audios=None):
        """tdc/cambrian_arch.py:864-1844.  Returns the reference's 10-tuple."""
        model = self.get_model()
        towers = model.get_vision_tower_aux_list()
        if towers is None or images is None or input_ids.shape[1] == 1:
            return (input_ids, position_ids, attention_mask, past_key_values, None, labels, None, None, None, None)
        frame_inputs = model.tdc_frame_inputs()      # config.tdc_frame_inputs: `images` holds decoded uint8 frames
        feature_inputs = model.tdc_feature_inputs()  # config.tdc_feature_inputs: `images` holds stored tower features
        return_aux = model.tdc_return_aux()          # config.tdc_return_aux: slots 6 / 7 / 9 of the 10-tuple
        if feature_inputs:
            feature_sets = self._feature_sets(images, image_sizes, input_ids.shape[0])      # validated before any engine call
        eng = model.tdc_engine()
        vcache = model.tdc_video_cache()             # config.tdc_video_cache_bytes (validated even when no video comes)
        batch_frames = model.tdc_batch_frames()      # config.tdc_batch_frames (0: every sample on its own)
        batch_prompts = model.tdc_batch_prompts()    # config.tdc_batch_prompts (0: every sample on its own)
        pad_fraction = model.tdc_prompt_pad_fraction()
        cfgd = self._cfg()
        K = cfgd.get("context_token_num", 16)
        if feature_inputs or frame_inputs:
            is_video = isinstance(images[0], (list, tuple))
        else:
            is_video = type(images[0]) is list or images[0].ndim == 5
        bsz = input_ids.shape[0]
        # every integer decision below (text lengths, <image> positions, which rows survive the mask) is taken on ONE host copy of
        # the ids / mask: a device-side torch.where(...).tolist() waits for everything queued on the stream - the previous
        # video's encode when calls follow each other
        ids_host = input_ids.detach().cpu()
        mask_host = None if attention_mask is None else attention_mask.detach().cpu().bool()
        visual = []          # per sample: [n_tokens, H] tensor on the engine device
        spliced = []         # per sample: `visual[i]` already holds the text rows around the visual tokens
        final_size = []
        aux_out = []         # config.tdc_return_aux: per sample the dict VideoEncoder.connector(aux=) filled

        def facts(i):
            """the host-side facts of sample i: its source (encode.py: what its frames are read from) with the engine's entries
            for that input kind, text lengths, prompt ids, audio, a21 hand-off, frame cap"""
            if feature_inputs:
                # config.tdc_feature_inputs: the towers ran when the set was exported (a set made of bare tensors carries no
                # signature to compare)
                fs = feature_sets[i]
                src, side_stream = FeatureSource(fs), False
                kw = dict(check_signature=fs.signature is not None)
                entry = lambda *a, **k: eng.encode_features(fs, *a, **kw, **k)
                entry_prompts = lambda qs, **k: eng.encode_features_prompts(fs, qs, **kw, **k)
            elif frame_inputs:
                # config.tdc_frame_inputs: a1 first, then only the kept frames are uploaded and resized
                kw = dict(cache=vcache, image_size=None if image_sizes is None else tuple(image_sizes[i]))
                src, side_stream = FrameSource(images[0][i] if is_video else images[0][i:i + 1], **kw), True
                entry, entry_prompts = (lambda *a, **k: eng.encode_frames(src.frames, *a, **kw, **k)), None
            else:
                vid_s, vid_d = (images[0][i], images[1][i]) if is_video else (images[0][i:i + 1], images[1][i:i + 1])
                if vid_s.ndim == 3:
                    vid_s, vid_d = vid_s.unsqueeze(0), vid_d.unsqueeze(0)
                src, side_stream = PixelSource(vid_s, vid_d, tuple(image_sizes[i]), vcache), True
                kw = {} if vcache is None else {"cache": vcache}                  # config.tdc_video_cache_bytes
                px = lambda: (vid_s.to(eng.dev), vid_d.to(eng.dev), src.image_size)      # uploaded when the sample is encoded
                if is_video:
                    entry = lambda *a, **k: eng.encode_video(*px(), *a, **kw, **k)
                else:       # single images: every image is a static frame, no segmentation / Q-Former (cambrian_arch.py:980-983)
                    entry = lambda *a, **k: encode_source(eng, PixelSource(*px(), vcache), *a, **k)
                entry_prompts = lambda qs, **k: eng.encode_video_prompts(*px(), qs, **kw, **k)
            cur_ids = ids_host[i]
            if mask_host is not None:
                cur_ids = cur_ids[mask_host[i] | (cur_ids == IMAGE_TOKEN_INDEX)]
            n_text = int((cur_ids != IMAGE_TOKEN_INDEX).sum())
            prompt_ids = None
            if is_video and cfgd.get("text_input", True):
                prompt = prompts[i] if prompts is not None else None
                if isinstance(prompt, str):
                    if model.bert_tokenizer is None:
                        raise RuntimeError("model.bert_tokenizer is not set (the reference loads "
                                           "./checkpoints/bert-base-uncased, tdc/cambrian_arch.py:405)")
                    prompt_ids = model.bert_tokenizer(prompt, padding="longest", truncation=True, max_length=256,
                                                      return_tensors="pt").input_ids[0].tolist()
                elif prompt is not None:
                    prompt_ids = [int(x) for x in prompt]      # pre-tokenised BERT ids
            audio = None
            if audios is not None and audios[i] is not None:
                # {"beats_windows": [BEATs features of the consecutive 10-s windows, [1, n, 768] each]} or
                # {"audio_tokens": [T, 50, 768]} (already interleaved); the BEATs encoder itself is not part of the path
                audio = audios[i]
                if not isinstance(audio, dict):
                    audio = {"audio_tokens": audio.to(eng.dev)}
                elif audio.get("audio_pcm") is not None:
                    # a decoder's PCM track (audio.PcmAudio): resampled to the 16 kHz waveform once, here, so the same-video
                    # grouping and every entry below see {"audio_wav": ...} (a clash with another key raises ValueError)
                    audio = normalize_audio(eng, audio)
                    eng.beats = model.tdc_beats()
                elif audio.get("audio_wav") is not None and audio.get("beats_windows") is None \
                        and audio.get("audio_tokens") is None:
                    # the reference's own audio dict (cambrian_arch.py:1547): raw waveform -> BEATs on the device
                    eng.beats = model.tdc_beats()
            f = dict(i=i, src=src, entry=entry, entry_prompts=entry_prompts, side_stream=side_stream, n_text=n_text,
                     prompt_ids=prompt_ids, audio=audio, splice=None)
            if is_video:
                # a21 hand-off: when embed_tokens lives on the engine device in the engine dtype the
                # emission gather also fetches the text embeddings and writes the inputs_embeds rows directly
                emb_w = getattr(getattr(model, "embed_tokens", None), "weight", None)
                pos_img = torch.where(cur_ids == IMAGE_TOKEN_INDEX)[0].tolist()
                if (getattr(self, "tdc_prefill_handoff", True) and emb_w is not None and emb_w.is_cuda
                        and emb_w.device == eng.dev and emb_w.dtype == eng.dtype and len(pos_img) == 1):
                    f["splice"] = {"table": emb_w, "before": cur_ids[:pos_img[0]].tolist(),
                                   "after": cur_ids[pos_img[0] + 1:].tolist()}
                # video_indices[i]: 0/1 per second of audio, 1 where a frame was decoded (cambrian_arch.py:916-926); [None]
                # (what generate() passes) / None: input frame t is second t
                f["vindex"] = video_indices[i] if video_indices is not None and i < len(video_indices) else None
                f["cap"] = model.tdc_frame_cap()
                f["btl"] = self._budget_text_len(ids_host[i])
                f["sharded"] = model.tdc_sharded_engine()
            return f

        def encode_one(f):
            """sample f through the engine on its own -> (visual tokens, spliced, final sizes)"""
            src, n_text, prompt_ids, audio, splice = (f[k] for k in ("src", "n_text", "prompt_ids", "audio", "splice"))
            keep = {}
            akw = {}
            if return_aux:      # the keyword goes down only when the key is on
                aux_out.append({})
                akw = {"aux": aux_out[-1]}
            if not is_video:
                vis = f["entry"](None, n_text, None, image=True, info=keep, **akw)
            elif f["sharded"] is not None:
                # config.tdc_shard_frames under an initialised torch.distributed (one process per GPU, every rank called
                # with the same video - how the reference's eval drivers start their workers, eval/eval_mlvu.py:129-157 -
                # but here the ranks split the FRAMES of the one video): this rank encodes frames [lo, hi) of the a1
                # selection, dist.ShardedVideoEncoder exchanges what crosses the rank boundaries and all-gathers the
                # emitted tokens, so every rank returns the same 10-tuple as the serial path, bit for bit.  The serial frame
                # cache (config.tdc_video_cache_bytes) is not used here; config.tdc_shard_cache_bytes gives each rank a
                # cache of its own frames (tdc_shard_cache)
                vid_s, vid_d = src.px_siglip, src.px_dino
                fp = f["sharded"].frame_plan(src.T0, f["btl"], f["cap"], f["vindex"])
                eng.two_streams = model.tdc_side_stream(fp["hi"] - fp["lo"])
                sel_s = torch.as_tensor(fp["siglip_frames"], dtype=torch.long, device=vid_s.device)
                sel_d = torch.as_tensor(fp["dino_frames"], dtype=torch.long, device=vid_d.device)
                vis = f["sharded"].encode_video(vid_s[sel_s].to(eng.dev), vid_d[sel_d].to(eng.dev), fp["T"], src.image_size,
                                                n_text, prompt_ids, audio=audio, sample_indices=fp["sample_indices"],
                                                cache=model.tdc_shard_cache(), info=keep)
                keep["final_size"] = [seg.unpad_newline_map(eng.side, src.image_size, 0)[1]] * fp["T"]
                splice = None
            else:
                if f["side_stream"]:
                    eng.two_streams = model.tdc_side_stream(min(src.T0, f["cap"]))
                vis = f["entry"](f["btl"], n_text, prompt_ids, audio=audio, frame_cap=f["cap"], splice=splice,
                                 video_index=f["vindex"], info=keep, **akw)
            return vis, splice is not None, keep["final_size"]

        def encode_group(fs, n_frames):
            """config.tdc_batch_frames: the samples fs in one tower and connector pass (VideoEncoder.encode_batch) -> what
            encode_one returns for each, bit for bit"""
            infos = [{} for _ in fs]
            samples = [dict(px_siglip=f["src"].px_siglip, px_dino=f["src"].px_dino, image_size=f["src"].image_size,
                            image=not is_video, budget_text_len=f.get("btl"), n_text_tokens=f["n_text"], prompt_ids=f["prompt_ids"],
                            audio=f["audio"], video_index=f.get("vindex"), splice=f["splice"]) for f in fs]
            eng.two_streams = model.tdc_side_stream(n_frames)
            vis = eng.encode_batch(samples, frame_cap=model.tdc_frame_cap(), infos=infos)
            return [(v, f["splice"] is not None, info["final_size"]) for v, f, info in zip(vis, fs, infos)]

        def encode_prompts(fs):
            """config.tdc_batch_prompts: the samples fs carry ONE video (same_source_key) - its front once, one compressor pass
            per group of prompts (the engine's multi-prompt entry for the input kind) -> what encode_one returns for each, bit
            for bit"""
            f0 = fs[0]
            infos = [{} for _ in fs]
            qs = [dict(budget_text_len=f["btl"], n_text_tokens=f["n_text"], prompt_ids=f["prompt_ids"], splice=f["splice"])
                  for f in fs]
            if f0["side_stream"]:
                eng.two_streams = model.tdc_side_stream(min(f0["src"].T0, f0["cap"]))
            vis = f0["entry_prompts"](qs, audio=f0["audio"], frame_cap=f0["cap"], video_index=f0["vindex"], infos=infos,
                                      max_prompts=batch_prompts, pad_fraction=pad_fraction)
            return [(v, f["splice"] is not None, info["final_size"]) for v, f, info in zip(vis, fs, infos)]

        if batch_prompts and bsz > 1 and is_video:
            # config.tdc_batch_prompts: every sample's host-side facts first, then the samples that carry the same video (in
            # order of its first sample) through encode_prompts; a video that only one sample carries runs encode_one
            fs = [facts(i) for i in range(bsz)]
            same = {}
            for f in fs:
                same.setdefault(same_source_key(eng, f["src"], f["btl"], f["cap"], f["audio"], f["vindex"]), []).append(f)
            results = [None] * bsz
            for members in same.values():
                rs = [encode_one(members[0])] if len(members) == 1 else encode_prompts(members)
                for f, r in zip(members, rs):
                    results[f["i"]] = r
        elif not batch_frames or bsz == 1:
            results = (encode_one(facts(i)) for i in range(bsz))
        else:
            # config.tdc_batch_frames: every sample's host-side facts first (the same exceptions as the loop above, raised
            # before any encode), then the groups of batch_groups in sample order; a group of one runs encode_one
            fs = [facts(i) for i in range(bsz)]
            fr = [len(frame_indices(eng.cfg, f["src"].T0, f["btl"], f["cap"])) if is_video else 1 for f in fs]
            geo = [tuple((tuple(px.shape[1:]), px.dtype, px.device) for px in (f["src"].px_siglip, f["src"].px_dino)) for f in fs]
            results = []
            for g in batch_groups(fr, batch_frames, geo):
                results += [encode_one(fs[g[0]])] if len(g) == 1 else encode_group([fs[i] for i in g], sum(fr[i] for i in g))
        for vis, sp, fsz in results:
            visual.append(vis)
            spliced.append(sp)
            final_size.extend(fsz)
        # ---- a21: splice text embeddings and visual tokens, truncate, pad (cambrian_arch.py:1425-1495, :1712-1844)
        _labels, _position_ids, _attention_mask = labels, position_ids, attention_mask
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids, dtype=torch.bool)
        else:
            attention_mask = attention_mask.bool()
        if position_ids is None:
            position_ids = torch.arange(0, input_ids.shape[1], dtype=torch.long, device=input_ids.device)
        if labels is None:
            labels = torch.full_like(input_ids, IGNORE_INDEX)
        attention_mask = attention_mask | (input_ids == IMAGE_TOKEN_INDEX)
        keep_host = torch.ones_like(ids_host, dtype=torch.bool) if mask_host is None else \
            (mask_host | (ids_host == IMAGE_TOKEN_INDEX))
        embed = model.embed_tokens
        new_embeds, new_labels = [], []
        for i in range(bsz):
            if bool(keep_host[i].all()):
                ids, lab, ids_h = input_ids[i], labels[i], ids_host[i]
            else:           # integer row indices made on the host: a boolean mask on the device would wait for its own count
                rows = torch.nonzero(keep_host[i])[:, 0]
                ids, lab, ids_h = input_ids[i][rows.to(input_ids.device)], labels[i][rows.to(labels.device)], ids_host[i][rows]
            img_pos = torch.where(ids_h == IMAGE_TOKEN_INDEX)[0].tolist()
            vis = visual[i]
            if not img_pos:
                new_embeds.append(torch.cat([embed(ids), vis[0:0].to(embed.weight.dtype)], 0))
                new_labels.append(lab)
                continue
            if len(img_pos) != 1:
                # The reference takes one entry of its per-video feature list per <image> token (cur_image_idx,
                # tdc/cambrian_arch.py:1457-1495, :1712-1727) while that list holds one entry per sample: a sample with
                # several <image> tokens runs off its end.  Same exception type here.
                raise IndexError("list index out of range: %d <image> tokens in sample %d, one video / image per sample "
                                 "(tdc/cambrian_arch.py:1716)" % (len(img_pos), i))
            p = img_pos[0]
            if spliced[i]:
                n_vis = vis.shape[0] - (ids.shape[0] - 1)
                new_embeds.append(vis)
                new_labels.append(torch.cat([lab[:p], torch.full((n_vis,), IGNORE_INDEX, device=lab.device,
                                                                 dtype=lab.dtype), lab[p + 1:]]))
                continue
            text = embed(torch.cat([ids[:p], ids[p + 1:]]))
            vis = vis.to(text.dtype).to(text.device)
            new_embeds.append(torch.cat([text[:p], vis, text[p:]], 0))
            new_labels.append(torch.cat([lab[:p], torch.full((vis.shape[0],), IGNORE_INDEX, device=lab.device,
                                                             dtype=lab.dtype), lab[p + 1:]]))
        mx = getattr(self.config, "tokenizer_model_max_length", None)
        if mx is not None:
            new_embeds = [x[:mx] for x in new_embeds]
            new_labels = [x[:mx] for x in new_labels]
        max_len = max(x.shape[0] for x in new_embeds)
        left = getattr(self.config, "tokenizer_padding_side", "right") == "left"
        emb_pad = []
        lab_pad = torch.full((bsz, max_len), IGNORE_INDEX, dtype=new_labels[0].dtype, device=new_labels[0].device)
        att = torch.zeros((bsz, max_len), dtype=attention_mask.dtype, device=attention_mask.device)
        pos = torch.zeros((bsz, max_len), dtype=position_ids.dtype, device=position_ids.device)
        for i, (e, l) in enumerate(zip(new_embeds, new_labels)):
            n = e.shape[0]
            if n == max_len:            # nothing to pad (always so for one sample): no 2 x 650-MB copy of a T = 512 stream
                emb_pad.append(e)
            else:
                z = torch.zeros((max_len - n, e.shape[1]), dtype=e.dtype, device=e.device)
                emb_pad.append(torch.cat((z, e), 0) if left else torch.cat((e, z), 0))
            if n > 0:
                sl = slice(max_len - n, max_len) if left else slice(0, n)
                lab_pad[i, sl] = l
                att[i, sl] = True
                pos[i, sl] = torch.arange(0, n, dtype=pos.dtype, device=pos.device)
        new_input_embeds = emb_pad[0].unsqueeze(0) if bsz == 1 else torch.stack(emb_pad, 0)
        new_labels_out = None if _labels is None else lab_pad
        att_out = None if _attention_mask is None else att.to(dtype=_attention_mask.dtype)
        pos_out = None if _position_ids is None else pos
        aux_feats = aux_masks = aux_ctx = None
        if return_aux:      # per tower / overall: the samples' rows in sample order along dim 0 (cambrian_arch.py:678-683, 1300-1303)
            def cat(xs):
                return xs[0] if len(xs) == 1 else torch.cat(xs, 0)
            aux_feats = [cat([d["features"][i] for d in aux_out]) for i in range(2)]
            aux_masks = [cat([d["masks"][i] for d in aux_out]) for i in range(2)]
            aux_ctx = cat([d["global_context"] for d in aux_out])
        return (None, pos_out, att_out, past_key_values, new_input_embeds, new_labels_out, aux_feats, aux_masks, final_size,
                aux_ctx)

    def initialize_vision_tokenizer(self, model_args, tokenizer):
        raise NotImplementedError("tokenizer surgery for training (tdc/cambrian_arch.py:1846-1898) is out of scope")
