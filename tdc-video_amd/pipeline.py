"""VideoEncoder: the hot path (stages S0-S10) as a sequence of libtdc_hip.so launches.

Python only sequences kernels and owns the buffers (torch tensors as device memory); every FLOP runs in the HIP
library.  Stage methods mirror the reference's stages so the parity tests can compare stage by stage:
  tower()        a2-a4   tdc/multimodal_encoder/{siglip,dino}_encoder.py + HF ViTs
  frame_sims()   a5      tdc/cambrian_arch.py:832-842
  connector()    a6-a10  tdc/cambrian_arch.py:1002-1053 (aux projectors, SVA), :1149-1150 (mm_projector), :1176-1293
  compress()     a11-a19 tdc/cambrian_arch.py:1507-1709 (all chunks of a video batched into ONE Q-Former pass)
"""
import math

import torch

from . import lib as L
from . import ops
from . import preprocess
from . import segment as seg
from . import weights as Wt
# the orchestration over an engine (encode.py): what the methods below call, and the names this module has always offered
from .encode import (batch_groups, cached_audio, compact_features_with, compress_many_with, compress_with, emission_plan,  # noqa: F401
                     encode_batch_with, encode_features_prompts_with, encode_features_with, encode_frames_prompts_with,
                     encode_frames_with, encode_image_cached, encode_missing, encode_video_cached, encode_video_prompts_with,
                     encode_video_with, export_features_from_frames_with, export_features_with, frame_indices, gather_frames,
                     join_side_tower, precise_features, prompt_groups, prompt_maps, same_video_key, sample_indicator,
                     select_segments_with, start_side_tower, text_prompt, visual_budget)
from .weights import pad64

ACT_CODES = {"gelu_tanh": L.ACT_GELU_TANH, "gelu_erf": L.ACT_GELU_ERF, "swiglu": L.ACT_SWIGLU}


def _lin(l):
    return L.Lin(l.w.data_ptr(), l.b.data_ptr() if l.b is not None else None, l.w.shape[0], l.w.shape[1])


class _LRU(dict):
    """Small bounded cache for the host-built index / mask / prompt tables (keys: geometry or prompt-id tuples): a server that
    sees many prompts and resolutions does not grow host and device memory without bound; the least recently used entry
    leaves when the 33rd arrives."""

    def __init__(self, maxsize=32):
        super().__init__()
        self.maxsize = maxsize

    def _touch(self, key):
        v = dict.pop(self, key)
        dict.__setitem__(self, key, v)          # dicts keep insertion order: the last entry is the most recent
        return v

    def get(self, key, default=None):
        return self._touch(key) if key in self else default

    def __getitem__(self, key):
        return self._touch(key)

    def __setitem__(self, key, value):
        if key in self:
            dict.pop(self, key)
        dict.__setitem__(self, key, value)
        while len(self) > self.maxsize:
            dict.pop(self, next(iter(self)))


class VideoEncoder:
    """defaults first: what __init__ may leave unset, and what encoders assembled field by field (tests) do not set"""
    native_towers = True          # towers through the C++ composite tdc_vit_fwd (per-kernel Python path when False)
    native_connector = True       # a6-a9 through tdc_connector_fwd
    native_qformer = True         # Q-Former through the C++ composite tdc_qformer_fwd
    # cross-attention block of the Q-Former: 2 = one kernel per layer (tdc_qformer_xattn), 1 = q GEMM + tdc_attention,
    # then output projection + residual + LayerNorm in one kernel, 0 = per-kernel sequence; applies when the shape allows it
    # (bert-base width, K % 16 == 0; mode 2 also Nenc % 4 == 0, Nenc <= 224)
    xattn_mode = 1
    two_streams = False
    tower_res_dtype = None
    beats = None                  # beats.BeatsEncoder for raw-waveform audio input
    selection_eps = None
    selection_max_fraction = 0.125
    frame_towers = (preprocess.SIGLIP, preprocess.DINOV2)      # {R, mean, std} per tower for the frame entries (section 15)
    frame_slab = 64               # frames per resize launch of pixels_from_frames (bounds its scratch; not the result)
    _tower_dtype = _conn_struct = _qf_struct = _tower_stream = _side_stream = _feature_sig = None

    def __init__(self, sd, cfg, dtype=torch.float16, device="cuda", siglip_heads=16, dino_heads=24,
                 qformer_heads=12, tower_batch=None, fp8_towers=False, tower_dtype=None, ln_fuse=False,
                 tower_res_dtype=None, dino_dtype=None, selection_refine=None, selection_eps=1e-3, selection_max_fraction=0.125,
                 frame_towers=None):
        """sd: reference-named state dict without the leading 'model.'; cfg: dict of reference config keys.
        dtype: 16-bit type of the connector, the Q-Former and every tensor handed to the caller; tower_dtype (default:
        dtype): 16-bit type of the two ViT towers - their last kernel (the token-grid resample) writes `dtype` rows.  bf16
        towers under an fp16 connector / compressor keep the compressed tokens within 1e-3 of the fp32 reference arithmetic (measured
        1.0e-4 at full depth; all-bf16: 6e-4 ... 2e-3): the 16-bit error of the context tokens is made behind the towers.
        dino_dtype (default: tower_dtype): operand type of the DINOv2 tower alone.  Its features alone drive the a5 segment
        selection (tdc/cambrian_arch.py:832-849): fp16 there keeps the adjacent-frame similarities at the reference's own
        precision (3.4e-5 instead of 4.2e-4 with bf16 operands) while SigLIP stays in tower_dtype.
        selection_refine (None = automatic: on when the DINOv2 operands are bf16 and not e4m3) / selection_eps: the a5 segment
        selection at the reference's precision under bf16 DINOv2 operands.  bf16 similarities are within selection_eps of the fp16
        tower's (measured 1.7e-4 ... 5.0e-4; default bound 1e-3); when the ranks that decide the selection are closer than
        4 selection_eps, the pairs inside the band [v_n+1 - 2 eps, v_n + 2 eps] - and only they - are re-encoded by a second, fp16-operand copy of the DINOv2
        tower (+2.2 GB of weights) and re-ranked (segment.selection_band / select_refined): exactly what ranking the fp16 tower's
        similarities selects.  A video whose decisive ranks are further apart (the bench's: 0.43) pays nothing; a band whose
        frames exceed max(8, selection_max_fraction x frames) - a plateau of near-identical similarities at the decisive rank, where
        the reference's own fp16 similarity values tie - is left to the fast tower's ranking (segment.band_allowed).
        fp8_towers (BASELINE config 5): the towers' LayerNorms emit e4m3 rows with per-row scales and the qkv / fc1 GEMMs
        run on fp8 operands (v_mfma_f32_16x16x128_f8f6f4); everything else stays in `tower_dtype`.
        ln_fuse: the towers' pre-LayerNorms folded into the neighbouring GEMMs (weights.ln_fusion_enabled; off by default).
        tower_batch: frames per tower launch sequence; None (default) = all frames of the call up to TOWER_BATCH_MAX, halved
        until the tower workspace fits the free HBM (`auto_tower_batch`) - the result does not depend on it, bit for bit
        (tests: test_batch_invariance_and_determinism), the rate does (512 / 256 / 128 / 64 frames: 428.8 / 425.7 / 420.1 /
        407.6 frames/s, profiles/r04_tower_batch.log).  The reference's own chunk is 64 (tdc/cambrian_arch.py:698-745).
        tower_res_dtype: type of the towers' residual stream in HBM - None / torch.float32: fp32 (the out-projection / fc2
        epilogues read-modify-write 8 B per element); torch.float16 (or bfloat16): that 16-bit type - 4 B per element, half
        the LayerNorm input bytes, sums formed in fp32 and rounded once per residual add.  fp16 is the reference's own
        arithmetic (its HF towers run under torch_dtype=float16, tdc/builder.py:69).  Composes with fp8_towers (round 6) and, when the
        operands have the stream's type, with ln_fuse.
        frame_towers: what the frame entries (pixels_from_frames, encode_frames ...) resize decoded frames to - a pair of
        dicts {R, mean, std}, SigLIP's then DINOv2's; default (preprocess.SIGLIP, preprocess.DINOV2): 384 / 378 px."""
        self.cfg = dict(cfg)
        if frame_towers is not None:
            self.frame_towers = tuple(frame_towers)
        self.tower_res_dtype = None if tower_res_dtype in (None, torch.float32) else tower_res_dtype
        assert self.tower_res_dtype in (None, torch.float16, torch.bfloat16)
        # the LayerNorm fold over a 16-bit stream: the consumer GEMMs read the stream itself as their A operand, so the
        # operands of both towers have the stream's type
        assert not (ln_fuse and self.tower_res_dtype is not None) or \
            (tower_dtype or dtype) == self.tower_res_dtype == (dino_dtype or tower_dtype or dtype), \
            "ln_fuse over a 16-bit residual stream needs tower operands of the stream's type"
        self.dtype, self.dev = dtype, torch.device(device)
        self._tower_dtype = tower_dtype = dtype if tower_dtype is None else tower_dtype
        self.tower_batch = tower_batch
        self.qheads = qformer_heads
        s_sd = Wt._strip(sd, "vision_tower_aux_list.0.vision_tower.")
        d_sd = Wt._strip(sd, "vision_tower_aux_list.1.vision_tower.")
        self.towers = {}
        if s_sd:
            self.towers["siglip"] = Wt.prep_siglip(s_sd, siglip_heads, tower_dtype, self.dev, fp8=fp8_towers, ln_fuse=ln_fuse)
        if d_sd:
            self.towers["dino"] = Wt.prep_dino(d_sd, dino_heads, dino_dtype or tower_dtype, self.dev, fp8=fp8_towers,
                                               ln_fuse=ln_fuse)
        for t in self.towers.values():
            t["dtype"] = dino_dtype or tower_dtype if t.kind == "dino" else tower_dtype
        # a5 at the reference's precision under bf16 DINOv2 operands: a second, fp16-operand DINOv2 tower for the pairs whose
        # similarities decide the selection (select_segments_with, on the serial and the sharded path)
        if selection_refine is None:
            selection_refine = bool(d_sd) and (dino_dtype or tower_dtype) == torch.bfloat16 and not fp8_towers
        if selection_refine and d_sd and (dino_dtype or tower_dtype) != torch.float16:
            tp = Wt.prep_dino(d_sd, dino_heads, torch.float16, self.dev)
            tp["dtype"] = torch.float16
            # its residual stream: fp16 (the reference's arithmetic) when the engine's is 16-bit, else the engine's fp32
            tp["res_dtype"] = torch.float16 if self.tower_res_dtype is not None else None
            self.towers["dino_precise"] = tp
            self.selection_eps = float(selection_eps)
        self.selection_max_fraction = float(selection_max_fraction)
        self.c = Wt.prep_connector(sd, cfg, dtype, self.dev)
        tok = cfg.get("mm_vision_tower_aux_token_len_list", [576, 576])
        self.out_grid = [int(round(t ** 0.5)) for t in tok]
        self.side = int(round(cfg.get("query_num_list", [144])[0] ** 0.5))
        self._tables = _LRU(32)
        self.K = cfg.get("context_token_num", 16)
        self.H = cfg["hidden_size"]

    @property
    def tower_dtype(self):
        return self._tower_dtype or self.dtype

    def _tdt(self, t):
        """operand type of tower `t` (its weights' type): tower_dtype unless dino_dtype set the DINOv2 tower apart"""
        return t.get("dtype") or self.tower_dtype

    def _res_dtype(self, t):
        """type of tower `t`'s residual stream: its own "res_dtype" (the precise DINOv2 copy) or the engine's; None = fp32"""
        return t["res_dtype"] if "res_dtype" in t else self.tower_res_dtype

    # ------------------------------------------------------------------------------------------------ towers
    def _bil(self, n_in, n_out):
        key = (n_in, n_out)
        if key not in self._tables:
            self._tables[key] = ops.bilinear_tables(n_in, n_out, self.dev)
        return self._tables[key]

    def tower(self, name, px):
        """px [B,3,H,W] (fp32, fp16 or bf16) -> features [B*g*g, pad64(D)] 16-bit `dtype` (g = 24)."""
        t = self.towers[name]
        out_grid = self.out_grid[0 if name == "siglip" else 1]      # "dino" / "dino_precise": the second entry
        outs = []
        tb = int(self.tower_batch) if self.tower_batch else self.auto_tower_batch(t, px)
        for s in range(0, px.shape[0], tb):
            outs.append(self._tower_batch(t, px[s:s + tb].contiguous(), out_grid))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    TOWER_BATCH_MAX = 512      # the largest batch measured (profiles/r04_tower_batch.log); one 512-frame batch needs ~15 GB

    def auto_tower_batch(self, t, px, free_bytes=None):
        """Frames per tower batch when the caller gave none: min(frames, TOWER_BATCH_MAX), halved until tdc_vit_workspace_bytes
        fits 60 % of the HBM this process can still get (free on the device + what torch's allocator holds unused + the
        workspace it would replace).  free_bytes: override of that figure (tests)."""
        import ctypes as C
        B = max(1, min(int(px.shape[0]), self.TOWER_BATCH_MAX))
        if len(t.layers) == 0 or not px.is_cuda:
            return B
        Hpx, Wpx = int(px.shape[2]), int(px.shape[3])
        m = self._vit_struct(t, Hpx // t.patch, Wpx // t.patch)[0]
        lib = L.load()
        if free_bytes is None:
            free, _total = torch.cuda.mem_get_info(self.dev)
            unused = torch.cuda.memory_reserved(self.dev) - torch.cuda.memory_allocated(self.dev)
            ws = vars(self).get(self._vit_ws_key(t))
            free_bytes = free + max(0, unused) + (ws.numel() if ws is not None else 0)
        budget = 0.6 * free_bytes
        while B > 1 and lib.tdc_vit_workspace_bytes(C.byref(m), B, Hpx, Wpx) > budget:
            B = (B + 1) // 2
        return B

    def _workspace(self, key, nbytes):
        """the native composite's device workspace in attribute `key`, grown to nbytes (kept for the engine's life)"""
        ws = vars(self).get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            setattr(self, key, ws)
        return ws

    def _vit_ws_key(self, t):       # one workspace per tower when the towers run concurrently on two streams
        return "_vit_ws_" + t.kind if self.two_streams else "_vit_ws"

    # ---- native composite (csrc/api.cpp: tdc_vit_fwd): the whole tower batch is one C call ------------------------------
    def _vit_struct(self, t, gh, gw):
        """ctypes mirror of tdc_vit_model for tower `t` on a gh x gw patch grid (cached; keeps the arrays alive)."""
        import ctypes as C
        cache = t.setdefault("_c_structs", {})
        if (gh, gw) in cache:
            return cache[(gh, gw)]
        pos, cls_row = Wt.tower_pos(t, gh, gw, self.dev)
        layers = (L.VitLayer * len(t.layers))()
        zeros = None
        if t.get("fp8"):    # one zero ln_c1 vector long enough for every lin of the tower (tdc_vit_layer.zeros)
            zn = max(l.w.shape[0] for Lr in t.layers for l in (Lr.qkv, Lr.out, Lr.fc1, Lr.fc2))
            zeros = t.setdefault("_zeros", torch.zeros(zn, dtype=torch.float32, device=self.dev))
        for i, Lr in enumerate(t.layers):
            layers[i] = L.VitLayer(Lr.ln1_g.data_ptr(), Lr.ln1_b.data_ptr(), Lr.ln2_g.data_ptr(), Lr.ln2_b.data_ptr(),
                                   _lin(Lr.qkv), _lin(Lr.out), _lin(Lr.fc1), _lin(Lr.fc2),
                                   Lr.qkv_c1.data_ptr() if Lr.qkv_c1 is not None else None,
                                   Lr.fc1_c1.data_ptr() if Lr.fc1_c1 is not None else None,
                                   Lr.qkv.wscale or 0.0, Lr.fc1.wscale or 0.0,
                                   zeros.data_ptr() if zeros is not None else None,
                                   Lr.out.wscale or 0.0, Lr.fc2.wscale or 0.0, Lr.fc1.w2max, Lr.fc1.bmax)
        m = L.VitModel()
        m.dtype, m.out_dtype_p1 = ops._dtcode(self._tdt(t)), ops._dtcode(self.dtype) + 1
        rd = self._res_dtype(t)
        m.res_dtype_p1 = 0 if rd is None else ops._dtcode(rd) + 1
        m.dim, m.heads, m.head_dim, m.n_layers, m.patch, m.has_cls = t.dim, t.heads, t.head_dim, len(t.layers), t.patch, \
            t.has_cls
        m.act = ACT_CODES[t.act]
        m.eps = t.eps
        m.patch_lin = _lin(t.patch_lin)
        m.pos, m.ldpos = pos.data_ptr(), pos.stride(0)
        m.cls_row = cls_row.data_ptr() if cls_row is not None else None
        fl = t.get("final_ln")
        m.lnf_g, m.lnf_b = (fl[0].data_ptr(), fl[1].data_ptr()) if fl else (None, None)
        m.layers_host = layers
        m.fused = int(bool(t.fused))
        m.fp8 = int(t.get("fp8") or 0)
        cache[(gh, gw)] = (m, layers, pos, cls_row)
        return cache[(gh, gw)]

    def _tower_batch_native(self, t, px, out_grid):
        import ctypes as C
        B, _, H, W = px.shape
        assert H == W and px.is_contiguous() and len(t.layers) > 0   # trailing pixels (384 = 27*14 + 6) are dropped: "valid" conv
        g = H // t.patch
        m = self._vit_struct(t, g, g)[0]
        lib = L.load()
        ws = self._workspace(self._vit_ws_key(t), lib.tdc_vit_workspace_bytes(C.byref(m), B, H, W))
        D = t.dim
        out = torch.empty(B * out_grid * out_grid, pad64(D), device=self.dev, dtype=self.dtype)
        i0, i1, fr = self._bil(g, out_grid)
        f32 = ops.px_kind(px, self._tdt(t))
        L.check(lib.tdc_vit_fwd(C.byref(m), ops._ptr(px), f32, B, H, W, out_grid, ops._ptr(i0), ops._ptr(i1),
                                ops._ptr(fr), ops._ptr(out), out.stride(0), ops._ptr(ws), ws.numel(), ops._stream()),
                "tdc_vit_fwd")
        return out

    def _tower_batch(self, t, px, out_grid):
        """One tower batch.  Default: the C++ composite (tdc_vit_fwd).  With `native_towers = False`: the SAME launches issued one
        by one from Python - the form the tests compare the composite with, bit for bit - over either residual stream
        (`tower_res_dtype`: None = fp32, read-modify-written as 8 B per element; a 16-bit type = tdc_vit_model.res_dtype_p1)."""
        if self.native_towers and len(t.layers) > 0:
            return self._tower_batch_native(t, px, out_grid)
        dt, dev = self._tdt(t), self.dev
        rd = self._res_dtype(t)
        s32 = rd is None                         # fp32 residual stream
        B = px.shape[0]
        D, Dp = t.dim, pad64(t.dim)
        patches, gh, gw = ops.im2col(px, t.patch, dt)
        assert gh == gw, "square inputs only (reference pads to square, mm_datautils.py:286-314)"
        P = gh * gw
        S = P + t.has_cls
        pos, cls_row = Wt.tower_pos(t, gh, gw, dev)
        x = torch.empty(B * S, Dp, device=dev, dtype=torch.float32 if s32 else rd)        # the residual stream
        ops.gemm(patches, t.patch_lin.w, t.patch_lin.b, res=pos, r_map=(P, 0, t.has_cls, 1), out=x, out_f32=s32,
                 c_map=(P, S, t.has_cls, 1))
        if t.has_cls:
            (ops.set_rows if s32 else ops.set_rows16)(x, B, S, 0, cls_row)

        def ln(g, b, **kw):                      # LayerNorm of the stream -> 16-bit operand rows (or e4m3 rows + scales)
            return ops.layernorm(x, g, b, t.eps, D, dt, x16_kernel=not s32, **kw)

        def update(a, lin, **kw):                # x <- x + a lin^T + b, in place (fp32: 8 B per element; 16-bit: one rounding)
            if not s32 and "out_dtype" in kw:    # e4m3 operands over the 16-bit stream: C / res are of the stream's type
                kw["out_dtype"] = rd
            return ops.gemm(a, lin.w, lin.b, res=x, out=x, out_f32=s32, **kw)
        h16 = torch.empty(B * S, Dp, device=dev, dtype=dt)
        qkv = torch.empty(B * S, t.layers[0].qkv.w.shape[0], device=dev, dtype=dt) if t.layers else None
        attn = torch.zeros(B * S, Dp, device=dev, dtype=dt)
        act = ACT_CODES[t.act]
        mlp_w = t.layers[0].fc2.w.shape[1] if t.layers else 0
        mlp = torch.empty(B * S, mlp_w, device=dev, dtype=dt) if t.layers else None
        scale = t.head_dim ** -0.5
        # t.fused: the block's LayerNorms are folded into the GEMMs around them - the residual-stream GEMM emits the
        # 16-bit row copy (into h16) and per-slot statistics, the next GEMM folds (mean, rstd) into its epilogue
        fused = bool(t.fused)
        fp8 = int(t.get("fp8") or 0)
        assert s32 or not fused or rd == dt, "the fold over a 16-bit stream reads the stream as the GEMM operand"
        slots = D // 64
        part = torch.empty(slots, B * S, 2, device=dev, dtype=torch.float32) if fused else None
        stats = torch.empty(B * S, 2, device=dev, dtype=torch.float32) if fused else None
        # fp32 stream: the producer also writes the 16-bit row copy the consumer reads; 16-bit stream: the consumer reads the
        # stream itself - only the partials are emitted and no LayerNorm kernel runs inside the layer loop
        emit = dict(x16=h16, ln_part=part) if (fused and s32) else dict(ln_part=part) if fused else {}
        xa = h16 if s32 else x                   # A operand of the folded consumers
        if fp8:     # e4m3 LayerNorm rows (per-row scales in `stats`) for the fp8-operand qkv / fc1 GEMMs
            h8 = torch.empty(B * S, t.layers[0].qkv.w.shape[1], device=dev, dtype=torch.uint8)
            stats = torch.empty(B * S, 2, device=dev, dtype=torch.float32)
        if fp8 >= 2:    # ... and e4m3 copies of the attention output / MLP hidden for out-proj / fc2
            a8 = torch.empty(B * S, t.layers[0].out.w.shape[1], device=dev, dtype=torch.uint8)
            m8 = torch.empty(B * S, t.layers[0].fc2.w.shape[1], device=dev, dtype=torch.uint8)
            mlp_n = t.layers[0].fc1.w.shape[0] // (2 if t.act == "swiglu" else 1)
            mlp_w = max(mlp_w, m8.shape[1])
            mlp = torch.empty(B * S, mlp_w, device=dev, dtype=dt)
        if fp8 >= 3:    # ... the hidden written as e4m3 by fc1 itself, with its row scales in stats2
            stats2 = torch.empty(B * S, 2, device=dev, dtype=torch.float32)
        for li, Lr in enumerate(t.layers):
            if fp8:
                ln(Lr.ln1_g, Lr.ln1_b, y8=h8, y8_stats=stats, y8_wscale=Lr.qkv.wscale)
                ops.gemm(h8, Lr.qkv.w, Lr.qkv.b, out=qkv, ln_stats=stats, ln_c1=Lr.qkv.zeros, out_dtype=dt)
            elif Lr.qkv_c1 is None:
                ln(Lr.ln1_g, Lr.ln1_b, y16=h16)
                ops.gemm(h16, Lr.qkv.w, Lr.qkv.b, out=qkv)
            else:
                ops.gemm(xa, Lr.qkv.w, Lr.qkv.b, out=qkv, ln_stats=stats, ln_c1=Lr.qkv_c1)
            ld = qkv.stride(0)
            ops.attention(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], attn, B, t.heads, t.head_dim, S, S, scale,
                          S * ld, S * ld, S * ld, S * attn.stride(0))
            if fp8 >= 2:
                ops.quantize_rows_fp8(attn, Dp, Lr.out.wscale, y8=a8, stats=stats)
                update(a8, Lr.out, ln_stats=stats, ln_c1=Lr.out.zeros, out_dtype=dt)
            else:
                update(attn, Lr.out, **emit)
            if fused:
                ops.ln_finalize(part, slots, B * S, t.eps, stats)
                ops.gemm(xa, Lr.fc1.w, Lr.fc1.b, act=act, out=mlp, ln_stats=stats, ln_c1=Lr.fc1_c1)
            elif fp8:
                ln(Lr.ln2_g, Lr.ln2_b, y8=h8, y8_stats=stats, y8_wscale=Lr.fc1.wscale)
                if fp8 >= 3:
                    ops.gemm(h8, Lr.fc1.w, Lr.fc1.b, act=act, out=m8, ln_stats=stats, ln_c1=Lr.fc1.zeros, out_dtype=dt,
                             out_stats=stats2, out_w2max=Lr.fc1.w2max, out_bmax=Lr.fc1.bmax, out_wscale=Lr.fc2.wscale)
                else:
                    ops.gemm(h8, Lr.fc1.w, Lr.fc1.b, act=act, out=mlp, ln_stats=stats, ln_c1=Lr.fc1.zeros, out_dtype=dt)
            else:
                ln(Lr.ln2_g, Lr.ln2_b, y16=h16)
                ops.gemm(h16, Lr.fc1.w, Lr.fc1.b, act=act, out=mlp)
            if fp8 >= 3:
                update(m8, Lr.fc2, ln_stats=stats2, ln_c1=Lr.fc2.zeros, out_dtype=dt)
            elif fp8 == 2:
                ops.quantize_rows_fp8(mlp, mlp_n, Lr.fc2.wscale, y8=m8, stats=stats)
                update(m8, Lr.fc2, ln_stats=stats, ln_c1=Lr.fc2.zeros, out_dtype=dt)
            elif fused and li + 1 < len(t.layers):
                update(mlp, Lr.fc2, **emit)
                ops.ln_finalize(part, slots, B * S, t.eps, stats)
            else:
                update(mlp, Lr.fc2)
        src, sdt = x, (dt if s32 else rd)
        if t.get("final_ln"):
            ln(t.final_ln[0], t.final_ln[1], y16=h16)
            src, sdt = h16, dt
        return ops.resample_tokens(src, B, t.has_cls, gh, out_grid, D, sdt, self._bil(gh, out_grid), out_dtype=self.dtype)

    # ------------------------------------------------------------------------------------------------ a5
    def sims_tensor(self, dino_feat, T):
        """adjacent-frame cosine similarity of the DINO features -> fp32 device tensor [T-1]."""
        n = dino_feat.shape[0] // T * dino_feat.shape[1]
        return ops.frame_cossim(dino_feat, T, n)

    # The segmentation is host logic on T - 1 similarities.  Reading them with .tolist() on the compute stream would also wait
    # for whatever was enqueued behind them (the SigLIP tower: a quarter of the step) and leave the device idle while the host
    # plans and enqueues the connector.  mark() / after(): an event behind the similarity kernel and a side stream that waits
    # for just that event - the host gets the numbers while the tower behind them is still running.
    def mark(self):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        return ev

    def tower_stream(self):
        """the ONE side stream the SigLIP tower runs on under `two_streams` (kept for the engine's life: its per-tower workspace
        `_vit_ws_siglip` and the cached tables are allocated under it once and never migrate between pool streams)"""
        st = self._tower_stream
        if st is None:
            st = self._tower_stream = torch.cuda.Stream(device=self.dev)
        return st

    def after(self, ev):
        side = self._side_stream
        if side is None:
            side = self._side_stream = torch.cuda.Stream(device=self.dev)
        side.wait_event(ev)
        return torch.cuda.stream(side)

    def fetch(self, t, ev):
        """device tensor t (ready at event ev) -> python list, without waiting for later work on the compute stream"""
        with self.after(ev):
            t.record_stream(torch.cuda.current_stream(self.dev))
            return t.cpu().tolist()

    def slot_sims(self, slab, pairs, defer=False):
        """a5 on cached rows: slab [slots, P, Dp] DINOv2 rows, pairs [(slot_a, slot_b)] -> host list of their cos-sims (the
        values sims_tensor gives for the two frames adjacent; read like the similarities: mark() / fetch()).  defer: return a
        function that reads them, so the host can enqueue more work before it waits."""
        sims = ops.pair_cossim(slab, pairs, slab[0].numel())
        ev = self.mark()
        return (lambda: self.fetch(sims, ev)) if defer else self.fetch(sims, ev)

    def gap_sims_tensor(self, dino_feat, T0, G):
        """the similarity table of a compact feature set: dino_feat [T0 * P, Dp], the DINOv2 rows of ALL
        T0 frames -> fp32 device tensor [G, T0 - 1], row g - 1, entry i = cos(f_i, f_{i+g}) for i + g < T0, every other entry
        0.0.  tdc_pair_cossim on the rows viewed as [T0, P, Dp] slots, at most 65535 pairs a call through one scratch: each
        value is bit for bit what sims_tensor gives for the two frames laid adjacent (what the lossless path computes behind
        its a1 gather), and row 0 is sims_tensor(dino_feat, T0).  Once per video, on export."""
        if not 1 <= G <= T0 - 1:
            raise ValueError("gap_sims_tensor: %d gaps of %d frames (1 .. frames - 1)" % (G, T0))
        if dino_feat.shape[0] % T0:
            raise ValueError("gap_sims_tensor: %d rows are not %d frames" % (dino_feat.shape[0], T0))
        slab = dino_feat.contiguous().view(T0, dino_feat.shape[0] // T0, dino_feat.shape[1])
        n = slab[0].numel()
        pairs = [(i, i + g) for g in range(1, G + 1) for i in range(T0 - g)]
        at = [(g - 1) * (T0 - 1) + i for g in range(1, G + 1) for i in range(T0 - g)]
        out = torch.zeros(G * (T0 - 1), device=self.dev, dtype=torch.float32)
        per = ops.PAIR_COSSIM_MAX
        scratch = ops.pair_cossim_scratch(min(per, len(pairs)), self.dev)
        for lo in range(0, len(pairs), per):
            vals = ops.pair_cossim(slab, pairs[lo:lo + per], n, scratch=scratch)
            out[torch.tensor(at[lo:lo + per], device=self.dev)] = vals
        return out.view(G, T0 - 1)

    def fingerprint(self, px, rows, row_bytes=None, row_stride=None):
        """frame cache keys: the 128-bit content fingerprints of the frames px[rows] (read in place; row_bytes / row_stride:
        other rows of px's bytes, ops.fingerprint_rows) -> host list of (u64, u64)"""
        fp = ops.fingerprint_rows(px.contiguous(), rows, row_bytes, row_stride)
        return [(a & 0xFFFFFFFFFFFFFFFF, b & 0xFFFFFFFFFFFFFFFF) for a, b in self.fetch(fp, self.mark())]

    def new_cache(self, max_bytes, kv_bytes=0):
        """a FrameCache of max_bytes for encode_video(cache=...) of this engine (cache.py); kv_bytes > 0: it also keeps the
        Q-Former's cross-attention K/V per (video, a1 selection) within that budget of their own"""
        from .cache import FrameCache, engine_signature
        return FrameCache(max_bytes, engine_signature(self), kv_bytes)

    # ---- stored tower features (features.py) --------------------------------------------------------
    def tower_width(self, name):
        """un-padded width of tower `name`'s rows: the input width of its aux projector (known without tower weights too)"""
        return self.c.aux[0 if name == "siglip" else 1].fc1.k

    def feature_rows(self, x):
        """stored rows [T, P, D] -> the [T * P, pad64(D)] rows `tower` returns: the padding columns are the zeros its last
        kernel writes (tdc_resample_tokens), so a5 and the connector launch on the pixel path's operands"""
        T, P, D = x.shape
        if x.dtype != self.dtype:
            raise ValueError("features are %s, this engine's towers emit %s" % (x.dtype, self.dtype))
        x = x.to(self.dev)
        if D == pad64(D):
            return x.reshape(T * P, D).contiguous()
        rows = torch.zeros(T * P, pad64(D), device=self.dev, dtype=self.dtype)
        rows[:, :D] = x.reshape(T * P, D)
        return rows

    def quantize_feature_rows(self, rows, D):
        """tower rows [n, >= D] (16-bit) -> (e4m3 bytes uint8 [n, D], fp32 scales [n]) of the compact feature store (DESIGN.md
        section 14): tdc_quantize_rows_fp8 with wscale = 1 and ldy8 = D - scale = max|row| / 448 (1 for a zero row), bytes =
        e4m3(row / scale)"""
        if rows.dtype != self.dtype:
            raise ValueError("features are %s, this engine's towers emit %s" % (rows.dtype, self.dtype))
        if D % 8 or D > 4608:
            raise ValueError("the compact feature store takes tower widths that are multiples of 8, at most 4608; got %d" % D)
        if rows.stride(0) % 8 or rows.data_ptr() % 16:          # stored [n, D] rows of a view: the kernel reads 16-byte pieces
            rows = rows.contiguous()
        y8 = torch.empty(rows.shape[0], D, device=self.dev, dtype=torch.uint8)
        _, stats = ops.quantize_rows_fp8(rows, D, 1.0, y8=y8)
        return y8, stats[:, 1].contiguous()

    def decode_feature_rows(self, x8, scale, idx, dtype):
        """compact rows x8 [T0, P, D] (e4m3 bytes) with scale [T0, P], the frames idx (None: all) -> the [T * P, pad64(D)] rows
        `tower` returns for them, up to the e4m3 rounding: ONE tdc_gather_rows launch gathers the kept frames, decodes them and
        lays them out; the padding columns are the zeros of the allocation"""
        T0, P, D = x8.shape
        if dtype != self.dtype:
            raise ValueError("the compact features decode to %s, this engine's towers emit %s" % (dtype, self.dtype))
        x8, scale = x8.to(self.dev).contiguous(), scale.to(self.dev).contiguous()
        if idx is None:
            frames = torch.arange(T0, device=self.dev, dtype=torch.int32)
        else:                                   # the kernel trusts its indices: range-checked here, on the host
            assert len(idx) and min(idx) >= 0 and max(idx) < T0, "frame out of range"
            frames = torch.tensor(list(idx), device=self.dev, dtype=torch.int32)
        assert T0 * P < 2 ** 31
        rows = (frames[:, None] * P + torch.arange(P, device=self.dev, dtype=torch.int32)[None]).reshape(-1)
        src = torch.stack([torch.zeros_like(rows), rows], 1).contiguous()
        n = rows.shape[0]
        Dp = pad64(D)
        out = (torch.empty if Dp == D else torch.zeros)(n, Dp, device=self.dev, dtype=self.dtype)
        return ops.gather_rows([x8.view(T0 * P, D)], src, n, D, out=out, validated=True, scales=[scale.view(T0 * P)],
                               dtype=self.dtype)

    def feature_signature(self):
        """features.tower_signature of this engine, computed once (it fingerprints every tower weight on the device)"""
        if self._feature_sig is None:
            from .features import compute_tower_signature
            self._feature_sig = compute_tower_signature(self)
        return self._feature_sig

    def frame_sims(self, dino_feat, T):
        """same as a python list (one D2H copy: the segmentation is host logic)."""
        return self.sims_tensor(dino_feat, T).tolist()

    def precise_dino(self, px):
        """px [n, 3, H, W] -> DINOv2 features [n * P, pad64(D)] from the fp16-operand copy of the tower (selection refinement)"""
        return self.tower("dino_precise", px)

    def pair_sims(self, feats, pairs):
        """feats: {frame: [P, Dp] feature rows}; pairs: [(a, b)] -> device fp32 tensor of cos-sim(feats[a], feats[b]) (the a5
        kernel on consecutive (a, b) blocks, every second value)"""
        rows = torch.cat([feats[f] for ab in pairs for f in ab], 0)
        return self.sims_tensor(rows, 2 * len(pairs))[0::2].contiguous()

    # ------------------------------------------------------------------------------------------------ a6-a10
    def aux_project(self, feat, i):
        a = self.c.aux[i]
        h = ops.gemm(feat, a.fc1.w, a.fc1.b, act=L.ACT_GELU_ERF)
        y = ops.gemm(h, a.fc2.w, a.fc2.b, out_f32=True)
        y16, _ = ops.layernorm(y, a.ln_g, a.ln_b, 1e-5, self.c.C, self.dtype)
        return y16

    def sva(self, aux, T, image_sizes, ctx=None):
        """aux: two [T*P, pad64(C)] 16-bit tensors -> queries [T*nq, pad64(C)] (vision_sampler_0, 3 layers).  ctx: the token
        mean of aux[0] when the caller has launched it already (connector with aux=)."""
        c, dt, dev = self.c, self.dtype, self.dev
        C, Cp = c.C, pad64(c.C)
        side = self.side
        nq = side * side
        P = aux[0].shape[0] // T
        n = int(round(P ** 0.5))
        r = n // side
        mask, _ = self._window_mask(T, P, image_sizes)      # host geometry, cached per (T, image size)
        if ctx is None:
            ctx = ops.token_mean(aux[0], T, P)                                # [T, Cp]
        q16 = torch.zeros(T * nq, Cp, device=dev, dtype=dt)
        q16[:, :C] = c.vision_query.to(dt).to(dev)[None, :]
        for Lr in c.sva:
            cproj = ops.gemm(ctx, Lr.proj_context.w)                          # [T, Cp]
            cin = ops.gemm(cproj, Lr.proj_in_c.w, out_f32=True)               # [T, Cp] fp32: per-frame bias
            qin = ops.gemm(q16, Lr.proj_in_q.w, res=cin, r_map=(nq, 1, 0, 0), out_f32=True)   # proj_in(cat[q, ctx])
            kvs = []
            for tw in range(2):
                xn, _ = ops.layernorm(aux[tw], c.ones_C, c.zeros_C, 1e-5, C, dt, add=Lr.pos[tw], add_period=P,
                                      add_mode=1)
                kvs.append(ops.gemm(xn, Lr.kv[tw].w, Lr.kv[tw].b))            # [T*P, 2C]: K | V
            qn, _ = ops.layernorm(qin, Lr.q_ln[0], Lr.q_ln[1], 1e-5, C, dt)
            qs = ops.gemm(qn, Lr.q_proj.w)
            att = ops.sva_attention(qs, kvs, mask, T, side, r, C, 16)
            q2 = ops.gemm(att, Lr.o_proj.w, res=qin, out_f32=True)            # queries + attention_output
            qn2, _ = ops.layernorm(q2, Lr.norm[0], Lr.norm[1], 1e-5, C, dt)
            h = ops.gemm(qn2, Lr.out1.w, act=L.ACT_GELU_ERF)
            q16 = ops.gemm(h, Lr.out2.w, res=q16)                             # + residual (layer input)
        return q16

    def mm_project(self, q16):
        h = ops.gemm(q16, self.c.mm1.w, self.c.mm1.b, act=L.ACT_GELU_ERF)
        return ops.gemm(h, self.c.mm2.w, self.c.mm2.b)

    def unpad_newline(self, feat, T, image_sizes):
        """feat [T*nq, Hp] -> X [T*N, Hp] with the newline column appended (all frames of a video share image_size).
        The gather map depends only on (T, image sizes): built once on the host, kept on the device."""
        side = self.side
        key = ("unpad", T, tuple(image_sizes[0]) if len(set(map(tuple, image_sizes))) == 1 else tuple(map(tuple, image_sizes)))
        hit = self._tables.get(key)
        if hit is None:
            import numpy as np
            cache, blocks, sizes = {}, [], []
            for t in range(T):
                k = tuple(image_sizes[t])
                if k not in cache:
                    m, sz = seg.unpad_newline_map(side, k, 0)
                    cache[k] = (np.asarray(m, dtype=np.int32).reshape(-1, 2), sz)
                m, sz = cache[k]
                blk = m.copy()
                blk[:, 1] += np.where(m[:, 0] == 0, t * side * side, 0).astype(np.int32)
                blocks.append(blk)
                sizes.append(sz)
            idx_np = np.concatenate(blocks, 0)
            ops.check_pairs_host(idx_np, [T * side * side, 1])
            idx = torch.from_numpy(idx_np).to(self.dev).contiguous()
            hit = self._tables[key] = (idx, sizes)
        idx, sizes = hit
        Hp = feat.shape[1]
        assert feat.shape[0] >= T * side * side
        X = ops.gather_rows([feat, self.c.image_newline], idx, idx.shape[0], Hp, validated=True)
        return X, list(sizes)

    # ---- native composite (csrc/api.cpp: tdc_connector_fwd): a6-a9 in one C call ------------------------------------------
    def _connector_struct(self):
        """ctypes mirror of tdc_connector_model (cached; keeps the arrays alive)."""
        if self._conn_struct is not None:
            return self._conn_struct
        c = self.c
        layers = (L.SvaLayer * len(c.sva))()
        for i, Lr in enumerate(c.sva):
            x = L.SvaLayer()
            x.proj_context, x.proj_in_c, x.proj_in_q = _lin(Lr.proj_context), _lin(Lr.proj_in_c), _lin(Lr.proj_in_q)
            x.pos[0], x.pos[1], x.ldpos = Lr.pos[0].data_ptr(), Lr.pos[1].data_ptr(), Lr.pos[0].stride(0)
            x.kv[0], x.kv[1] = _lin(Lr.kv[0]), _lin(Lr.kv[1])
            x.q_ln_g, x.q_ln_b = Lr.q_ln[0].data_ptr(), Lr.q_ln[1].data_ptr()
            x.q_proj, x.o_proj = _lin(Lr.q_proj), _lin(Lr.o_proj)
            x.norm_g, x.norm_b = Lr.norm[0].data_ptr(), Lr.norm[1].data_ptr()
            x.out1, x.out2 = _lin(Lr.out1), _lin(Lr.out2)
            layers[i] = x
        vq = torch.zeros(pad64(c.C), device=self.dev, dtype=self.dtype)
        vq[: c.C] = c.vision_query.to(self.dtype).to(self.dev)
        m = L.ConnectorModel()
        m.dtype, m.C, m.side, m.heads, m.n_layers = ops._dtcode(self.dtype), c.C, self.side, 16, len(c.sva)
        for i in range(2):
            a = c.aux[i]
            m.aux[i] = L.AuxProj(_lin(a.fc1), _lin(a.fc2), a.ln_g.data_ptr(), a.ln_b.data_ptr())
        m.vision_query, m.ones_C, m.zeros_C = vq.data_ptr(), c.ones_C.data_ptr(), c.zeros_C.data_ptr()
        m.layers_host = layers
        m.mm1, m.mm2 = _lin(c.mm1), _lin(c.mm2)
        self._conn_struct = (m, layers, vq)
        return self._conn_struct

    def _window_mask(self, T, P, image_sizes):
        side = self.side
        r = int(round(P ** 0.5)) // side
        key = ("mask", T, P, tuple(image_sizes[0]) if len(set(map(tuple, image_sizes))) == 1 else tuple(map(tuple, image_sizes)))
        hit = self._tables.get(key)
        if hit is None:
            import numpy as np
            cache, rows = {}, []
            for t in range(T):
                k = tuple(image_sizes[t])
                if k not in cache:
                    m0 = seg.window_mask_bytes(side, r, k)
                    # both towers share the geometry (same grid)
                    cache[k] = np.asarray([a + b for a, b in zip(m0, m0)], dtype=np.uint8)
                rows.append(cache[k])
            hit = self._tables[key] = torch.from_numpy(np.concatenate(rows, 0)).to(self.dev).contiguous()
        return hit, r

    def _connector_native(self, sig_feat, dino_feat, T, image_sizes, kept=None):
        """kept (aux0, aux1, ctx): buffers of _aux_keep_alloc that receive the aux rows and their per-frame mean instead of the
        workspace (tdc_connector_model.aux_keep / ctx_keep); `out` is the kept=None one bit for bit."""
        import ctypes as C
        m = self._connector_struct()[0]
        P = sig_feat.shape[0] // T
        mask, r = self._window_mask(T, P, image_sizes)
        m.r = r
        if kept is not None:
            # kept aux rows: a copy of the model struct carries the buffers, the cached one stays as is
            mk = L.ConnectorModel()
            C.pointer(mk)[0] = m
            Cp = pad64(self.c.C)
            for b, rows in zip(kept, (T * P, T * P, T)):
                assert b.is_cuda and b.device == sig_feat.device and b.dtype == self.dtype and b.is_contiguous() and \
                    tuple(b.shape) == (rows, Cp) and b.data_ptr() % 256 == 0, "kept is _aux_keep_alloc(T, P)"
            mk.aux_keep[0], mk.aux_keep[1], mk.ctx_keep = kept[0].data_ptr(), kept[1].data_ptr(), kept[2].data_ptr()
            m = mk
        assert dino_feat.shape[0] == T * P and P == (self.side * r) ** 2
        assert sig_feat.shape[1] >= m.aux[0].fc1.k and dino_feat.shape[1] >= m.aux[1].fc1.k
        lib = L.load()
        ws = self._workspace("_conn_ws", lib.tdc_connector_workspace_bytes(C.byref(m), T))
        out = torch.empty(T * self.side * self.side, pad64(self.c.H), device=self.dev, dtype=self.dtype)
        L.check(lib.tdc_connector_fwd(C.byref(m), ops._ptr(sig_feat), sig_feat.stride(0), ops._ptr(dino_feat),
                                      dino_feat.stride(0), T, ops._ptr(mask), ops._ptr(out), out.stride(0), ops._ptr(ws),
                                      ws.numel(), ops._stream()), "tdc_connector_fwd")
        return out

    def _aux_keep_alloc(self, T, P):
        """the three caller-owned buffers of tdc_connector_model.aux_keep / ctx_keep: aux rows [T*P, pad64(C)] of both towers
        and their per-frame mean [T, pad64(C)] (torch's allocator hands out 512-byte aligned blocks)"""
        Cp = pad64(self.c.C)
        return tuple(torch.empty(n, Cp, device=self.dev, dtype=self.dtype) for n in (T * P, T * P, T))

    def _aux_maps(self, T, P, image_sizes):
        """host geometry of the three aux outputs (segment.aux_window_map per frame), built once per (T, image sizes) and kept
        on the device: (feat_idx [n*r*r, 2], ctx_idx [n, 2], masks bool [n, r*r], n) - gather maps into the [T*P] aux rows and
        the [T] mean rows, range-checked on the host before upload."""
        side = self.side
        r = int(round(P ** 0.5)) // side
        key = ("aux", T, P, tuple(image_sizes[0]) if len(set(map(tuple, image_sizes))) == 1 else tuple(map(tuple, image_sizes)))
        hit = self._tables.get(key)
        if hit is None:
            import numpy as np
            assert T * P < 2 ** 31
            cache, feat, ctx, masks = {}, [], [], []
            for t in range(T):
                k = tuple(image_sizes[t])
                if k not in cache:
                    cache[k] = seg.aux_window_map(side, r, k)[:2]
                src, m = cache[k]
                feat.append(src.reshape(-1) + t * P)
                ctx.append(np.full(src.shape[0], t, dtype=np.int64))
                masks.append(m)

            def pairs(rows, limit):
                p = np.zeros((rows.shape[0], 2), dtype=np.int32)
                p[:, 1] = rows
                ops.check_pairs_host(p, [limit])
                return torch.from_numpy(p).to(self.dev).contiguous()
            ctx_rows = np.concatenate(ctx, 0)
            hit = self._tables[key] = (pairs(np.concatenate(feat, 0), T * P), pairs(ctx_rows, T),
                                       torch.from_numpy(np.concatenate(masks, 0)).to(self.dev).contiguous(),
                                       int(ctx_rows.shape[0]))
        return hit + (r,)

    def aux_outputs(self, aux0, aux1, ctx, T, image_sizes, aux):
        """slots 6, 7 and 9 of the reference's 10-tuple (tdc/cambrian_arch.py:1187-1193, 1295-1303) from the aux rows
        [T*P, pad64(C)] of both towers and their per-frame mean [T, pad64(C)]: three tdc_gather_rows launches into contiguous
        [n, r*r, C] / [n, 1, C] tensors of exactly C columns; the masks are host geometry.  Fills the dict `aux`."""
        C = self.c.C
        P = aux0.shape[0] // T
        feat_idx, ctx_idx, masks, n, r = self._aux_maps(T, P, image_sizes)
        if n == 0:
            raise ValueError("aux outputs: un-padding image sizes %r keeps no window" % (list(map(tuple, image_sizes)),))
        assert aux1.shape[0] == T * P and ctx.shape[0] == T
        feats = [ops.gather_rows([a], feat_idx, n * r * r, C, validated=True).view(n, r * r, C) for a in (aux0, aux1)]
        gctx = ops.gather_rows([ctx], ctx_idx, n, C, validated=True).view(n, 1, C)
        aux.update(features=feats, masks=[masks, masks.clone()], global_context=gctx)

    def connector(self, sig_feat, dino_feat, T, image_sizes, keep=None, aux=None):
        """a6-a10.  aux: a dict that receives the reference's three aux outputs (aux_outputs) - the native
        composite then leaves its aux rows in buffers of this call (aux_keep), the per-kernel route holds them anyway; X is
        the aux=None one bit for bit."""
        if keep is None and self.native_connector:
            kept = None if aux is None else self._aux_keep_alloc(T, sig_feat.shape[0] // T)
            feat = self._connector_native(sig_feat, dino_feat, T, image_sizes, kept)
            if aux is not None:
                self.aux_outputs(kept[0], kept[1], kept[2], T, image_sizes, aux)
            return self.unpad_newline(feat, T, image_sizes)
        rows = [self.aux_project(sig_feat, 0), self.aux_project(dino_feat, 1)]
        ctx = None
        if aux is not None:
            ctx = ops.token_mean(rows[0], T, rows[0].shape[0] // T)
            self.aux_outputs(rows[0], rows[1], ctx, T, image_sizes, aux)
        q = self.sva(rows, T, image_sizes, ctx)
        feat = self.mm_project(q)
        X, sizes = self.unpad_newline(feat, T, image_sizes)
        if keep is not None:
            keep.update(aux0=rows[0], aux1=rows[1], sva=q, mm_proj=feat)
        return X, sizes

    # ------------------------------------------------------------------------------------------------ a11-a19
    def qformer(self, enc, F, Nenc, query, qsrc, prompt_ids, multi=None, kv=None):
        """Batched Q-Former (tdc/Qformer.py:804-965) over F compressed frames.
        enc [F*Nenc, Hp] 16-bit; query [nC*K, Dq_pad] (query_proj output per chunk); qsrc int32 [F] chunk of frame.
        Returns last hidden state rows of the K query tokens as the combined buffer h16 [F*S, Dq_pad] and S.
        multi (the multi-prompt form): dict of HOST lists kv_src [F], frame_prompt [F] and the int
        enc_frames = U; prompt_ids is then a list of P id lists, F counts virtual frames, enc holds U frames and S = K + Lmax.
        kv (kept K/V; checked by compress_frames): the stacked K/V GEMM writes kv.buf, or, when kv.ready,
        is not launched - enc is then not read and may be None."""
        qf, dt = self.c.qformer, self.dtype
        Dq = qf.dim
        K = self.K
        heads = self.qheads
        hd = Dq // heads
        U, self_len, kv_src = F, None, None
        if multi is not None:
            if not self.multi_prompt_ok(Nenc):                    # refused before any launch
                raise ValueError("the multi-prompt Q-Former runs xattn_mode 0 / 1 only")
            U = int(multi["enc_frames"])
            assert enc is None or enc.shape[0] >= U * Nenc
            lens = [len(p or []) for p in prompt_ids]
            Lt = max(lens)
            ops.index_tensor(multi["kv_src"], 0, U, "cpu", "qformer kv_src")
            kv_src = [int(v) for v in multi["kv_src"]]
            h32, h16 = ops.qformer_embed(query, qsrc, qf.word, qf.pos, prompt_ids, qf.emb_ln[0], qf.emb_ln[1], 1e-12, F, K, Dq,
                                         dt, frame_prompt=multi["frame_prompt"])
            self_len = [K + lens[int(p)] for p in multi["frame_prompt"]] if Lt else None
        else:
            ids = self._prompt_tensor(prompt_ids)
            Lt = 0 if ids is None else ids.numel()
            h32, h16 = ops.qformer_embed(query, qsrc, qf.word, qf.pos, ids, qf.emb_ln[0], qf.emb_ln[1], 1e-12, F, K, Dq, dt)
        S = K + Lt
        # the cross-attention block: fused form = key GEMM + transposed value GEMM + one kernel per cross layer
        mode = int(self.xattn_mode) if qf.cross_k is not None else 0
        fused = mode >= 2 and ops.qformer_xattn_supported(Dq, heads, K, Nenc)
        if kv is not None and fused:                              # refused before any launch
            raise ValueError("kept K/V (kv=) runs xattn_mode 0 / 1 only")
        out_fused = not fused and mode >= 1 and ops.qformer_xattn_supported(Dq, heads, K, 8)
        if fused or out_fused:
            self._tile_cross_weights()
        ops.profile_tag(L.PROF_TAG_XATTN_BLOCK)
        if fused:
            k_all = ops.gemm(enc, qf.cross_k.w, qf.cross_k.b, M=F * Nenc)     # [F*Nenc, n_cross*Dq]
            vt_all = torch.empty(qf.cross_v.w.shape[0], pad64(F * Nenc + 4), device=self.dev, dtype=dt)   # ldvt >= round_up(F*Nenc, 8)
            ops.gemm(qf.cross_v.w, enc[:F * Nenc], out=vt_all, c_pad8=True)   # V^T = Wv enc^T: [n_cross*Dq, F*Nenc]
        elif kv is not None and kv.ready:
            kv_all = kv.buf                                                   # the rows an earlier pass projected
        else:
            kv_all = ops.gemm(enc, qf.cross_kv.w, qf.cross_kv.b, M=U * Nenc,  # [F*Nenc, n_cross*2*Dq] (multi: U frames)
                              out=None if kv is None else kv.buf)
        ops.profile_tag(0)
        Dp = h16.shape[1]
        ctx = torch.zeros(F * S, Dp, device=self.dev, dtype=dt)
        ctx_q = torch.zeros(F * K, Dp, device=self.dev, dtype=dt)
        t32 = torch.empty(F * S, Dp, device=self.dev, dtype=torch.float32)
        t16 = torch.empty(F * K, Dp, device=self.dev, dtype=dt) if out_fused else None
        scale = 1.0 / math.sqrt(hd)
        qmap = (K, S, 0, 1)
        tmap = (Lt, S, K, 1) if Lt else None
        for Lr in qf.layers:
            q16 = False          # this layer's query rows between the cross-attention output and the FFN LayerNorm: 16-bit only
            qkv = ops.gemm(h16, Lr.qkv.w, Lr.qkv.b)
            ld = qkv.stride(0)
            ops.attention(qkv[:, 0:Dq], qkv[:, Dq:2 * Dq], qkv[:, 2 * Dq:3 * Dq], ctx, F, heads, hd, S, S, scale,
                          S * ld, S * ld, S * ld, S * ctx.stride(0), k_len=self_len)
            ops.gemm(ctx, Lr.attn_out.w, Lr.attn_out.b, res=h32, out=t32, out_f32=True)
            ops.layernorm(t32, Lr.attn_ln[0], Lr.attn_ln[1], 1e-12, Dq, dt, y16=h16, y32=h32)
            ops.profile_tag(L.PROF_TAG_XATTN_BLOCK)
            if Lr.cross is not None and fused:
                j = Lr.cross.idx
                ops.qformer_xattn(h16, h32, F, K, S, Lr.cross.q_tiled, Lr.cross.q.b, Lr.cross.out_tiled, Lr.cross.out.b,
                                  k_all[:, j * Dq:(j + 1) * Dq], vt_all[j * Dq:(j + 1) * Dq], qf.cross_bv[j * Dq:(j + 1) * Dq],
                                  Nenc, Lr.cross.ln[0], Lr.cross.ln[1], 1e-12, Dq, heads, scale)
            elif Lr.cross is not None:
                cq = ops.gemm(h16, Lr.cross.q.w, Lr.cross.q.b, M=F * K, a_map=qmap)          # [F*K, Dq]
                j = Lr.cross.idx
                kk = kv_all[:, j * 2 * Dq: j * 2 * Dq + Dq]
                vv = kv_all[:, j * 2 * Dq + Dq: (j + 1) * 2 * Dq]
                ldk = kv_all.stride(0)
                ops.attention(cq[:, :Dq], kk, vv, ctx_q, F, heads, hd, K, Nenc, scale, K * cq.stride(0), Nenc * ldk,
                              Nenc * ldk, K * ctx_q.stride(0), kv_index=kv_src)
                if out_fused:
                    # the residual of this kernel and of the query FFN behind it is the 16-bit hidden state (the reference's
                    # half-precision arithmetic, tdc/Qformer.py:285-289,335-341): the fp32 copy of the query rows is neither
                    # read nor written until the FFN's LayerNorm rewrites both copies - half the bytes of the kernel
                    ops.qformer_xattn_out(h16, None, F, K, S, ctx_q, Lr.cross.out_tiled, Lr.cross.out.b, Lr.cross.ln[0],
                                          Lr.cross.ln[1], 1e-12, Dq, heads, res16=True)
                    q16 = True
                else:
                    ops.gemm(ctx_q, Lr.cross.out.w, Lr.cross.out.b, res=h32, r_map=qmap, out=t32, out_f32=True, M=F * K)
                    ops.layernorm(t32, Lr.cross.ln[0], Lr.cross.ln[1], 1e-12, Dq, dt, y16=h16, y32=h32, rows=F * K,
                                  y_map=qmap)
            ops.profile_tag(0)
            m = ops.gemm(h16, Lr.ffn_q.fc1.w, Lr.ffn_q.fc1.b, act=L.ACT_GELU_ERF, M=F * K, a_map=qmap)
            if q16:
                ops.gemm(m, Lr.ffn_q.fc2.w, Lr.ffn_q.fc2.b, res=h16, r_map=qmap, out=t16, M=F * K)
            else:
                ops.gemm(m, Lr.ffn_q.fc2.w, Lr.ffn_q.fc2.b, res=h32, r_map=qmap, out=t32, out_f32=True, M=F * K)
            if Lt:
                m2 = ops.gemm(h16, Lr.ffn_t.fc1.w, Lr.ffn_t.fc1.b, act=L.ACT_GELU_ERF, M=F * Lt, a_map=tmap)
                t32b = ops.gemm(m2, Lr.ffn_t.fc2.w, Lr.ffn_t.fc2.b, res=h32, r_map=tmap, out_f32=True, M=F * Lt)
            ops.layernorm(t16 if q16 else t32, Lr.ffn_q.ln[0], Lr.ffn_q.ln[1], 1e-12, Dq, dt, y16=h16, y32=h32, rows=F * K,
                          y_map=qmap)
            if Lt:
                ops.layernorm(t32b, Lr.ffn_t.ln[0], Lr.ffn_t.ln[1], 1e-12, Dq, dt, y16=h16, y32=h32, rows=F * Lt,
                              y_map=tmap)
        return h16, S

    def audio_tokens(self, beats_windows, sample_indices, T, lo=0, hi=None, window_sizes=None):
        """a20 (tdc/cambrian_arch.py:1552-1598): BEATs window features -> audio tokens of frames [lo, hi) of the T frames,
        [hi - lo, 50, 768] 16-bit (pooling of short / dropped seconds with tdc_adaptive_pool_tokens, zero padded tail).
        beats_windows: list of [1, n_w, 768] for ALL windows, or a dict {window: features} holding at least the windows the
        frames [lo, hi) draw from, together with window_sizes = token count of every window."""
        dt, dev = self.dtype, self.dev
        hi = T if hi is None else hi
        if isinstance(beats_windows, dict):
            assert window_sizes is not None
            src = beats_windows
        else:
            src = dict(enumerate(beats_windows))
            window_sizes = [int(w.reshape(-1, w.shape[-1]).shape[0]) for w in beats_windows]
        Da = next(iter(src.values())).shape[-1]
        plan = seg.audio_plan(list(window_sizes), [int(v) for v in sample_indices])
        wins = {}

        def win(w):
            if w not in wins:
                w2 = src[w].reshape(-1, Da).to(dev)
                assert w2.shape[0] == window_sizes[w]
                buf = torch.zeros(w2.shape[0], pad64(Da), device=dev, dtype=dt)
                buf[:, :Da] = w2.to(dt)
                wins[w] = buf
            return wins[w]
        out = torch.zeros(hi - lo, 50, Da, device=dev, dtype=dt)

        def pooled50(x):
            return x if x.shape[0] == 50 else ops.adaptive_pool_tokens(x.contiguous(), x.shape[0], 50, 1)
        for i in range(lo, min(hi, T, len(plan))):
            parts, direct = plan[i]
            toks = [pooled50(win(w)[s:e]) for (w, s, e) in parts]
            x = toks[0] if len(toks) == 1 else pooled50(torch.cat(toks, 0))
            out[i - lo] = x[:, :Da]
        return out

    def beats_windows(self, wav, mask=None, only=None):
        """tdc/cambrian_arch.py:1552-1560: BEATs features of the consecutive 10-s windows of wav [1, n] (16 kHz).
        `self.beats` is a beats.BeatsEncoder (set by the owner of the weights, e.g. model.initialize_audio).
        only = set of window indices -> dict {window: features} of just those windows."""
        if self.beats is None:
            raise RuntimeError("raw audio given but no BEATs encoder is attached (VideoEncoder.beats)")
        return self.beats.window_features(wav, only=only, mask=mask)

    def resample_pcm(self, pcm):
        """a decoded track (audio.PcmAudio) -> its mono 16 kHz waveform [1, n] fp32 on this device (tdc_pcm_resample; DESIGN.md
        section 22): what encode.normalize_audio puts in the place of audio={"audio_pcm": pcm}"""
        from . import audio as pcm_audio
        return pcm_audio.resample(pcm, device=self.dev)

    def local_audio(self, audio, sample_indices, T, lo=0, hi=None):
        """a20 for the frames [lo, hi) of the T kept frames: the caller's `audio` (None, a [T, 50, 768] token tensor, or
        the dict forms of prepare_inputs_labels_for_multimodal) -> [hi - lo, 50, 768] audio tokens (None without audio).
        With a raw waveform only the BEATs windows those frames draw from are encoded (frame sharding: dist.py)."""
        hi = T if hi is None else hi
        if audio is None:
            return None
        if not isinstance(audio, dict):
            return audio[lo:hi]
        if audio.get("audio_tokens") is not None:
            return audio["audio_tokens"][lo:hi]
        wins = audio.get("beats_windows")
        if wins is not None:
            return self.audio_tokens(wins, sample_indices, T, lo, hi)
        wav = audio["audio_wav"]                               # raw 16 kHz waveform: BEATs on the device (8(f)-1)
        if self.beats is None:
            raise RuntimeError("raw audio given but no BEATs encoder is attached (VideoEncoder.beats)")
        sizes = self.beats.window_token_counts(wav.shape[1])
        plan = seg.audio_plan(sizes, [int(v) for v in sample_indices])
        need = sorted({w for i in range(lo, min(hi, T, len(plan))) for (w, _, _) in plan[i][0]})
        if lo == 0 and hi >= T:
            need = None                                        # the whole video: every window, one batched call
        feats = self.beats_windows(wav, audio.get("audio_wav_mask"), only=need)
        if need is None:
            return self.audio_tokens(feats, sample_indices, T, lo, hi)
        return self.audio_tokens(feats, sample_indices, T, lo, hi, window_sizes=sizes)

    def with_audio(self, X, T, N, audio):
        """a20: frames become [visual N | audio_proj(audio) Na] rows (tdc/cambrian_arch.py:1611-1614)."""
        c, dt, dev = self.c, self.dtype, self.dev
        if audio is None:
            return X, N
        Hp = X.shape[1]
        Na = audio.shape[1]
        A16 = torch.zeros(T * Na, pad64(audio.shape[2]), device=dev, dtype=dt)
        A16[:, : audio.shape[2]] = audio.reshape(T * Na, -1).to(dt)
        Xf = torch.empty(T * (N + Na), Hp, device=dev, dtype=dt)
        Xf.view(T, N + Na, Hp)[:, :N].copy_(X.view(T, N, Hp))          # visual rows (device copy)
        ops.gemm(A16, c.audio_proj.w, c.audio_proj.b, out=Xf, c_map=(Na, N + Na, N, 1))   # audio rows
        return Xf, N + Na

    def make_queries(self, Xf, N, Nf, key_rows):
        """a12: adaptive-avg-pool the (visual part of the) key frames N -> K tokens and apply query_proj.
        key_rows: frame indices into Xf.  Returns [len(key_rows)*K, Dq_pad]."""
        keys = torch.tensor(key_rows, dtype=torch.int32, device=self.dev)
        pooled = ops.adaptive_pool_tokens(Xf, N, self.K, len(key_rows), keys, frame_rows=Nf)
        return ops.gemm(pooled, self.c.query_proj.w, self.c.query_proj.b)

    def learned_queries(self):
        """query_type == 'learned' (tdc/cambrian_arch.py:1639-1640): `query_tokens` [1, K, Dq] -> [K, Dq_pad] 16-bit."""
        qt = self.c.query_tokens
        if qt is None:
            raise RuntimeError("query_type='learned' needs `query_tokens` in the state dict")
        return qt

    def _tile_cross_weights(self):
        """fragment-major copies of the cross-attention query / output weights for tdc_qformer_xattn (made once, on the device)"""
        qf = self.c.qformer
        if qf.cross_k is None:
            return
        for Lr in qf.layers:
            if Lr.cross is not None and Lr.cross.q_tiled is None:
                Lr.cross.q_tiled = ops.xattn_tile_weight(Lr.cross.q.w)
                Lr.cross.out_tiled = ops.xattn_tile_weight(Lr.cross.out.w)

    def _qformer_struct(self):
        """ctypes mirror of tdc_qformer_model (cached)."""
        fused_on = int(self.xattn_mode)
        if self._qf_struct is not None and self._qf_struct[2] == fused_on:
            return self._qf_struct
        c, qf = self.c, self.c.qformer
        self._tile_cross_weights()
        zero = L.Lin(None, None, 0, 0)
        layers = (L.QformerLayer * len(qf.layers))()
        for i, Lr in enumerate(qf.layers):
            x = L.QformerLayer()
            x.qkv, x.attn_out = _lin(Lr.qkv), _lin(Lr.attn_out)
            x.attn_ln_g, x.attn_ln_b = Lr.attn_ln[0].data_ptr(), Lr.attn_ln[1].data_ptr()
            if Lr.cross is not None:
                x.has_cross, x.cross_idx = 1, Lr.cross.idx
                x.cross_q, x.cross_out = _lin(Lr.cross.q), _lin(Lr.cross.out)
                x.cross_ln_g, x.cross_ln_b = Lr.cross.ln[0].data_ptr(), Lr.cross.ln[1].data_ptr()
                if Lr.cross.q_tiled is not None:
                    x.cross_q_tiled, x.cross_out_tiled = Lr.cross.q_tiled.data_ptr(), Lr.cross.out_tiled.data_ptr()
            else:
                x.has_cross, x.cross_idx, x.cross_q, x.cross_out = 0, 0, zero, zero
            x.fq1, x.fq2 = _lin(Lr.ffn_q.fc1), _lin(Lr.ffn_q.fc2)
            x.fq_ln_g, x.fq_ln_b = Lr.ffn_q.ln[0].data_ptr(), Lr.ffn_q.ln[1].data_ptr()
            x.ft1, x.ft2 = _lin(Lr.ffn_t.fc1), _lin(Lr.ffn_t.fc2)
            x.ft_ln_g, x.ft_ln_b = Lr.ffn_t.ln[0].data_ptr(), Lr.ffn_t.ln[1].data_ptr()
            layers[i] = x
        m = L.QformerModel()
        m.dtype, m.dim, m.heads, m.n_layers, m.H, m.eps = ops._dtcode(self.dtype), qf.dim, self.qheads, len(qf.layers), \
            c.H, 1e-12
        m.word, m.pos, m.ldw = qf.word.data_ptr(), qf.pos.data_ptr(), qf.word.stride(0)
        m.emb_ln_g, m.emb_ln_b = qf.emb_ln[0].data_ptr(), qf.emb_ln[1].data_ptr()
        m.cross_kv, m.vision_proj = _lin(qf.cross_kv), _lin(c.vision_proj)
        if qf.cross_k is not None:
            m.cross_k, m.cross_v, m.cross_bv = _lin(qf.cross_k), _lin(qf.cross_v), qf.cross_bv.data_ptr()
            m.xattn_mode = fused_on
        m.layers_host = layers
        self._qf_struct = (m, layers, fused_on)
        return self._qf_struct

    def _prompt_tensor(self, prompt_ids):
        """BERT prompt ids as a device int32 tensor, validated on the host (an out-of-range id would fault in the kernel)."""
        if prompt_ids is None or len(prompt_ids) == 0:
            return None
        key = ("ids", tuple(int(i) for i in prompt_ids))
        hit = self._tables.get(key)
        if hit is None:
            qf = self.c.qformer
            assert max(key[1]) < qf.word.shape[0] and min(key[1]) >= 0 and len(key[1]) <= qf.pos.shape[0]
            hit = self._tables[key] = torch.tensor(key[1], dtype=torch.int32, device=self.dev)
        return hit

    def _compress_native(self, enc, F, Nf, qtable, qs, prompt_ids, multi=None, kv=None):
        import ctypes as C
        m = self._qformer_struct()[0]
        K = self.K
        assert qs.dtype == torch.int32 and qs.numel() >= F        # value range checked on the host list (compress_frames)
        U = F
        if kv is not None:
            # kept K/V (tdc_qformer_model.kv_keep): a copy of the model struct carries the buffer, the cached one stays as is
            mk = L.QformerModel()
            C.pointer(mk)[0] = m
            mk.kv_keep, mk.kv_state = kv.buf.data_ptr(), int(bool(kv.ready))
            m = mk
        if multi is not None:
            # the multi-prompt form (tdc_qformer_prompts): a copy of the model struct carries the block, the cached one stays as is
            qf = self.c.qformer
            U = int(multi["enc_frames"])
            ids, plen, Lt = ops.prompt_table(prompt_ids, qf.word.shape[0], qf.pos.shape[0], self.dev)
            lens = [len(p or []) for p in prompt_ids]
            assert len(multi["kv_src"]) == F and len(multi["frame_prompt"]) == F and U >= 1
            pr = L.QformerPrompts()
            pr.n_prompts, pr.enc_frames = len(prompt_ids), U
            kv_t = ops.index_tensor(multi["kv_src"], 0, U, self.dev, "kv_src")
            fp_t = ops.index_tensor(multi["frame_prompt"], 0, len(prompt_ids), self.dev, "frame_prompt")
            sl_t = ops.index_tensor([K + lens[int(p)] for p in multi["frame_prompt"]], K, K + Lt + 1, self.dev, "self_len")
            pr.kv_src, pr.frame_prompt, pr.prompt_len, pr.self_len = kv_t.data_ptr(), fp_t.data_ptr(), plen.data_ptr(), \
                sl_t.data_ptr()
            mm = L.QformerModel()
            C.pointer(mm)[0] = m
            mm.prompts = C.pointer(pr)
            m = mm
        else:
            ids = self._prompt_tensor(prompt_ids)
            Lt = 0 if ids is None else ids.numel()
        assert qtable.shape[1] >= pad64(m.dim)
        if enc is None:                                           # ready K/V: the composite does not read enc
            assert kv is not None and kv.ready
            enc_ptr, ldenc = C.c_void_p(0), 0
        else:
            assert enc.shape[0] >= U * Nf and enc.shape[1] >= m.cross_kv.k
            enc_ptr, ldenc = ops._ptr(enc), enc.stride(0)
        lib = L.load()
        ws = self._workspace("_qf_ws", lib.tdc_qformer_workspace_bytes(C.byref(m), F, K, Lt, Nf))
        out = torch.empty(F * K, pad64(self.c.H), device=self.dev, dtype=self.dtype)
        L.check(lib.tdc_qformer_fwd(C.byref(m), enc_ptr, ldenc, F, Nf, ops._ptr(qtable), qtable.stride(0),
                                    ops._ptr(qs), ops._ptr(ids if Lt else None), Lt, K, ops._ptr(out), out.stride(0),
                                    ops._ptr(ws), ws.numel(), ops._stream()), "tdc_qformer_fwd")
        return out

    def multi_prompt_ok(self, Nf):
        """whether compress_frames takes the multi-prompt form here: not under the whole-block cross-attention kernel
        (xattn_mode 2 where its shape support holds) - the callers then run one pass per prompt"""
        qf = self.c.qformer
        return not (int(self.xattn_mode) >= 2 and qf.cross_k is not None and
                    ops.qformer_xattn_supported(qf.dim, self.qheads, self.K, Nf))

    def kv_cache_ok(self, Nf):
        """whether compress_frames takes kept K/V (kv=) here: as multi_prompt_ok, not under the whole-block cross-attention
        kernel, which keeps K and transposed V in two buffers of other shapes - the callers then run the plain path"""
        return self.multi_prompt_ok(Nf)

    def kv_entry_bytes(self, U, Nf):
        """bytes of the kept K/V of U frames of Nf rows: U * Nf * n_cross * 2 * dim 16-bit values"""
        return U * Nf * self.c.qformer.cross_kv.w.shape[0] * 2

    def kv_alloc(self, U, Nf):
        """an unfilled kept-K/V buffer [U * Nf, n_cross * 2 * dim] for compress_frames(kv=KeptKV(buf, ready=False))"""
        return torch.empty(U * Nf, self.c.qformer.cross_kv.w.shape[0], device=self.dev, dtype=self.dtype)

    def compress_frames(self, Xf, Nf, frame_rows, qtable, qsrc, prompt_ids, keep=None, multi=None, kv=None):
        """a13-a18 for the frames `frame_rows` of Xf: Q-Former against queries qtable[qsrc[f]] -> [F*K, >=H] unit rows.
        multi = dict(kv_src, frame_prompt) (prompt_maps): frame_rows are the U DISTINCT frames, gathered and projected to K/V
        once; qsrc / kv_src / frame_prompt have one entry per virtual frame, prompt_ids is the list of the prompts' id lists;
        -> [F*K, >=H] in virtual-frame order, each row block bit for bit that of the prompt's own call.
        kv = cache.KeptKV(buf, ready): buf [U*Nf, n_cross*2*dim] (kv_alloc) holds the stacked cross-attention
        K/V of the U frames instead of the workspace.  Not ready: this pass projects into it, by the launch that fills the
        workspace otherwise.  Ready: neither the enc gather nor that GEMM is launched.  The result is the kv=None one bit for bit."""
        c, dev = self.c, self.dev
        K, H = self.K, c.H
        U = len(frame_rows)
        F = U if multi is None else len(qsrc)
        Hp = Xf.shape[1]
        assert F == len(qsrc) and (max(qsrc) + 1) * K <= qtable.shape[0] and min(qsrc) >= 0
        assert min(frame_rows) >= 0 and (max(frame_rows) + 1) * Nf <= Xf.shape[0]
        if kv is not None:
            if not self.kv_cache_ok(Nf):
                raise ValueError("compress_frames: kept K/V (kv=) runs xattn_mode 0 / 1 only (kv_cache_ok)")
            b, n = kv.buf, c.qformer.cross_kv.w.shape[0]
            assert b.is_cuda and b.device == Xf.device and b.dtype == self.dtype and b.dim() == 2 and b.is_contiguous() and \
                tuple(b.shape) == (U * Nf, n) and b.data_ptr() % 256 == 0, "kv.buf is kv_alloc(U, Nf)"
        enc = None
        if kv is None or not kv.ready:
            fr = torch.tensor(frame_rows, dtype=torch.int32, device=dev)
            enc_idx = torch.zeros(U * Nf, 2, dtype=torch.int32, device=dev)
            enc_idx[:, 1] = (fr[:, None] * Nf + torch.arange(Nf, dtype=torch.int32, device=dev)[None, :]).reshape(-1)
            enc = ops.gather_rows([Xf], enc_idx, U * Nf, Hp, validated=True)  # frame_rows range-checked above
        qs = torch.tensor(qsrc, dtype=torch.int32, device=dev)
        if multi is not None:
            if not self.multi_prompt_ok(Nf):
                raise ValueError("compress_frames: the multi-prompt form runs xattn_mode 0 / 1 only (multi_prompt_ok)")
            multi = dict(multi, enc_frames=U)
        if self.native_qformer:
            comp = self._compress_native(enc, F, Nf, qtable, qs, prompt_ids, multi, kv)
            if keep is not None:
                keep.update(compressed=comp)
            return comp
        h16, S = self.qformer(enc, F, Nf, qtable, qs, prompt_ids, multi, kv)
        comp = ops.gemm(h16, c.vision_proj.w, c.vision_proj.b, M=F * K, a_map=(K, S, 0, 1))
        ops.l2_normalize(comp, F * K, H)
        if keep is not None:
            keep.update(compressed=comp, last_hidden=h16, S=S)
        return comp

    def query_width(self):
        return pad64(self.c.qformer.dim)

    def emit_into(self, Xf, comp, pairs, out):
        """emit() into the first len(pairs) rows of a caller-owned [>= len(pairs), H] buffer (the sharded path's send buffer)."""
        return self.emit(Xf, comp, pairs, out=out)

    def compact_rows(self, src, idx, cols):
        """rows src[idx[:, 1]] -> a new [len(idx), cols] tensor (one tdc_gather_rows; idx validated by its builder)."""
        return ops.gather_rows([src], idx, idx.shape[0], cols, validated=True)

    def emit(self, Xf, comp, pairs, splice=None, out=None):
        """a19: one gather over (frame tokens | context tokens | frame_seg) -> [len(pairs), H].
        a21 hand-off (cambrian_arch.py:1712-1790 / cambrian_qwen.py:457-462): with
        splice = {"table": embed_tokens.weight [V, H] 16-bit on this device, "before": ids, "after": ids} the same
        launch also gathers the text embeddings, so the result is the LLM's inputs_embeds row block
        [len(before) + len(pairs) + len(after), H] with no intermediate visual tensor."""
        import numpy as np
        tables = [Xf, comp if comp is not None else self.c.frame_seg, self.c.frame_seg]
        p_np = pairs.cpu().numpy() if torch.is_tensor(pairs) else np.asarray(pairs, dtype=np.int32)
        p_np = np.ascontiguousarray(p_np.reshape(-1, 2).astype(np.int32, copy=False))
        if splice is not None:
            tab = splice["table"]
            assert tab.is_cuda and tab.device == Xf.device and tab.dtype == Xf.dtype and tab.shape[1] == self.c.H, \
                "prefill hand-off needs embed_tokens on the engine device in the engine dtype"

            def text(ids_):
                t = np.zeros((len(ids_), 2), dtype=np.int32)
                t[:, 0] = 3
                t[:, 1] = np.asarray([int(v) for v in ids_], dtype=np.int32)
                return t
            p_np = np.concatenate([text(splice["before"]), p_np, text(splice["after"])], 0)
            tables.append(tab)
        ops.check_pairs_host(p_np, [t.shape[0] if t.dim() == 2 else 1 for t in tables])
        idx = torch.from_numpy(p_np).to(self.dev)
        return ops.gather_rows(tables, idx, idx.shape[0], self.c.H, out=out, validated=True)

    def compress(self, X, T, N, seg_indices, prompt_ids, max_visual_len, audio=None, keep=None, splice=None):
        """X [T*N, Hp] -> emitted visual tokens [n, H] (tdc/cambrian_arch.py:1520-1709)."""
        return compress_with(self, X, T, N, seg_indices, prompt_ids, max_visual_len, audio, keep, splice)

    # ------------------------------------------------------------------------------------------------ top level
    def encode_video(self, px_siglip, px_dino, image_size, budget_text_len, n_text_tokens, prompt_ids, audio=None,
                     frame_cap=224, keep=None, splice=None, video_index=None, info=None, cache=None, aux=None, image=False):
        """One video: pixels -> emitted visual tokens [n, H] (S0-S10).  `budget_text_len` is the text length used by
        get_max_num_frames (cambrian_arch.py:753-759), `n_text_tokens` the non-image token count (:1499-1505).
        frame_cap: the reference's "in case of OOM" constant 224 of BOTH caps (cambrian_arch.py:907-916 before the towers,
        :813-822 inside adapt_segment) as a parameter.
        keep: dict that receives every stage tensor (and makes the connector run its per-kernel form, which produces them);
        info: dict that receives the host-side facts only (frame_indices, selected, seg_indices, final_size, n_visual) - free.
        cache: a FrameCache (new_cache): frames whose content it holds skip the towers and the connector, new ones are stored -
        the result is bit for bit that of cache=None (encode_video_cached).  keep= bypasses the cache (its per-kernel
        connector form is what produces the stage tensors).
        aux: a dict that receives the reference's three aux outputs for the kept frames: features (two
        [n, r*r, C] tensors), masks (two bool [n, r*r]) and global_context [n, 1, C], n = the frames' un-padded windows; the
        visual tokens are those of aux=None bit for bit.  With cache= it raises ValueError (the cache keeps connector rows, not
        aux rows).  image=True: the one frame as a single image - the towers and the connector only, rows [:, :H]."""
        return encode_video_with(self, px_siglip, px_dino, image_size, budget_text_len, n_text_tokens, prompt_ids,
                                 audio, frame_cap, keep, splice, video_index, info, cache, aux, image)

    def encode_video_prompts(self, px_siglip, px_dino, image_size, prompts, audio=None, frame_cap=224, video_index=None,
                             infos=None, cache=None, max_prompts=8, pad_fraction=0.25):
        """Several prompts about ONE video: prompts = dicts of budget_text_len, n_text_tokens, prompt_ids, optional splice
        -> one result per prompt, bit for bit what encode_video returns for it (encode_video_prompts_with)."""
        return encode_video_prompts_with(self, px_siglip, px_dino, image_size, prompts, audio, frame_cap, video_index, infos,
                                         cache, max_prompts, pad_fraction)

    def encode_batch(self, samples, frame_cap=224, infos=None):
        """Several videos / single images in one tower and connector pass: samples = dicts of encode_video's arguments
        (px_siglip, px_dino, image_size, budget_text_len, n_text_tokens, prompt_ids, audio, video_index, splice) plus
        `image`; -> one result per sample, bit for bit what encode_video (an image: the mixin's image branch) returns for it.
        infos: one info dict per sample (encode_batch_with).  All samples share the pixel geometry and type."""
        return encode_batch_with(self, samples, frame_cap, infos)

    def export_features(self, px_siglip, px_dino, image_size, store="f16", gaps=None):
        """The frozen towers once per video: ALL frames of px_siglip / px_dino ([T0, 3, H, W]; one frame is an image) through
        both towers -> features.FeatureSet (the rows `tower` returns without their padding columns, image_size, the towers'
        signature) for encode_features / encode_features_prompts, .save(path) and FeatureSet.load.  No a1 sub-sampling: it
        reads the prompt length and the frame cap.  The set serves any connector / Q-Former checkpoint, `context_token_num`,
        cap and prompt; it is refused (ValueError) by an engine whose towers differ in any output bit.
        The selection refinement needs pixels and cannot run from a set: an engine built with `tdc_dino_dtype = "float16"`
        (dino_dtype=torch.float16) stores DINOv2 rows of the reference's own precision, and no refinement is then wanted.
        store="e4m3": the compact set - one e4m3 byte per value and one fp32 scale per token row, half
        the bytes wherever the set lives or moves, decoded in the row gather of encode_features; it carries the exact a5
        similarities of the 16-bit rows, so a call that keeps every frame selects the lossless path's key frames bit for bit.
        The connector and Q-Former operands are lossy (measured contract: section 14).
        gaps (compact sets only; default None: no table, the set as it always was): "auto" or an int >= 1 - the set also carries
        the similarities of the 16-bit rows across that many frame gaps (section 16), so a call whose a1 SUB-SAMPLES selects
        the lossless path's key frames bit for bit as well, without an a5 launch.  "auto" covers every prompt length and frame
        cap: ceil(T0 / (max_num_segments + 2)) gaps, 4 * G * (T0 - 1) bytes."""
        return export_features_with(self, px_siglip.to(self.dev), px_dino.to(self.dev), image_size, store, gaps)

    def compact_features(self, fs, gaps=None):
        """a lossless FeatureSet -> the compact one, on the device: the bytes export_features(store="e4m3", gaps=gaps) gives.
        A set that is compact already comes back as it is; asked for more gaps than it holds, ValueError."""
        return compact_features_with(self, fs, gaps)

    def encode_features(self, fs, budget_text_len, n_text_tokens, prompt_ids, audio=None, frame_cap=224, splice=None,
                        video_index=None, info=None, check_signature=True, image=False, aux=None):
        """encode_video from a FeatureSet instead of pixels: bit for bit what encode_video returns for the pixels the set was
        exported from, whenever that call refines nothing (a band the refinement would re-encode is ranked as stored and
        reported in info["refine_unavailable_pairs"]).  check_signature=False: no comparison of the set's signature with this
        engine's towers (an engine that holds none).  image=True: a one-frame set as a single image - the connector only.
        aux: as encode_video's."""
        return encode_features_with(self, fs, budget_text_len, n_text_tokens, prompt_ids, audio, frame_cap, splice, video_index,
                                    info, check_signature, image, aux)

    def encode_features_prompts(self, fs, prompts, audio=None, frame_cap=224, video_index=None, infos=None, max_prompts=8,
                                pad_fraction=0.25, check_signature=True):
        """encode_video_prompts from a FeatureSet: the front from features once, then one compressor pass per group of
        prompts -> one result per prompt, bit for bit what encode_features returns for it."""
        return encode_features_prompts_with(self, fs, prompts, audio, frame_cap, video_index, infos, max_prompts, pad_fraction,
                                            check_signature)

    # ---- decoded uint8 frames in ------------------------------------------------------------------
    def pixels_from_frames(self, frames, idx=None, stats=None):
        """decoded frames uint8 [T0, H, W, 3] (torch tensor - pageable, pinned or on the device - or numpy array) and the
        ascending host list idx of the frames to keep (None: all) -> (px_siglip, px_dino) of the kept frames in the engine's
        `dtype`, bit for bit preprocess.process_images(frames[idx], dtype, frame_towers): the reference's process_images on the
        device.  Only the kept frames are uploaded and resized (preprocess.preprocess_selected).  frames may also be a
        preprocess.YuvFrames (NV12 / I420 planes): the kept frames' planes are uploaded and converted to
        RGB on the device in front of the same resize, and `frames[idx]` above reads as the RGB frames they convert to.  Either
        kind may be wrapped in a preprocess.Oriented (a display rotation / mirror): the kept frames are
        turned upright on the device and `frames[idx]` reads as the upright frames.  frames may also be a preprocess.RgbFrames
        (channel-first, B G R, 4-byte-pixel or gray pictures, pitched or cropped), bare or inside an
        Oriented: the kept frames are packed to R G B on the device and `frames[idx]` reads as the frames they stand for.
        Any of these kinds may be wrapped in a preprocess.Interlaced, bare or inside an Oriented: only
        the kept field of the kept frames is uploaded, the full-height frames are rebuilt from it on the device and
        `frames[idx]` reads as the rebuilt frames."""
        if len(self.frame_towers) != 2:
            raise ValueError("frame_towers is a pair of {R, mean, std} dicts (SigLIP, DINOv2), got %d" % len(self.frame_towers))
        px_siglip, px_dino = preprocess.preprocess_selected(frames, idx, self.frame_towers, self.dtype, self.frame_slab,
                                                            self.dev, stats=stats)
        return px_siglip, px_dino

    def encode_frames(self, frames, budget_text_len, n_text_tokens, prompt_ids, audio=None, frame_cap=224, splice=None,
                      video_index=None, info=None, cache=None, image_size=None, image=False, aux=None):
        """encode_video from the decoded frames of a video, uint8 [T0, H, W, 3] as a decoder hands them over (host or device),
        instead of pixels: a1 runs first, on the frame count, and only the frames it keeps are uploaded, resized and normalised
        (pixels_from_frames) - bit for bit what encode_video returns for preprocess.process_images of all frames.  The other
        arguments are encode_video's; image_size defaults to the frames' (H, W), what the reference's drivers pass.  info
        gains frames_in and frames_resized.  image=True: one frame as a single image - the towers and the connector only.
        aux: as encode_video's.  frames may be a preprocess.YuvFrames (4:2:0 planes as the decoder wrote them): the result is
        that of the RGB frames the planes convert to.  frames may be a preprocess.RgbFrames - [T0, 3, H, W]
        as torchcodec / torchvision.io return it, B G R as OpenCV does, RGBA / BGRA / ARGB surfaces, a gray plane, any of them
        pitched or cropped: the result is that of the [T0, H, W, 3] frames Pillow's .convert("RGB") makes of them (DESIGN.md
        section 24)."""
        return encode_frames_with(self, frames, budget_text_len, n_text_tokens, prompt_ids, audio, frame_cap, splice,
                                  video_index, info, cache, image_size, image, aux)

    def encode_frames_prompts(self, frames, prompts, audio=None, frame_cap=224, video_index=None, infos=None, cache=None,
                              max_prompts=8, pad_fraction=0.25, image_size=None):
        """encode_video_prompts from decoded frames (uint8 RGB or a preprocess.YuvFrames): one result per prompt, bit for bit
        what encode_frames returns for it"""
        return encode_frames_prompts_with(self, frames, prompts, audio, frame_cap, video_index, infos, cache, max_prompts,
                                          pad_fraction, image_size)

    def export_features_from_frames(self, frames, store="f16", image_size=None, slab=None, gaps=None):
        """export_features from decoded frames: every frame, preprocessed and run through the towers `slab` frames at a time
        (default encode.EXPORT_FRAMES_SLAB; the rows do not depend on it) - the set export_features gives for
        preprocess.process_images of the frames, bit for bit, without the pixels of all frames ever being resident.  frames may
        be a preprocess.YuvFrames."""
        return export_features_from_frames_with(self, frames, store, image_size, slab, gaps)
