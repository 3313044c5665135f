"""Orchestration of the video encode over an "engine": every policy decision of the path has one
function here, called by the serial path, the batched, cached and multi-prompt ones and the frame-sharded one (dist.py).

A video comes as pixels, decoded frames or stored tower features: a source each (PixelSource, FrameSource, FeatureSource) that
knows T0, image_size, front() - a2-a10 and a20 of the frames a1 kept - and image().  encode_source (one prompt) and
encode_source_prompts (several) evaluate a1 and run any source; the *_with names are their adapters per input kind.

The engine is pipeline.VideoEncoder on GPUs; the CPU tests plug in doubles.  The engine protocol:
  required   cfg, K, H, dtype; tower(name, px), sims_tensor(dino, T), connector(sig, dino, T, sizes, keep), local_audio,
             with_audio, make_queries, learned_queries, query_width, compress_frames, emit
  kept K/V   probed: kv_cache_ok(Nf), kv_entry_bytes(U, Nf), kv_alloc(U, Nf) and compress_frames(..., kv=) (DESIGN.md
             section 17) - an engine without kv_cache_ok reports "unsupported" and runs the plain path
  refinement selection_eps, selection_max_fraction, precise_dino(px), pair_sims(feats, pairs)
  frame cache fingerprint(px, rows), slot_sims(slab, pairs, defer), compact_rows(src, idx, cols), beats / beats_windows /
             audio_tokens (raw-waveform audio)
  PCM audio   probed: resample_pcm(pcm) -> the track's fp32 16 kHz waveform [1, n] on the engine's device (normalize_audio;
             audio.resample on an engine without the method)
  probed     mark / fetch / after (the host read beside the compute stream), two_streams / tower_stream (SigLIP on a side
             stream), emit_into, multi_prompt_ok, dev, side - absent on the doubles
  features   towers (what features.tower_signature fingerprints); probed: tower_width(name), feature_rows(x) (the tower
             rows' padding columns), feature_signature() (the signature, cached); compact sets (section 14):
             quantize_feature_rows(rows, D) -> (e4m3 bytes [n, D], fp32 scales [n]), decode_feature_rows(bytes [T0, P, D],
             scales [T0, P], idx or None, dtype) -> the rows [T * P, width] of the frames idx as `tower` returns them;
             probed: gap_sims_tensor(dino rows, T0, G) -> fp32 [G, T0 - 1], the similarities across gaps 1 .. G (section 16;
             gap_sims does it through sims_tensor on an engine without the method)
  frames     pixels_from_frames(frames uint8 [T0, H, W, 3], idx or None) -> (px_siglip, px_dino) of the frames idx, as the
             pixel entries take them
"""
import torch

from . import segment as seg


def normalize_audio(e, audio):
    """the ONE place decoded PCM becomes a waveform: a dict with "audio_pcm" (audio.PcmAudio) comes back
    as the same dict with "audio_wav" in its place - the whole track resampled to 16 kHz, fp32, on the engine's device
    (engine.resample_pcm where the engine has it, audio.resample otherwise) - and everything below sees a waveform.  Called
    where an audio dict first enters the orchestration (encode_source, encode_source_prompts, encode_batch_with,
    same_source_key, audio_key, the sharded encode); any other audio comes back as the object it is, so such a call issues
    the launches it always did.  "audio_pcm" beside "audio_wav", "beats_windows", "audio_tokens" or "audio_wav_mask" raises
    ValueError (a PcmAudio has no padding, so no mask goes with it)."""
    if not isinstance(audio, dict) or audio.get("audio_pcm") is None:
        return audio
    clash = [k for k in ("audio_wav", "beats_windows", "audio_tokens", "audio_wav_mask") if audio.get(k) is not None]
    if clash:
        raise ValueError("audio_pcm cannot be given together with %s" % ", ".join(clash))
    from .audio import is_pcm_audio, resample
    pcm = audio["audio_pcm"]
    if not is_pcm_audio(pcm):
        raise ValueError("audio_pcm must be an audio.PcmAudio, got %s" % type(pcm).__name__)
    rs = getattr(e, "resample_pcm", None)
    wav = rs(pcm) if rs is not None else resample(pcm, device=getattr(e, "dev", None))
    out = {k: v for k, v in audio.items() if k != "audio_pcm" and v is not None}
    out["audio_wav"] = wav
    return out


def visual_budget(cfg, n_text_tokens):
    """max_visual_len of a sample with n_text_tokens non-image tokens (tdc/cambrian_arch.py:1499-1505)"""
    return cfg["tokenizer_model_max_length"] - cfg.get("inference_max_length", 16) - n_text_tokens


def emission_plan(e, T, Nf, seg_indices, max_visual_len):
    """a11-a19 -> (segment.emit_plan, whether all chunks share the learned query block: cambrian_arch.py:1639-1640)"""
    cfg = getattr(e, "cfg", {})
    return (seg.emit_plan(T, Nf, e.K, seg_indices, max_visual_len, cfg.get("add_static", True)),
            cfg.get("query_type", "Avg_pool") == "learned")


def text_prompt(cfg, prompt_ids):
    """the Q-Former's text prompt: the sample's BERT ids, or none when `text_input` is off"""
    return prompt_ids if cfg.get("text_input", True) else None


def compress_with(e, X, T, N, seg_indices, prompt_ids, max_visual_len, audio=None, keep=None, splice=None, info=None,
                  kvs=None):
    Xf, Nf = e.with_audio(X, T, N, audio)
    plan, learned = emission_plan(e, T, Nf, seg_indices, max_visual_len)
    return compress_planned(e, Xf, N, Nf, plan, learned, prompt_ids, keep, splice, info, kvs)


# ---- kept cross-attention K/V: one entry per (video, a1 selection) in the frame cache ----------------
def kv_store(cache, keys, image_size, audio_key=None):
    """the K/V store of one front over the frames keyed `keys` (FrameCache.frame_keys, one per kept frame): what
    compress_planned / compress_many_with take as kvs=.  audio_key: same_video_key's audio material, None without audio."""
    return dict(cache=cache, keys=list(keys), image_size=tuple(image_size), audio=audio_key, used=set())


def kv_key(kvs, frames, Nf):
    """everything that changes a bit of the K/V of the compressed frames `frames`: their content keys in order, the rows per
    frame, image_size, and with audio (whose rows with_audio puts into Xf) its content and sampled seconds"""
    return (tuple(kvs["keys"][f] for f in frames), int(Nf), kvs["image_size"], kvs["audio"])


def kv_begin(e, kvs, frames, Nf, info=None):
    """look the entry of `frames` up -> (kv for compress_frames - None: the plain path -, commit() to call after the pass).
    hit: a ready buffer; miss: room is made, a buffer allocated, and commit() stores it once the pass has filled it; an entry
    above the budget, or an engine that cannot take kv= here, runs the plain path.  info["kv"] receives the record that
    info["cache"]["kv"] reports (cache_info_of)."""
    from .cache import KeptKV
    cache, U = kvs["cache"], len(frames)
    ok = getattr(e, "kv_cache_ok", None)
    rec = dict(state="unsupported", frames=U, bytes=0)
    kv, commit = None, (lambda: None)
    if ok is not None and ok(Nf):
        nbytes = rec["bytes"] = e.kv_entry_bytes(U, Nf)
        key = kv_key(kvs, frames, Nf)
        buf = cache.kv_get(key)
        if buf is not None:
            rec["state"], kv = "hit", KeptKV(buf, True)
            kvs["used"].add(key)
        elif not cache.kv_room(nbytes, kvs["used"]):
            rec["state"] = "bypassed"
        else:
            rec["state"], kv = "filled", KeptKV(e.kv_alloc(U, Nf), False)

            def commit():
                cache.kv_put(key, kv.buf, nbytes)
                kvs["used"].add(key)
    if info is not None:
        info["kv"] = rec
    return kv, commit


def cache_info_of(f, info):
    """info["cache"] of a call over the front f, read after the compressor ran; with a K/V budget it carries "kv": the
    record kv_begin left in info (a call without compressed frames: bypassed, no frames)"""
    ci = f["cache_info"]()
    rec = info.pop("kv", None)
    if f.get("kv") is not None:
        ci["kv"] = rec or dict(state="bypassed", frames=0, bytes=0)
    return ci


def compress_kept(e, kvs, info, Xf, Nf, frames, *rest):
    """e.compress_frames(Xf, Nf, frames, *rest) through the K/V store kvs (None: no store): kv= is passed only when kv_begin
    hands a buffer out - a hit or a fill, committed once the pass has run -, so an engine of today sees today's call"""
    kv, commit = kv_begin(e, kvs, frames, Nf, info) if kvs is not None else (None, None)
    if kv is None:
        return e.compress_frames(Xf, Nf, frames, *rest)
    comp = e.compress_frames(Xf, Nf, frames, *rest, kv=kv)
    commit()
    return comp


def compress_planned(e, Xf, N, Nf, plan, learned, prompt_ids, keep=None, splice=None, info=None, kvs=None):
    """compress_with after its planning: one prompt's Q-Former pass and emission over the rows Xf (with_audio) by `plan`.
    kvs (kv_store): the pass takes the cross-attention K/V of its compressed frames from the store, or fills its entry."""
    comp = None
    if plan["comp_frames"]:
        if learned:
            qtable, qsrc = e.learned_queries(), [0] * len(plan["comp_frames"])
        else:
            qtable, qsrc = e.make_queries(Xf, N, Nf, plan["key_frames"]), plan["comp_chunk"]
        comp = compress_kept(e, kvs if keep is None else None, info, Xf, Nf, plan["comp_frames"], qtable, qsrc, prompt_ids, keep)
    pairs = seg.emit_pairs(plan, Nf, e.K)
    if keep is not None:
        keep["plan"] = plan
        keep["n_visual"] = len(pairs)
    if info is not None:
        info["n_visual"] = len(pairs)
    if splice is not None:
        return e.emit(Xf, comp, pairs, splice)
    return e.emit(Xf, comp, pairs)


# ---- several prompts about one video in one compressor pass ------------------------------------------
MULTI_PROMPT_MAX_ROWS = 255     # K + Lmax of a group: below the 256 query rows from which tdc_attention's AUTO form changes kernels


def prompt_groups(selections, text_lens, frames, K, max_prompts, pad_fraction=0.25, max_rows=MULTI_PROMPT_MAX_ROWS):
    """`config.tdc_batch_prompts`: prompts p = 0 .. P-1 grouped greedily in call order.  A prompt joins the open group of its
    a1 selection (selections[p], any hashable) while the group holds fewer than max_prompts, its frame stride K + Lmax stays
    within max_rows, and its padding rows sum_p (Lmax - text_lens[p]) * frames[p] stay within pad_fraction of its
    sum_p (K + Lmax) * frames[p] rows; otherwise that group is closed and the prompt opens a new one.  -> lists of prompt
    indices ordered by their first member; a group of one runs the single-prompt path (compress_with)."""
    if max_prompts < 1:
        raise ValueError("max_prompts must be >= 1")
    groups, open_of = [], {}
    for p, key in enumerate(selections):
        g = open_of.get(key)
        if g is not None and len(g) < max_prompts:
            members = g + [p]
            Lmax = max(text_lens[i] for i in members)
            pad = sum((Lmax - text_lens[i]) * frames[i] for i in members)
            rows = sum((K + Lmax) * frames[i] for i in members)
            if K + Lmax <= max_rows and pad <= pad_fraction * rows:
                g.append(p)
                continue
        g = [p]
        groups.append(g)
        open_of[key] = g
    return groups


def prompt_maps(plans, learned=False):
    """The index maps of one group (the prompts' seg.emit_plan Plans over ONE video): the distinct compressed frames
    `enc_frames` and distinct key frames `key_frames` (both ascending), and per VIRTUAL frame - the compressed frames of prompt
    0, then prompt 1, ... - kv_src (position of its frame in enc_frames), qsrc (position of its chunk's key frame in
    key_frames; 0 with the shared learned query block), frame_prompt; offsets[p] = first virtual frame of prompt p."""
    enc_frames = sorted({f for pl in plans for f in pl["comp_frames"]})
    key_frames = sorted({pl["key_frames"][c] for pl in plans for c in pl["comp_chunk"]})
    upos = {f: i for i, f in enumerate(enc_frames)}
    kpos = {f: i for i, f in enumerate(key_frames)}
    kv_src, qsrc, frame_prompt, offsets = [], [], [], []
    for p, pl in enumerate(plans):
        offsets.append(len(kv_src))
        for f, c in zip(pl["comp_frames"], pl["comp_chunk"]):
            kv_src.append(upos[f])
            qsrc.append(0 if learned else kpos[pl["key_frames"][c]])
            frame_prompt.append(p)
    offsets.append(len(kv_src))
    return dict(enc_frames=enc_frames, key_frames=key_frames, kv_src=kv_src, qsrc=qsrc, frame_prompt=frame_prompt,
                offsets=offsets)


def compress_many_with(e, X, T, N, seg_indices, prompts, audio=None, infos=None, max_prompts=8, pad_fraction=0.25,
                       kvs=None):
    """a11-a19 for several prompts over ONE video's connector rows X (audio: the a20 tokens, as compress_with takes them):
    prompts = dicts of n_text_tokens, prompt_ids, optional splice -> one emitted tensor per prompt, bit for bit compress_with's.
    Per group (prompt_groups) the distinct compressed frames are gathered and projected to K/V once, the distinct key frames
    pooled once, and ONE Q-Former pass runs over the prompts' virtual frames (prompt_maps); a group of one, and every group on
    an engine whose compress_frames cannot take the form (multi_prompt_ok), runs compress_with.  kvs (kv_store): a group's
    pass takes the K/V of its distinct frames from the store or fills their entry; every member's info reports that record."""
    cfg = getattr(e, "cfg", {})
    K = e.K
    P = len(prompts)
    pids = [text_prompt(cfg, p["prompt_ids"]) for p in prompts]
    Xf, Nf = e.with_audio(X, T, N, audio)
    planned = [emission_plan(e, T, Nf, seg_indices, visual_budget(cfg, p["n_text_tokens"])) for p in prompts]
    plans, learned = [pl for pl, _ in planned], (planned[0][1] if planned else False)
    lens = [len(i) if i is not None else 0 for i in pids]
    groups = prompt_groups([0] * P, lens, [len(pl["comp_frames"]) for pl in plans], K, max_prompts, pad_fraction)
    ok = getattr(e, "multi_prompt_ok", lambda nf: True)(Nf)
    out = [None] * P
    for gi, g in enumerate(groups):
        gplans = [plans[p] for p in g]
        multi = ok and len(g) > 1 and all(pl["comp_frames"] for pl in gplans)
        Lmax = max(lens[p] for p in g)
        maps = prompt_maps(gplans, learned) if multi else None
        if multi:
            qtable = e.learned_queries() if learned else e.make_queries(Xf, N, Nf, maps["key_frames"])
            mm = dict(kv_src=maps["kv_src"], frame_prompt=maps["frame_prompt"])
            grec = {}
            comp = compress_kept(e, kvs, grec, Xf, Nf, maps["enc_frames"], qtable, maps["qsrc"], [pids[p] or [] for p in g], None,
                                 mm)
        for j, p in enumerate(g):
            info = infos[p] if infos is not None else None
            splice = prompts[p].get("splice")
            if not multi:                                         # today's path, on the plan made above
                out[p] = compress_planned(e, Xf, N, Nf, plans[p], learned, pids[p], None, splice, info, kvs)
                if info is not None:
                    info["prompts"] = dict(group=gi, group_size=1, pad_rows=0, shared_kv_frames=len(plans[p]["comp_frames"]))
                continue
            lo, hi = maps["offsets"][j], maps["offsets"][j + 1]
            pairs = seg.emit_pairs(plans[p], Nf, K)
            out[p] = e.emit(Xf, comp[lo * K:hi * K], pairs, splice) if splice is not None else \
                e.emit(Xf, comp[lo * K:hi * K], pairs)
            if info is not None:
                if "kv" in grec:
                    info["kv"] = dict(grec["kv"])
                info["n_visual"] = len(pairs)
                info["prompts"] = dict(group=gi, group_size=len(g), pad_rows=(Lmax - lens[p]) * len(plans[p]["comp_frames"]),
                                       shared_kv_frames=len(maps["enc_frames"]))
    return out


def encode_video_prompts_with(e, px_siglip, px_dino, image_size, prompts, audio=None, frame_cap=224, video_index=None,
                              infos=None, cache=None, max_prompts=8, pad_fraction=0.25):
    """Several prompts about ONE video -> one result per prompt, bit for bit what encode_video(...) returns for it.  The towers,
    a5 and the connector run once per distinct a1 selection (through `cache` when one is given); the prompts of a selection go
    through compress_many_with.  prompts: dicts of budget_text_len, n_text_tokens, prompt_ids, optional splice.  infos: one dict
    per prompt, filled as encode_video's info= plus info["prompts"] (the selection's front facts - info["cache"] among them -
    are those of the ONE front pass the selection's prompts share)."""
    return encode_source_prompts(e, PixelSource(px_siglip, px_dino, image_size, cache), prompts, audio, frame_cap, video_index,
                                 infos, max_prompts, pad_fraction)


def encode_source_prompts(e, src, prompts, audio=None, frame_cap=224, video_index=None, infos=None, max_prompts=8,
                          pad_fraction=0.25):
    """encode_video_prompts_with over any source (PixelSource, FrameSource, FeatureSource): a1 per prompt, here and nowhere
    below; the front of each distinct selection runs once (prompts_over_fronts)"""
    audio = normalize_audio(e, audio)
    sels = [frame_indices(e.cfg, src.T0, pr["budget_text_len"], frame_cap) for pr in prompts]       # a1
    return prompts_over_fronts(e, sels, prompts, lambda idx, finfo: src.front(e, idx, audio, video_index, finfo), infos,
                               max_prompts, pad_fraction)


def prompts_over_fronts(e, selections, prompts, front, infos=None, max_prompts=8, pad_fraction=0.25):
    """encode_source_prompts behind a1: the prompts of one video grouped by their a1 selection (selections[p]),
    front(idx, info) -> the front of the selection idx (run once per distinct selection), compress_many_with over each"""
    sels, order = {}, []
    for p, idx in enumerate(selections):
        key = tuple(idx)
        if key not in sels:
            sels[key] = []
            order.append(key)
        sels[key].append(p)
    out = [None] * len(prompts)
    base = 0
    for key in order:
        members = sels[key]
        finfo = {} if infos is not None else None
        f = front(selections[members[0]], finfo)
        sub = [infos[p] for p in members] if infos is not None else None
        res = compress_many_with(e, f["X"], f["T"], f["N"], f["seg_idx"], [prompts[p] for p in members], f["audio"], sub,
                                 max_prompts, pad_fraction, f.get("kv"))
        for p, r in zip(members, res):
            out[p] = r
            if infos is not None:
                info = infos[p]
                info.update(finfo)
                selection_facts(info, f)
                if "cache_info" in f:
                    info["cache"] = cache_info_of(f, info)
                info["prompts"]["group"] += base
        if infos is not None and members:
            base = max(infos[p]["prompts"]["group"] for p in members) + 1
    return out


def content_key(e, v):
    """hashable identity of an audio entry's content: tensors by shape, type and the 128-bit fingerprint of their bytes"""
    if torch.is_tensor(v):
        if v.numel() == 0:
            return ("tensor", str(v.dtype), tuple(v.shape))
        d = v.detach().to(e.dev).contiguous().view(-1)
        return ("tensor", str(v.dtype), tuple(v.shape), tuple(e.fingerprint(d, [0], d.numel() * d.element_size(), 0)[0]))
    if isinstance(v, dict):
        return ("dict",) + tuple((k, content_key(e, v[k])) for k in sorted(v))
    if isinstance(v, (list, tuple)):
        return ("list",) + tuple(content_key(e, x) for x in v)
    return ("value", repr(v))


def audio_key(e, audio, T0, idx, video_index=None):
    """what two calls must share of their audio: its content and the seconds it is sampled at (None without audio) - part of
    the same-video keys and of the name of a kept K/V entry"""
    if audio is None:
        return None
    return (content_key(e, normalize_audio(e, audio)), tuple(sample_indicator(T0, idx, video_index)))


def same_source_key(e, src, budget_text_len, frame_cap, audio=None, video_index=None):
    """`config.tdc_batch_prompts`: what two samples of one call must share to be questions about the SAME video: the content
    of what a1 keeps of their source (PixelSource.same_key, FeatureSource.same_key) and their audio (audio_key)"""
    idx = frame_indices(e.cfg, src.T0, budget_text_len, frame_cap)                                  # a1
    return src.same_key(e, idx, normalize_audio(e, audio), video_index)


def same_video_key(e, px_siglip, px_dino, image_size, budget_text_len, frame_cap, audio=None, video_index=None):
    """same_source_key of a video's pixels"""
    return same_source_key(e, PixelSource(px_siglip, px_dino, image_size), budget_text_len, frame_cap, audio, video_index)


def frame_indices(cfg, T0, budget_text_len, frame_cap):
    """a1 (tdc/cambrian_arch.py:899-916): the input frames kept, at most frame_cap (a5's second cap, :813-822, keeps all)"""
    return seg.uniform_indices(T0, min(seg.get_max_num_frames(budget_text_len, cfg), frame_cap))


def sample_indicator(T0, idx, video_index=None):
    """`sample_indices` of tdc/cambrian_arch.py:916-930: one 0/1 entry per second of the video's audio, 1 where a frame
    that survives the a1 cap was sampled.  video_index = the caller's `video_indices[i]` (0/1 per second, 1 = a frame was
    decoded there; None: input frame t is second t)."""
    if video_index is None:
        samp = [0] * T0
        for i in idx:
            samp[i] = 1
        return samp
    vi = [int(v) for v in (video_index.tolist() if hasattr(video_index, "tolist") else video_index)]
    if len(idx) == T0:
        return vi
    pos = [i for i, v in enumerate(vi) if v == 1]
    samp = [0] * len(vi)
    for i in idx:
        samp[pos[i]] = 1
    return samp


def start_side_tower(e, px_siglip):
    """`two_streams`, before the DINOv2 tower: SigLIP on the engine's side stream fills the partly filled last tile rounds of
    the other tower's GEMMs (T = 64: +0.6-1.1 %).  -> (stream, features) for join_side_tower, or None (off, host tensors)."""
    if not (getattr(e, "two_streams", False) and px_siglip.is_cuda):
        return None
    side = e.tower_stream() if hasattr(e, "tower_stream") else torch.cuda.Stream(device=px_siglip.device)
    side.wait_stream(torch.cuda.current_stream(px_siglip.device))
    with torch.cuda.stream(side):
        return side, e.tower("siglip", px_siglip)


def join_side_tower(e, started, px_siglip):
    """-> the SigLIP features for the compute stream: start_side_tower's, joined, or enqueued now if it started none"""
    if started is None:
        return e.tower("siglip", px_siglip)
    side, sig = started
    torch.cuda.current_stream(sig.device).wait_stream(side)
    sig.record_stream(torch.cuda.current_stream(sig.device))
    return sig


def select_segments_with(e, sims, refine, info=None):
    """a5 (tdc/cambrian_arch.py:832-849) on the T - 1 host similarities.  With engine.selection_eps, the pairs whose order that
    error leaves open (segment.selection_band) are re-ranked on refine(band) -> their fp16-tower similarities in band order,
    unless the band is a plateau (segment.band_allowed).  info receives refined_pairs and refine_skipped_pairs.  refine=None
    (stored tower features: no pixels to re-encode): the similarities are ranked as they are and info receives
    refine_unavailable_pairs = the size of the band that would have been refined."""
    mns = e.cfg.get("max_num_segments", 24)
    eps = getattr(e, "selection_eps", None)
    band = seg.selection_band(sims, mns, eps) if eps else []
    if band and not seg.band_allowed(band, len(sims) + 1, getattr(e, "selection_max_fraction", 0.125)):
        if info is not None:
            info["refine_skipped_pairs"] = len(band)
        band = []
    if band and refine is None:
        if info is not None:
            info["refine_unavailable_pairs"] = len(band)
        band = []
    if info is not None:
        info["refined_pairs"] = list(band)
    return seg.select_refined(sims, mns, eps, band, refine(band)) if band else seg.select_segments(sims, mns)


def precise_features(e, px_dino, frames, lo=0):
    """{frame: its feature rows from the fp16-operand DINOv2 tower} for the ascending `frames` (pixels: px_dino[frame - lo])"""
    fp = e.precise_dino(px_dino[torch.tensor([f - lo for f in frames], device=px_dino.device)])
    Pp = fp.shape[0] // len(frames)
    return {f: fp[j * Pp:(j + 1) * Pp] for j, f in enumerate(frames)}


def towers_and_selection(e, px_s, px_d, spans, infos=None):
    """a3-a5 of ONE tower pass over the kept frames px_s / px_d of one or several samples; spans: per sample (offset of its
    first frame, T, whether a5 segments it: T > max_num_segments + 1); infos: one dict (or None) per sample for
    select_segments_with.  -> (SigLIP features, DINOv2 features, seg_idx per sample).  a5 takes each sample's in-sample adjacent
    pairs out of one similarity launch over the whole pass (cross-sample pairs are dropped), read to the host once, and
    selects - and refines, on the sample's own pixels - per sample."""
    side_sig = start_side_tower(e, px_s)
    dino = e.tower("dino", px_d)                                                                    # a4
    sig = sims = None
    if any(segmented for _, _, segmented in spans):                                                 # a5
        sims_dev = e.sims_tensor(dino, px_d.shape[0])
        ev = e.mark() if hasattr(e, "mark") and sims_dev.is_cuda else None
        if side_sig is None:
            # the SigLIP tower does not depend on the selection: enqueue it BEFORE the one host read of the similarities, so
            # the device keeps working while the host ranks them (a3) - read on a side stream (fetch): no wait for the tower
            sig = e.tower("siglip", px_s)
        sims = e.fetch(sims_dev, ev) if ev is not None else sims_dev.tolist()
    seg_idx = []
    for j, (o, T, segmented) in enumerate(spans):
        if not segmented:
            seg_idx.append(list(range(T)))
            continue

        def refine(band, o=o):
            return e.pair_sims(precise_features(e, px_d, seg.band_frames(band), -o), [(i, i + 1) for i in band]).tolist()
        seg_idx.append(select_segments_with(e, sims[o:o + T - 1], refine, infos[j] if infos is not None else None))
    if sig is None:
        sig = join_side_tower(e, side_sig, px_s)                                                    # a3
    return sig, dino, seg_idx


def segmented(cfg, T):
    """whether a5 runs over T kept frames: only more than max_num_segments + 1 of them are segmented"""
    return T > cfg.get("max_num_segments", 24) + 1


def aux_kw(aux, cache=None):
    """the keyword that carries aux= (VideoEncoder.connector: the reference's three aux outputs) one level
    down - nothing when it was not asked for, so engines and sources that predate it are called as they always were.  With a
    frame cache it raises: the cache keeps connector rows, not aux rows."""
    if aux is None:
        return {}
    if not isinstance(aux, dict):
        raise ValueError("aux= is a dict that receives features / masks / global_context, got %r" % type(aux).__name__)
    if cache is not None:
        raise ValueError("aux= and cache= cannot be given together: the frame cache keeps connector rows, not aux rows")
    return {"aux": aux}


def pixel_front(e, cache, px_siglip, px_dino, rows, idx, T0, image_size, audio=None, keep=None, video_index=None, info=None,
                aux=None):
    """the prompt-independent part of an encode behind a1 (a2-a10, a20) from pixels: the kept frames are the rows `rows` of
    px_siglip / px_dino and the frames idx of the T0-frame video -> dict(X, T, N, seg_idx, audio, idx, final_size, sig, dino).
    Through the cache (front_cached_selected, which adds `cache_info` and leaves sig / dino out) unless there is none, keep=
    asks for the stage tensors only the uncached per-kernel connector form produces, or the call is over the cache's budget."""
    f = None
    aux = aux_kw(aux, cache)
    if cache is not None and keep is None:
        f = front_cached_selected(e, cache, px_siglip, px_dino, rows, idx, T0, image_size, audio, video_index, info)
    if f is not None:
        return f
    T = len(idx)
    if T != px_siglip.shape[0]:             # every frame kept: the pixels stay where they lie
        sel = torch.tensor(rows, device=px_siglip.device)
        px_siglip, px_dino = px_siglip[sel], px_dino[sel]
    sig, dino, (seg_idx,) = towers_and_selection(e, px_siglip, px_dino, [(0, T, segmented(e.cfg, T))],
                                                 None if info is None else [info])                  # a3-a5
    return front_after_towers(e, sig, dino, seg_idx, T0, idx, image_size, audio, keep, video_index, **aux)


def front_after_towers(e, sig, dino, seg_idx, T0, idx, image_size, audio=None, keep=None, video_index=None, aux=None):
    """what a front does once the tower rows of the a1-kept frames idx (of T0) and their a5 selection are known - the
    connector (a6-a10) and the frames' audio (a20) -> the front's dict.  Shared by pixel_front and FeatureSource.front."""
    T = len(idx)
    sizes = [tuple(image_size)] * T
    X, final_size = e.connector(sig, dino, T, sizes, keep, **aux_kw(aux))                           # a6-a10
    N = X.shape[0] // T
    if audio is not None:                                                                           # a20
        audio = e.local_audio(audio, sample_indicator(T0, idx, video_index), T, 0, T)
    return dict(X=X, T=T, N=N, seg_idx=seg_idx, audio=audio, idx=idx, final_size=final_size, sig=sig, dino=dino)


def image_rows(e, px_siglip, px_dino, image_size, cache=None, aux=None):
    """a single image ([1, 3, H, W] each): no a1 / a5 / Q-Former -> (connector rows [N, Hp], [final size]); through the frame
    cache when one is given"""
    aux = aux_kw(aux, cache)
    if cache is not None:
        return encode_image_cached(e, cache, px_siglip, px_dino, image_size)
    return e.connector(e.tower("siglip", px_siglip), e.tower("dino", px_dino), 1, [tuple(image_size)], **aux)


class PixelSource:
    """what an encode reads its frames from: here the pixels of ALL T0 frames of a video (px_siglip, px_dino [T0, 3, H, W]),
    through a FrameCache when one is given.  A source has T0 and image_size, front(e, idx, audio, video_index, info, keep) ->
    the front (a2-a10, a20) of the frames idx a1 kept, and image(e, info) -> the connector rows of its one frame as a single
    image (info receives what that entry reports).  FrameSource and FeatureSource are the other two."""

    def __init__(self, px_siglip, px_dino, image_size, cache=None):
        self.px_siglip, self.px_dino, self.image_size, self.cache = px_siglip, px_dino, image_size, cache
        self.T0 = px_siglip.shape[0]

    def front(self, e, idx, audio=None, video_index=None, info=None, keep=None, aux=None):
        return pixel_front(e, self.cache, self.px_siglip, self.px_dino, idx, idx, self.T0, self.image_size, audio, keep,
                           video_index, info, aux)

    def image(self, e, info=None, aux=None):
        X, sizes = image_rows(e, self.px_siglip, self.px_dino, self.image_size, self.cache, aux)
        if info is not None:
            info["final_size"] = sizes
        return X

    def same_key(self, e, idx, audio=None, video_index=None):
        """same_source_key behind a1: the frame cache's key material (FrameCache.frame_keys: the fingerprints of the a1-selected
        pixels, pixel geometry, image_size) and the audio.  Frames a1 drops are never read, so they do not count."""
        from .cache import FrameCache
        keys, _ = FrameCache.frame_keys(e, self.px_siglip.to(e.dev), self.px_dino.to(e.dev), idx, self.image_size)
        return (self.T0, tuple(idx), tuple(keys), audio_key(e, audio, self.T0, idx, video_index))


def encode_source(e, src, budget_text_len, n_text_tokens, prompt_ids, audio=None, frame_cap=224, keep=None, splice=None,
                  video_index=None, info=None, image=False, aux=None):
    """One video from any source (PixelSource, FrameSource, FeatureSource) -> emitted visual tokens [n, H]
    (VideoEncoder.encode_video documents the arguments).  a1 is evaluated here and nowhere below.  image=True: the source's one
    frame as a single image - its connector rows [:, :H], as prepare_inputs_labels_for_multimodal's image branch; a1 is not
    evaluated and budget_text_len may be None.  aux: a dict that receives the connector's three aux outputs (aux_kw); refused
    before any launch when the source carries a frame cache."""
    aux = aux_kw(aux, getattr(src, "cache", None))
    if image:
        return src.image(e, info, **aux)[:, :e.H]
    audio = normalize_audio(e, audio)
    idx = frame_indices(e.cfg, src.T0, budget_text_len, frame_cap)                                  # a1
    f = src.front(e, idx, audio, video_index, info, keep, **aux)
    return encode_front(e, f, n_text_tokens, prompt_ids, keep, splice, info)


def encode_video_with(e, px_siglip, px_dino, image_size, budget_text_len, n_text_tokens, prompt_ids, audio=None,
                      frame_cap=224, keep=None, splice=None, video_index=None, info=None, cache=None, aux=None, image=False):
    """One video: pixels -> emitted visual tokens [n, H].  cache: a FrameCache - the front runs through it, the result is bit
    for bit that of cache=None, and info["cache"] says what the call reused and encoded.  aux / image: encode_source's."""
    return encode_source(e, PixelSource(px_siglip, px_dino, image_size, cache), budget_text_len, n_text_tokens, prompt_ids,
                         audio, frame_cap, keep, splice, video_index, info, image, aux)


def selection_facts(info, f):
    """what info= (and keep=) report of the front f.  selected: what a5's second frame cap keeps - every frame (frame_indices)"""
    info.update(frame_indices=f["idx"], selected=list(range(f["T"])), seg_indices=f["seg_idx"], final_size=f["final_size"])


def encode_front(e, f, n_text_tokens, prompt_ids, keep=None, splice=None, info=None):
    """one prompt over the front f (a source's front): a11-a19 (+a21) -> emitted visual tokens [n, H]"""
    cfg = e.cfg
    vis = compress_with(e, f["X"], f["T"], f["N"], f["seg_idx"], text_prompt(cfg, prompt_ids),      # a11-a19 (+a21)
                        visual_budget(cfg, n_text_tokens), f["audio"], keep, splice, info, f.get("kv"))
    if keep is not None:
        selection_facts(keep, f)
        keep.update(siglip_feat=f["sig"], dino_feat=f["dino"], X=f["X"])
    if info is not None:
        selection_facts(info, f)
        if "cache_info" in f:               # read after the compressor ran
            info["cache"] = cache_info_of(f, info)
    return vis


def batch_groups(frames, ceiling, keys=None):
    """`config.tdc_batch_frames`: the samples of one call grouped greedily in batch order, the a1-selected frames of a group
    (frames[i]; images count 1) summing to at most `ceiling`; a sample above the ceiling forms its own group, and so does a
    change of keys[i] (the pixel geometry: frames of one group share one tower input).  -> lists of sample indices"""
    groups, cur, n = [], [], 0
    for i, f in enumerate(frames):
        if cur and (n + f > ceiling or (keys is not None and keys[i] != keys[cur[-1]])):
            groups.append(cur)
            cur, n = [], 0
        cur.append(i)
        n += f
    if cur:
        groups.append(cur)
    return groups


def gather_frames(pxs, plans, device):
    """the frames plans[j] of every pixel tensor pxs[j], in order, as one [sum, 3, H, W] tensor on `device`.  Each kept frame is
    copied once: from a host tensor that copy is the upload itself, on the device it is the a1 index copy (whole tensors when
    every frame is kept)."""
    px0 = pxs[0]
    out = torch.empty((sum(len(p) for p in plans),) + tuple(px0.shape[1:]), dtype=px0.dtype, device=device)
    o = 0
    for px, idx in zip(pxs, plans):
        if tuple(px.shape[1:]) != tuple(px0.shape[1:]) or px.dtype != px0.dtype:
            raise ValueError("a batch shares one tower input: pixels %s %s and %s %s differ"
                             % (tuple(px0.shape[1:]), px0.dtype, tuple(px.shape[1:]), px.dtype))
        dst = out[o:o + len(idx)]
        if len(idx) == px.shape[0]:
            dst.copy_(px)
        elif px.device == out.device:
            torch.index_select(px, 0, torch.tensor(idx, device=px.device), out=dst)
        else:
            dst.copy_(px[torch.tensor(idx)])
        o += len(idx)
    return out


def encode_batch_with(e, samples, frame_cap, infos=None):
    """Several samples in one tower and connector pass (`config.tdc_batch_frames`), each result bit for bit that of its own
    encode_video_with call (an image: its connector rows [:, :H], as prepare_inputs_labels_for_multimodal's image branch).
    samples: dicts of encode_video's arguments - px_siglip, px_dino, image_size, budget_text_len, n_text_tokens, prompt_ids,
    audio, video_index, splice - and `image` (True: one static frame, no a1 / a5 / Q-Former).  infos: one dict per sample
    (or None) that receives what encode_video's info= does (images: final_size).  -> list of per-sample results.
    a1 runs per sample; the kept frames of all samples go through one DINOv2 and one SigLIP pass; a5 takes the in-sample
    adjacent pairs of one similarity launch over the group (the cross-sample pairs are dropped) read to the host once, and
    selects (and refines, on the sample's own pixels) per sample; one connector call takes every frame's image_size and its
    rows are split by the returned sizes; a20, a11-a19 and the a21 hand-off run per sample.  This rests on tower batch
    invariance, the per-pair cos-sim reduction and the per-frame connector."""
    cfg = e.cfg
    mns = cfg.get("max_num_segments", 24)
    plans = [[0] if s.get("image") else frame_indices(cfg, s["px_siglip"].shape[0], s["budget_text_len"], frame_cap)
             for s in samples]                                                                      # a1
    offs = [0]
    for idx in plans:
        offs.append(offs[-1] + len(idx))
    Tg = offs[-1]
    dev = getattr(e, "dev", samples[0]["px_siglip"].device)
    px_s = gather_frames([s["px_siglip"] for s in samples], plans, dev)
    px_d = gather_frames([s["px_dino"] for s in samples], plans, dev)
    spans = [(o, len(idx), not s.get("image") and len(idx) > mns + 1) for s, idx, o in zip(samples, plans, offs)]
    sig, dino, seg_idx = towers_and_selection(e, px_s, px_d, spans, infos)                          # a3-a5
    sizes = [tuple(s["image_size"]) for s, idx in zip(samples, plans) for _ in idx]
    X, final_size = e.connector(sig, dino, Tg, sizes)                                               # a6-a10
    out, r = [], 0
    for j, (s, idx) in enumerate(zip(samples, plans)):
        T, o = len(idx), offs[j]
        fs = final_size[o:o + T]
        n = sum(h * (w + 1) for h, w in fs)          # unpad_newline: h rows of w tokens + a newline each
        Xs = X[r:r + n]
        r += n
        info = infos[j] if infos is not None else None
        if s.get("image"):
            out.append(Xs[:, :e.H])
            if info is not None:
                info["final_size"] = fs
            continue
        audio = normalize_audio(e, s.get("audio"))
        if audio is not None:                                                                       # a20
            audio = e.local_audio(audio, sample_indicator(s["px_siglip"].shape[0], idx, s.get("video_index")), T, 0, T)
        out.append(compress_with(e, Xs, T, n // T, seg_idx[j], text_prompt(cfg, s["prompt_ids"]),   # a11-a19 (+a21)
                                 visual_budget(cfg, s["n_text_tokens"]), audio, None, s.get("splice"), info))
        if info is not None:
            selection_facts(info, dict(idx=idx, T=T, seg_idx=seg_idx[j], final_size=fs))
    assert r == X.shape[0], "connector rows %d, split %d" % (X.shape[0], r)
    return out


def encode_missing(e, cache, keys, px_siglip, px_dino, idx, image_size, after_dino=None):
    """the frames idx[j] whose keys[j] the cache lacks (one per distinct key) through the towers and the connector, stored
    -> those keys, or None when this call's frames do not fit the budget (nothing stored).  after_dino(new keys, their DINOv2
    rows) is called between the two towers (encode_video_cached enqueues the a5 similarities there)."""
    new = cache.lookup(keys)
    if new:
        first = {}
        for j, k in enumerate(keys):
            first.setdefault(k, j)
        rows = [idx[first[k]] for k in new]
        if rows == list(range(px_siglip.shape[0])):          # every input frame, in order: no gather copy
            ps, pd = px_siglip, px_dino
        else:
            sel = torch.tensor(rows, device=px_siglip.device)
            ps, pd = px_siglip[sel], px_dino[sel]
        dino = e.tower("dino", pd)
        if after_dino is not None:
            after_dino(new, dino)
        sig = e.tower("siglip", ps)
        Xn, fsz = e.connector(sig, dino, len(new), [tuple(image_size)] * len(new))
        if not cache.store(new, Xn, dino, fsz, set(keys)):
            return None
    return new


def encode_image_cached(e, cache, px_siglip, px_dino, image_size):
    """a single image ([1, 3, H, W] each) through the frame cache: (connector rows [N, Hp], [final size]) - what
    e.connector(e.tower(...), e.tower(...), 1, [image_size]) returns, bit for bit"""
    cache.bind(e)
    keys, _ = cache.frame_keys(e, px_siglip, px_dino, [0], image_size)
    if encode_missing(e, cache, keys, px_siglip, px_dino, [0], image_size) is None:
        return image_rows(e, px_siglip, px_dino, image_size)
    return cache.assemble(e, keys), cache.final_sizes(keys)


def cached_audio(e, cache, audio, sample_indices, T, lo=0, hi=None):
    """a20 of encode_video_cached: local_audio(audio, sample_indices, T, lo, hi), with the BEATs windows of a raw waveform taken
    from the cache where it holds their waveform and mask slices (keys: fingerprints of the slices; window features are
    item-wise).  [lo, hi): the frames of one rank of the frame-sharded path (dist.py) - only their windows are used."""
    hi = T if hi is None else hi
    if not (isinstance(audio, dict) and audio.get("audio_tokens") is None and audio.get("beats_windows") is None
            and audio.get("audio_wav") is not None and getattr(e, "beats", None) is not None):
        return e.local_audio(audio, sample_indices, T, lo, hi)
    from .beats import SAMPLE_RATE
    wav, mask = audio["audio_wav"], audio.get("audio_wav_mask")
    n_s = wav.shape[1]
    starts = e.beats.window_starts(n_s)
    sizes = e.beats.window_token_counts(n_s)
    plan = seg.audio_plan(sizes, [int(v) for v in sample_indices])
    need = sorted({w for i in range(lo, min(hi, T, len(plan))) for (w, _, _) in plan[i][0]})
    if not need:
        return e.local_audio(audio, sample_indices, T, lo, hi)
    m = None if mask is None else torch.as_tensor(mask).bool().cpu()
    if m is not None and not bool(m.any()):
        m = None                                                  # what window_features does with an all-False mask
    n, eb = SAMPLE_RATE * 10, wav.element_size()
    wd = wav if wav.is_cuda else wav.to(e.dev)                    # fingerprinted on the device (a host waveform is copied)
    keys = {}
    for w in need:
        a, b = SAMPLE_RATE * starts[w], min(n_s, SAMPLE_RATE * (starts[w] + 10))
        mk = None if m is None else tuple(int(v) for v in fingerprint_mask(m[0, a:b]))
        keys[w] = ("beats", str(wav.dtype), b - a, mk)
    full = [w for w in need if keys[w][2] == n]
    fps = {}
    if full:
        fps.update(zip(full, e.fingerprint(wd, full, n * eb, n * eb)))
    for w in need:
        if w not in fps:
            fps[w] = e.fingerprint(wd, [1], keys[w][2] * eb, SAMPLE_RATE * starts[w] * eb)[0]
    keys = {w: keys[w] + (tuple(fps[w]),) for w in need}
    feats = cache.windows(keys, lambda todo: e.beats_windows(wav, mask, only=todo))
    return e.audio_tokens(feats, sample_indices, T, lo, hi, window_sizes=sizes)


def fingerprint_mask(m):
    """host fingerprint of a boolean mask slice (the mask lives on the host: window_features reads it there)"""
    from .cache import fingerprint_rows_host
    return fingerprint_rows_host(m.to(torch.uint8).numpy()[None])[0]


def front_cached_selected(e, cache, px_siglip, px_dino, rows, idx, T0, image_size, audio=None, video_index=None, info=None):
    """the prompt-independent part of a cached encode behind a1 (a2-a10, a20): the kept frames are the rows `rows` of
    px_siglip / px_dino and the frames idx of the T0-frame video.  PixelSource passes rows = idx (the pixels of all T0 frames);
    FrameSource has resized only the kept frames and passes rows = 0 .. T-1.  Audio and the returned idx refer to the video's
    own frame numbers; the cache keys are the fingerprints of the pixels either way.
    The kept frames are fingerprinted where they lie; only the frames the cache lacks run through the towers and the connector
    (frames are independent through a3-a10) and are stored; the a5 similarities come from the cache or from the cached DINOv2
    rows (tdc_pair_cossim), the refinement's precise values from the cache or from the pixels passed; the connector rows of the
    kept frames are gathered out of the slab.  -> pixel_front's dict plus `cache_info()` (the info["cache"] entry, read after
    the compressor ran), or None when the call's frames exceed the budget (info["cache"] says bypassed; nothing stored).  The
    tower batches see the HBM the cache holds as taken (auto_tower_batch): the rate may change, not the bits."""
    cache.bind(e)
    T = len(idx)
    keys, dkeys = cache.frame_keys(e, px_siglip, px_dino, rows, image_size)
    before = cache.stats()
    segs = segmented(e.cfg, T)
    early = {}
    # a3/a4, a6-a10 for the frames the cache lacks, a5 of the new frames' pairs enqueued BEFORE the SigLIP tower; a call whose
    # frames exceed the budget (known once the first frames fixed the row geometry) runs uncached
    new = encode_missing(e, cache, keys, px_siglip, px_dino, rows, image_size, lambda new, dino: early.update(
        cache.early_sims(e, keys, dkeys, new, dino, segs))) if cache.fits(keys) else None
    if new is None:
        if info is not None:
            info["cache"] = dict(bypassed=True, frames=T, frames_hit=0, frames_encoded=T, pairs_computed=0)
            if cache.kv_enabled:            # no frame keys to name an entry by: the compressor runs as without a store
                info["cache"]["kv"] = dict(state="bypassed", frames=0, bytes=0)
        return None
    if not segs:                                                                                    # a5
        seg_idx = list(range(T))
    else:
        sims = cache.adjacent_sims(e, keys, dkeys, early)

        def precise(pairs):
            frames = seg.band_frames(pairs)
            feats = precise_features(e, px_dino, [rows[f] for f in frames])
            return e.pair_sims(feats, [(rows[i], rows[i + 1]) for i in pairs]).tolist()
        seg_idx = select_segments_with(e, sims, lambda band: cache.precise_sims(band, dkeys, precise), info)
    X = cache.assemble(e, keys)
    N = cache.rows_per_frame
    final_size = cache.final_sizes(keys)
    kvs = None
    if cache.kv_enabled:                    # the kept K/V of this selection: named by the frames' keys and its audio
        kvs = kv_store(cache, keys, image_size, audio_key(e, audio, T0, idx, video_index))
    if audio is not None:                                                                           # a20
        audio = cached_audio(e, cache, audio, sample_indicator(T0, idx, video_index), T)
    f = dict(X=X, T=T, N=N, seg_idx=seg_idx, audio=audio, idx=idx, final_size=final_size,
             cache_info=lambda: cache.call_info(before, cache.stats(), keys, new))
    if kvs is not None:
        f["kv"] = kvs
    return f


def encode_video_cached(e, cache, px_siglip, px_dino, image_size, budget_text_len, n_text_tokens, prompt_ids, audio=None,
                        frame_cap=224, splice=None, video_index=None, info=None):
    """encode_video_with(..., cache=cache): one video through a FrameCache (cache.py), bit for bit the uncached result"""
    return encode_source(e, PixelSource(px_siglip, px_dino, image_size, cache), budget_text_len, n_text_tokens, prompt_ids,
                         audio, frame_cap, None, splice, video_index, info)


# ---- encode from stored tower features (features.FeatureSet) ------------------------------------------
def stored_rows(e, name, rows, T0):
    """tower rows [T0 * P, >= D] as FeatureSet stores them: [T0, P, D], the padding columns dropped (D: engine.tower_width)"""
    D = e.tower_width(name) if hasattr(e, "tower_width") else rows.shape[1]
    return rows[:, :D].reshape(T0, rows.shape[0] // T0, D)


def check_store(store, gaps=None):
    if store not in ("f16", "e4m3"):
        raise ValueError("export_features: store is \"f16\" (lossless) or \"e4m3\" (compact), got %r" % (store,))
    if gaps is not None and store != "e4m3":
        raise ValueError("export_features: gaps=%r asks for the similarity table of a compact set (store=\"e4m3\"); a "
                         "lossless set keeps its rows and needs none" % (gaps,))


def auto_gaps(cfg, T0):
    """the widest gap between two frames a5 can ever rank on a T0-frame video: a1 keeps uniform_indices(T0, m), whose
    neighbours lie floor(T0 / m) or ceil(T0 / m) apart, and a5 runs only for m > max_num_segments + 1"""
    return -(-T0 // (cfg.get("max_num_segments", 24) + 2))


def resolve_gaps(cfg, T0, gaps):
    """the `gaps` argument of the exports -> the number of table rows G (0: no table).  None: no table; "auto": auto_gaps;
    an int >= 1: that many.  Clipped to T0 - 1, so one frame has no table."""
    if gaps is None:
        return 0
    if isinstance(gaps, str) and gaps == "auto":
        G = auto_gaps(cfg, T0)
    elif isinstance(gaps, int) and not isinstance(gaps, bool) and gaps >= 1:
        G = gaps
    else:
        raise ValueError("gaps is None (no table), \"auto\" or an int >= 1, got %r" % (gaps,))
    return min(G, T0 - 1)


def gap_sims(e, dino, T0, G, sims=None):
    """fp32 [G, T0 - 1]: row g - 1, entry i = the a5 similarity of frames i and i + g of the DINOv2 tower rows `dino`
    ([T0 * P, width], all T0 frames) for i + g < T0, every other entry 0.0.  engine.gap_sims_tensor where
    the engine has it; otherwise per gap sims_tensor on the pairs' rows laid adjacent, every second value (as pair_sims), row 0
    being sims - sims_tensor(dino, T0) - when the caller holds it."""
    if hasattr(e, "gap_sims_tensor"):
        return e.gap_sims_tensor(dino, T0, G)
    fr = dino.reshape(T0, dino.shape[0] // T0, dino.shape[1])
    out = torch.zeros(G, T0 - 1, dtype=torch.float32, device=dino.device)
    for g in range(1, G + 1):
        if g == 1:
            row = sims if sims is not None else e.sims_tensor(dino, T0)
        else:
            n = T0 - g
            row = e.sims_tensor(torch.stack([fr[:n], fr[g:]], 1).reshape(-1, dino.shape[1]), 2 * n)
            row = torch.as_tensor(row, dtype=torch.float32)[0::2]
        out[g - 1, :T0 - g] = torch.as_tensor(row, dtype=torch.float32).to(out.device)
    return out


def export_features_with(e, px_siglip, px_dino, image_size, store="f16", gaps=None):
    """a3 / a4 of EVERY input frame (no a1: it reads the prompt length and the cap; both_towers) -> features.FeatureSet.
    store="e4m3": the compact set (compact_rows) - the bytes compact_features_with makes of the lossless set.  gaps (compact
    sets; resolve_gaps): the set also carries the similarities across that many frame gaps."""
    check_store(store, gaps)
    T0 = px_siglip.shape[0]
    if px_dino.shape[0] != T0 or T0 < 1:
        raise ValueError("export_features: %d SigLIP and %d DINOv2 frames" % (T0, px_dino.shape[0]))
    sig, dino = both_towers(e, px_siglip, px_dino)
    return feature_set_of(e, sig, dino, T0, image_size, store, gaps)


def both_towers(e, px_siglip, px_dino):
    """a3 / a4 with no selection between them -> (SigLIP rows, DINOv2 rows): SigLIP on the side stream under `two_streams`,
    after the DINOv2 tower otherwise"""
    side_sig = start_side_tower(e, px_siglip)
    dino = e.tower("dino", px_dino)                                                                 # a4
    return join_side_tower(e, side_sig, px_siglip), dino                                            # a3


def feature_set_of(e, sig, dino, T0, image_size, store="f16", gaps=None):
    """the tower rows of ALL T0 frames -> the FeatureSet an export returns: lossless, or compact (compact_rows)"""
    from .features import FeatureSet, tower_signature
    if store == "e4m3":
        return compact_rows(e, sig, dino, T0, image_size, tower_signature(e), gaps)
    return FeatureSet(stored_rows(e, "siglip", sig, T0), stored_rows(e, "dino", dino, T0), image_size, tower_signature(e))


def compact_rows(e, sig, dino, T0, image_size, signature, gaps=None):
    """the tower rows of ALL T0 frames ([T0 * P, >= D] each, as `tower` returns them) -> the compact FeatureSet (DESIGN.md
    section 14): per tower the e4m3 bytes and one fp32 scale per token row (engine.quantize_feature_rows: scale = max|row| / 448,
    1 for a zero row), and the a5 similarities of these 16-bit DINOv2 rows - taken before they are dropped, by the launch the
    lossless path takes them with, so a selection over all T0 frames is the lossless path's bit for bit.  gaps (resolve_gaps):
    the table of the same rows' similarities across gaps 1 .. G (gap_sims), which keeps that true under a1's sub-sampling."""
    from .features import FeatureSet
    G = resolve_gaps(getattr(e, "cfg", {}), T0, gaps)
    sims = e.sims_tensor(dino, T0) if T0 > 1 else None
    if sims is not None and not torch.is_tensor(sims):
        sims = torch.tensor(sims, dtype=torch.float32)
    if sims is not None:
        sims = sims.float().reshape(T0 - 1)
    table = gap_sims(e, dino, T0, G, sims) if G >= 1 else None
    parts = []
    for name, rows in (("siglip", sig), ("dino", dino)):
        D = e.tower_width(name) if hasattr(e, "tower_width") else rows.shape[1]
        b, sc = e.quantize_feature_rows(rows, D)
        parts += [b.reshape(T0, rows.shape[0] // T0, D), sc.reshape(T0, rows.shape[0] // T0)]
    return FeatureSet(parts[0], parts[2], image_size, signature, parts[1], parts[3],
                      sims, sig.dtype, table)


def compact_features_with(e, fs, gaps=None):
    """a lossless FeatureSet -> its compact form, the bytes export_features_with(store="e4m3", gaps=gaps) gives for the same
    pixels.  A compact set comes back as it is; it cannot gain gaps (ValueError): its 16-bit rows are gone."""
    from .features import is_compact
    if is_compact(fs):
        G = resolve_gaps(getattr(e, "cfg", {}), fs.frames, gaps)
        if G > fs.gaps:
            raise ValueError("compact_features: the set is compact already and holds the similarities of %d gap(s); %d are "
                             "asked for, and only the 16-bit rows of a lossless set can give them" % (fs.gaps, G))
        return fs
    sig, dino = feature_rows(e, fs)
    return compact_rows(e, sig, dino, fs.frames, fs.image_size, fs.signature, gaps)


def check_features(e, fs):
    """refuse a FeatureSet whose towers are not this engine's: ValueError naming both signatures"""
    from .features import tower_signature
    mine = tower_signature(e)
    if fs.signature != mine:
        raise ValueError("the feature set was exported by towers %r, this engine's towers are %r (check_signature=False "
                         "skips the comparison)" % (fs.signature, mine))


def feature_rows(e, fs, idx=None):
    """the stored rows of the frames idx (None: all) as the towers hand them on: ([T * P, width] SigLIP, DINOv2) on the
    engine's device.  The gather is plain indexing on the device, as the pixel path's px[sel]; engine.feature_rows restores
    the zero padding columns the towers write, so every launch behind it sees the pixel path's operands.
    A compact set: its bytes and scales go to the device and engine.decode_feature_rows does the a1 gather, the decode and the
    padded layout in one launch per tower - the 16-bit rows of a dropped frame never exist."""
    from .features import is_compact
    dev = getattr(e, "dev", fs.siglip.device)
    out = []
    for name, x in (("siglip", fs.siglip), ("dino", fs.dino)):
        if hasattr(e, "tower_width") and x.shape[2] != e.tower_width(name):
            raise ValueError("%s features are %d wide, the engine's tower is %d wide" % (name, x.shape[2], e.tower_width(name)))
        x = x.to(dev)
        if is_compact(fs):
            sc = (fs.siglip_scale if name == "siglip" else fs.dino_scale).to(dev)
            out.append(e.decode_feature_rows(x, sc, None if idx is None or len(idx) == x.shape[0] else idx, fs.rows_dtype))
            continue
        if idx is not None and len(idx) != x.shape[0]:              # every frame kept: the rows stay where they lie
            x = x[torch.tensor(idx, device=x.device)]
        out.append(e.feature_rows(x) if hasattr(e, "feature_rows") else x.reshape(-1, x.shape[2]))
    return out


class FeatureSource:
    """the stored tower rows of a video (features.FeatureSet) as an encode's source (PixelSource documents the members).
    check_signature: the set's signature is compared with the engine's towers (check_features) once, before the first rows are
    read"""

    def __init__(self, fs, check_signature=True):
        self.fs, self.unchecked = fs, check_signature
        self.T0, self.image_size = fs.frames, fs.image_size

    def check(self, e):
        if self.unchecked:
            check_features(e, self.fs)
            self.unchecked = False

    def front(self, e, idx, audio=None, video_index=None, info=None, keep=None, aux=None):
        """pixel_front from the stored rows instead of pixels: the kept frames' rows gathered, a5 by the pixel path's launch on
        the gathered DINOv2 rows, then front_after_towers -> the same dict, the same bits.  A compact set: a5 ranks the stored
        similarities of the ORIGINAL rows wherever the set holds every gap between neighbouring kept frames
        (features.stored_sims: every frame kept, or a gap table - section 16), else those of the decoded rows;
        info["selection_sims"] says which.  The selection refinement needs pixels: under engine.selection_eps a non-empty band is
        ranked on the stored similarities and reported as info["refine_unavailable_pairs"] (select_segments_with,
        refine=None)."""
        from .features import is_compact, stored_sims
        self.check(e)
        fs, T = self.fs, len(idx)
        sig, dino = feature_rows(e, fs, idx)
        compact = is_compact(fs)
        if segmented(e.cfg, T):                                                                     # a5
            # the similarities of the ORIGINAL 16-bit rows, stored with the set: every frame kept (gap 1), or sub-sampled within
            # the set's gap table - no launch, and the lossless path's selection bit for bit
            sims = stored = stored_sims(fs, idx) if compact else None
            if sims is None:
                sims_dev = e.sims_tensor(dino, T)
                ev = e.mark() if hasattr(e, "mark") and sims_dev.is_cuda else None
                sims = e.fetch(sims_dev, ev) if ev is not None else sims_dev.tolist()
            if compact and info is not None:
                info["selection_sims"] = "stored" if stored is not None else "decoded"
            seg_idx = select_segments_with(e, sims, None, info)
        else:
            seg_idx = list(range(T))
        return front_after_towers(e, sig, dino, seg_idx, self.T0, idx, fs.image_size, audio, keep, video_index, aux)

    def image(self, e, info=None, aux=None):
        if self.T0 != 1:
            raise ValueError("image=True takes a one-frame feature set, got %d frames" % self.T0)
        self.check(e)
        sig, dino = feature_rows(e, self.fs)
        X, sizes = e.connector(sig, dino, 1, [tuple(self.image_size)], **aux_kw(aux))
        if info is not None:
            info["final_size"] = sizes
        return X

    def same_key(self, e, idx, audio=None, video_index=None):
        """same_source_key behind a1: the content of both feature tensors (content_key), image_size, the a1 selection and the
        audio; a compact set: its scales too, and its gap table (a set with one selects on other similarities than a set
        without)"""
        from .features import is_compact
        fs = self.fs
        akey = audio_key(e, audio, self.T0, idx, video_index)
        key = (content_key(e, fs.siglip), content_key(e, fs.dino), tuple(fs.image_size), tuple(idx), akey)
        if is_compact(fs):                      # the same bytes under other scales are other rows
            key += (content_key(e, fs.siglip_scale), content_key(e, fs.dino_scale), str(fs.rows_dtype))
            if getattr(fs, "gap_sims", None) is not None:
                key += (content_key(e, fs.gap_sims),)
        return key


def encode_features_with(e, fs, budget_text_len, n_text_tokens, prompt_ids, audio=None, frame_cap=224, splice=None,
                         video_index=None, info=None, check_signature=True, image=False, aux=None):
    """encode_video_with from a FeatureSet: bit for bit its result for the pixels the set was exported from, whenever that
    call refines nothing.  image=True (a one-frame set): the connector rows [:, :H] of the image (info receives final_size)."""
    return encode_source(e, FeatureSource(fs, check_signature), budget_text_len, n_text_tokens, prompt_ids, audio, frame_cap,
                         None, splice, video_index, info, image, aux)


def encode_features_prompts_with(e, fs, prompts, audio=None, frame_cap=224, video_index=None, infos=None, max_prompts=8,
                                 pad_fraction=0.25, check_signature=True):
    """encode_video_prompts_with from a FeatureSet: the front from features once per distinct a1 selection, the selection's
    prompts through compress_many_with -> one result per prompt, bit for bit encode_features_with's"""
    return encode_source_prompts(e, FeatureSource(fs, check_signature), prompts, audio, frame_cap, video_index, infos,
                                 max_prompts, pad_fraction)


def same_features_key(e, fs, budget_text_len, frame_cap, audio=None, video_index=None):
    """same_source_key of a stored video"""
    return same_source_key(e, FeatureSource(fs), budget_text_len, frame_cap, audio, video_index)


# ---- encode from decoded uint8 frames: select, then resize what runs ----------------------------------
EXPORT_FRAMES_SLAB = 256        # frames per tower pass of export_features_from_frames_with (tower rows do not depend on it)


def frames_size(frames, image_size=None):
    """(T0, image_size) of decoded frames [T0, H, W, 3]; image_size defaults to (H, W), what the reference's drivers pass"""
    shape = tuple(frames.shape) if hasattr(frames, "shape") else (len(frames),) + tuple(frames[0].shape)
    if len(shape) != 4 or shape[0] < 1:
        raise ValueError("frames must be [T0, H, W, 3] with T0 >= 1, got %s" % (shape,))
    return int(shape[0]), (tuple(image_size) if image_size is not None else (int(shape[1]), int(shape[2])))


class FrameSource:
    """the decoded frames of a video (uint8 [T0, H, W, 3]) as an encode's source (PixelSource documents the members): a1 has
    run FIRST, on the frame count alone, and only the kept frames are resized and normalised (engine.pixels_from_frames).
    image_size defaults to the frames' (H, W); frames of another shape raise here, before any engine call.  A
    preprocess.YuvFrames (4:2:0 planes; .shape is that of the RGB frames they convert to) is a source like any other: the
    engine converts what it keeps.  So is a preprocess.Oriented over either kind (.shape is that of
    the upright frames, so image_size defaults to the upright (H', W')), and a preprocess.RgbFrames
    (channel-first, B G R, 4-byte-pixel or gray pictures; .shape is that of the RGB frames it stands for; DESIGN.md section
    24), and a preprocess.Interlaced over any of these kinds but an Oriented, which goes around it (one field kept and rebuilt
    to full height; .shape is that of the rebuilt frames)."""

    def __init__(self, frames, image_size=None, cache=None):
        self.frames, self.cache = frames, cache
        self.T0, self.image_size = frames_size(frames, image_size)

    def front(self, e, idx, audio=None, video_index=None, info=None, keep=None, aux=None):
        """the kept frames' pixels (rows 0 .. T-1), then pixel_front with T0 and idx handed over as PixelSource hands them - the
        same launches on the same operands, so the same dict and the same bits as the pixel front on process_images of ALL
        frames.  Audio and info["frame_indices"] refer to the video's own frame numbers.  The cache keys are the pixel
        fingerprints, so a video asked first through pixels hits here.  info gains frames_in = T0 and frames_resized =
        len(idx)."""
        T = len(idx)
        px_siglip, px_dino = e.pixels_from_frames(self.frames, idx)
        if info is not None:
            info.update(frames_in=self.T0, frames_resized=T)
        return pixel_front(e, self.cache, px_siglip, px_dino, list(range(T)), idx, self.T0, self.image_size, audio, keep,
                           video_index, info, aux)

    def image(self, e, info=None, aux=None):
        if self.T0 != 1:
            raise ValueError("image=True takes one frame, got %d" % self.T0)
        px_siglip, px_dino = e.pixels_from_frames(self.frames, None)
        X, sizes = image_rows(e, px_siglip, px_dino, self.image_size, self.cache, aux)
        if info is not None:
            info.update(final_size=sizes, frames_in=1, frames_resized=1)
        return X


def encode_frames_with(e, frames, budget_text_len, n_text_tokens, prompt_ids, audio=None, frame_cap=224, splice=None,
                       video_index=None, info=None, cache=None, image_size=None, image=False, aux=None):
    """encode_video_with from decoded frames: bit for bit its result on process_images of the same frames.  image=True (one
    frame): the connector rows [:, :H] of the image (through the cache when one is given; info receives final_size)."""
    return encode_source(e, FrameSource(frames, image_size, cache), budget_text_len, n_text_tokens, prompt_ids, audio,
                         frame_cap, None, splice, video_index, info, image, aux)


def encode_frames_prompts_with(e, frames, prompts, audio=None, frame_cap=224, video_index=None, infos=None, cache=None,
                               max_prompts=8, pad_fraction=0.25, image_size=None):
    """encode_video_prompts_with from decoded frames: the front from frames once per distinct a1 selection (each resizes its
    own kept frames), the selection's prompts through compress_many_with -> one result per prompt, bit for bit
    encode_frames_with's"""
    return encode_source_prompts(e, FrameSource(frames, image_size, cache), prompts, audio, frame_cap, video_index, infos,
                                 max_prompts, pad_fraction)


def export_features_from_frames_with(e, frames, store="f16", image_size=None, slab=None, gaps=None):
    """export_features_with from decoded frames: EVERY frame (no a1), preprocessed and run through both towers `slab` frames
    at a time (default EXPORT_FRAMES_SLAB), the rows concatenated.  Tower rows do not depend on the tower batch, so the set equals
    export_features_with(*process_images(frames)) bit for bit - without the pixels of all T0 frames ever existing."""
    check_store(store, gaps)
    T0, image_size = frames_size(frames, image_size)
    slab = EXPORT_FRAMES_SLAB if slab is None else int(slab)
    if slab < 1:
        raise ValueError("export_features: slab must be a positive frame count, got %r" % (slab,))
    sigs, dinos = [], []
    for s in range(0, T0, slab):
        sig, dino = both_towers(e, *e.pixels_from_frames(frames, list(range(s, min(s + slab, T0)))))
        sigs.append(sig)
        dinos.append(dino)
    sig = sigs[0] if len(sigs) == 1 else torch.cat(sigs, 0)
    dino = dinos[0] if len(dinos) == 1 else torch.cat(dinos, 0)
    return feature_set_of(e, sig, dino, T0, image_size, store, gaps)
