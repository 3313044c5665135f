"""Frame-sharded encoding of ONE long video over the GPUs of a node; one process per GPU,
torch.distributed (backend "nccl" = RCCL over xGMI on ROCm; "gloo" in the CPU tests).

Rank r owns the contiguous frames [lo, hi) of the frames that survive the a1 cap.  Cross-rank data flow per video:
  0. a1 (frame budget + uniform sub-sampling) is host integer logic on (T0, text length): every rank computes the same
     selection (`frame_plan`) and loads / is handed only its own frames.
  1. DINO on the local frames; every rank but the first sends the feature rows of its FIRST frame (576 x 1536 16-bit values,
     1.77 MB) to its left neighbour, which needs them for its last adjacent similarity (round 1 re-encoded that frame on
     both ranks: one frame in 65 sounds cheap, but it pushes the DINOv2 qkv / fc1 GEMMs of a 64-frame shard over a tile-round
     boundary of the persistent kernel - ~2 % of the step against ~0.1 ms of xGMI transfer); callers that still pass the
     halo frame's pixels get the old behaviour.  All-gather of the T-1 fp32 similarities -> every rank runs the identical
     stable selection -> identical plan.
  2. SigLIP + connector on the local frames (no communication).  Audio (a20): a rank runs BEATs on the 10-second windows
     its own seconds fall into (a window that straddles a rank boundary is encoded by both ranks, like the DINO halo)
     and builds the audio tokens of its own frames; no exchange.
  3. Chunks whose key frame lives on another rank: the owner sends its K x Dq query block (K=16: 24 KB) point to point
     (query_type 'learned': every rank holds the same `query_tokens`, nothing is sent).
  4. Q-Former on the local compressed frames; every rank emits the tokens of its own frames in plan order;
     all-gather (padded to the longest shard; shard lengths are known from the plan) -> identical full stream on every
     rank, tail clipping (a19) already applied through the shared plan.
The numerical work is delegated to an engine object (pipeline.VideoEncoder on GPUs; a test double in the gloo tests);
the transport to a comm object (TorchComm = torch.distributed; the tests also plug in an in-process thread transport to
rehearse world sizes a one-GPU box cannot host as processes).
"""
import numpy as np
import torch

from . import segment as seg
from .cache import fingerprint_rows_host
from .encode import (cached_audio, emission_plan, encode_missing, frame_indices, join_side_tower, normalize_audio,
                     precise_features, sample_indicator, select_segments_with, start_side_tower, text_prompt, visual_budget)


def owner_of(frame, ranges):
    for r, (lo, hi) in enumerate(ranges):
        if lo <= frame < hi:
            return r
    raise ValueError(frame)


def split_plan(plan, ranges, Nf, K):
    """Per rank: emission pairs (table, row) in plan order with LOCAL rows (int32 array [n_r, 2]); the separator follows
    its frame.  Also returns, per rank, the dict global compressed-frame index -> local index."""
    starts = np.asarray([lo for lo, _ in ranges], dtype=np.int64)
    comp_frames = np.asarray(plan["comp_frames"] if plan["comp_frames"] else [0], dtype=np.int64)
    n_comp = len(plan["comp_frames"])
    comp_owner = np.searchsorted(starts, comp_frames[:max(n_comp, 1)], side="right") - 1
    comp_local_idx = np.zeros(max(n_comp, 1), dtype=np.int64)
    comp_local = [dict() for _ in ranges]
    for r in range(len(ranges)):
        m = np.nonzero(comp_owner[:n_comp] == r)[0]
        comp_local_idx[m] = np.arange(len(m))
        comp_local[r] = {int(g): i for i, g in enumerate(m.tolist())}
    kind, a, b = plan.kind, plan.a, plan.b
    n = len(kind)
    a_c = np.where(kind == 1, a, 0)
    frame = np.where(kind == 0, a, np.where(kind == 1, comp_frames[a_c], -1))
    last = np.maximum.accumulate(np.where(kind != 2, np.arange(n), -1)) if n else np.zeros(0, dtype=np.int64)
    frame_ff = np.where(last >= 0, frame[np.maximum(last, 0)], starts[0]) if n else frame
    owner = np.searchsorted(starts, frame_ff, side="right") - 1
    row = np.where(kind == 0, (a - starts[owner]) * Nf + b, np.where(kind == 1, comp_local_idx[a_c] * K + b, 0))
    both = np.stack([kind, row], 1).astype(np.int32)
    per = [np.ascontiguousarray(both[owner == r]) for r in range(len(ranges))]
    return per, comp_local


class TorchComm:
    """torch.distributed transport (RCCL on the GPUs of a node; gloo in the CPU tests and in the one-GPU rehearsals).
    RCCL operations are ordered on the stream; gloo's point-to-point operations read a device tensor from the host through
    its raw pointer with no stream ordering at all, so with gloo the device is synchronised before anything is posted."""

    def __init__(self, rank, world, group=None):
        self.rank, self.world, self.group = rank, world, group
        self._host_side = None

    def _sync_if_host_side(self, t):
        if self._host_side_now() and t is not None and t.is_cuda:
            torch.cuda.synchronize(t.device)

    def _host_side_now(self):
        if self._host_side is None:
            import torch.distributed as dist
            self._host_side = dist.get_backend(self.group) != "nccl"
        return self._host_side

    def all_gather(self, t):
        import torch.distributed as dist
        self._sync_if_host_side(t)
        out = [torch.empty_like(t) for _ in range(self.world)]
        dist.all_gather(out, t, group=self.group)
        return out

    def all_gather_into(self, out, t):
        """out [world * n, ...] <- the ranks' t [n, ...] in rank order: ONE collective into a caller-owned buffer (RCCL: the
        direct all-gather over the xGMI links, no list of per-rank outputs, no concatenation afterwards)."""
        import torch.distributed as dist
        self._sync_if_host_side(t)
        dist.all_gather_into_tensor(out, t, group=self.group)
        self._sync_if_host_side(t)

    def exchange(self, sends, recvs):
        """sends: [(tensor, dst)], recvs: [(buffer, src)] - posted in this order on every rank, completed before return."""
        import torch.distributed as dist
        ops_ = [dist.P2POp(dist.isend, t, dst, self.group) for t, dst in sends] + \
               [dist.P2POp(dist.irecv, buf, src, self.group) for buf, src in recvs]
        if ops_:
            self._sync_if_host_side((sends + recvs)[0][0])
            for rq in dist.batch_isend_irecv(ops_):
                rq.wait()
            self._sync_if_host_side((sends + recvs)[0][0])


class ShardedVideoEncoder:
    def __init__(self, engine, rank, world, group=None, comm=None):
        self.e, self.rank, self.world = engine, rank, world
        self.comm = comm if comm is not None else TorchComm(rank, world, group)
        self._bufs = {}        # (tag, rows, cols, dtype) -> preallocated send / receive buffers of the token all-gather
        self._maps = {}        # shard lengths -> device index map of the compaction gather

    def new_cache(self, nbytes):
        """a FrameCache of nbytes for encode_video(cache=...) - this rank's own frames (engine.new_cache)"""
        return self.e.new_cache(nbytes)

    # ---- a1 on every rank --------------------------------------------------------------------------------------------
    def frame_plan(self, T0, budget_text_len, frame_cap=224, video_index=None, halo=False):
        """tdc/cambrian_arch.py:899-935 for a T0-frame video: which input frames survive the budget, which of them this rank
        encodes (`siglip_frames`; `dino_frames` = the same - plus the next rank's first frame with halo=True, the
        re-encode-instead-of-exchange variant), and the per-second 0/1 vector the audio interleave needs.  Pure host
        integers: identical on every rank."""
        idx = frame_indices(self.e.cfg, T0, budget_text_len, frame_cap)
        T = len(idx)
        lo, hi = seg.shard_ranges(T, self.world)[self.rank]
        want_halo = bool(halo)
        halo = 1 if (halo and lo < hi < T) else 0    # a rank without frames (T < world) has no halo either
        return dict(idx=idx, T=T, lo=lo, hi=hi, siglip_frames=idx[lo:hi], dino_frames=idx[lo:hi + halo], recompute_halo=want_halo,
                    sample_indices=sample_indicator(T0, idx, video_index))

    def _tokens_per_frame(self, image_size, audio):
        """rows per frame in the Q-Former KV / static emission (cur_h * (cur_w + 1), + 50 with audio) without running the
        connector - only a rank that owns no frame needs it (to lay out the shared plan)."""
        side = getattr(self.e, "side", None)
        if side is None:
            return self.e.N + (0 if audio is None else 2)          # CPU test double
        r0, r1, c0, c1 = seg.unpad_bounds(side, side, image_size)
        return (r1 - r0) * (c1 - c0 + 1) + (50 if audio is not None else 0)

    def _all_gather_var(self, t, counts):
        """all-gather of 1-D/2-D tensors with per-rank leading sizes `counts` (known to every rank): the small exchanges
        (similarities) and engines / transports without the buffered form."""
        mx = max(counts)
        pad = torch.zeros((mx,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        if t.shape[0]:
            pad[: t.shape[0]] = t
        out = self.comm.all_gather(pad)
        return torch.cat([o[:c] for o, c in zip(out, counts)], 0)

    def _buf(self, tag, rows, cols, dtype, device):
        key = (tag, rows, cols, dtype, str(device))
        b = self._bufs.get(key)
        if b is None:
            for k in [k for k in self._bufs if k[0] == tag]:      # one buffer per role: a new shape replaces the old one
                del self._bufs[k]
            b = self._bufs[key] = torch.zeros(rows, cols, dtype=dtype, device=device)
        return b

    def _gather_tokens(self, emit_local, counts, cols, dtype, device):
        """The final exchange: every rank's emitted rows -> the whole stream on every rank.
        `emit_local(out)` writes this rank's counts[rank] rows into out[:counts[rank]].  Buffered form (engine with
        `compact_rows`, transport with `all_gather_into`): the rank emits straight into its padded send buffer, ONE
        all_gather_into_tensor fills a preallocated [world * max, cols] buffer and one row gather (tdc_gather_rows with an
        index map cached per shard-length tuple) drops the padding - no per-step allocation besides the result, no list of
        per-rank tensors, no torch.cat.  At the bench's size (T = 512, K = 144, world 8) a rank contributes ~9.4 k rows =
        67 MB and receives 538 MB."""
        mx, n = max(counts), counts[self.rank]
        e = self.e
        if not (hasattr(e, "compact_rows") and hasattr(self.comm, "all_gather_into")):
            local = torch.zeros(0, cols, dtype=dtype, device=device)
            if n:
                local = torch.empty(n, cols, dtype=dtype, device=device)
                emit_local(local)
            return self._all_gather_var(local, counts)
        send = self._buf("send", mx, cols, dtype, device)
        recv = self._buf("recv", self.world * mx, cols, dtype, device)
        if n:
            emit_local(send)
        self.comm.all_gather_into(recv, send)
        key = tuple(counts)
        idx = self._maps.get(key)
        if idx is None:
            self._maps.clear()
            rows = np.concatenate([r * mx + np.arange(c, dtype=np.int64) for r, c in enumerate(counts)]) if sum(counts) else \
                np.zeros(0, dtype=np.int64)
            pairs = np.zeros((len(rows), 2), dtype=np.int32)
            pairs[:, 1] = rows
            idx = self._maps[key] = torch.from_numpy(pairs).to(device)
        return e.compact_rows(recv, idx, cols)

    def _refined_sims(self, band, px_dino_local_halo, ranges, recompute_halo):
        """the `refine` of encode.select_segments_with, sharded: the pairs of `band` - the same list on every rank - are
        re-encoded by the engine's precise DINOv2 tower.  Pair i belongs to the rank that owns frame i; it needs frame i + 1 as
        well, which for the last local frame is the right neighbour's first: that rank sends the precise feature rows of its
        first frame (as the boundary exchange of step 1 does for the fast tower), unless the caller handed this rank the halo
        frame's pixels (recompute_halo).  -> the refined values of the whole band in band order, on every rank."""
        e, rank, world = self.e, self.rank, self.world
        lo, hi = ranges[rank]
        inband = set(band)
        mine = [i for i in band if lo <= i < hi]
        frames = {f for i in mine for f in (i, i + 1) if f < hi}
        send_first = rank > 0 and (lo - 1) in inband and hi > lo and not recompute_halo      # left neighbour's last pair
        if send_first:
            frames.add(lo)
        cross = rank < world - 1 and hi > lo and (hi - 1) in inband                          # my last pair crosses the boundary
        if cross and recompute_halo:
            frames.add(hi)                                                                   # its pixels are local (row hi - lo)
        feats = precise_features(e, px_dino_local_halo, sorted(frames), lo) if frames else {}
        if not recompute_halo:
            sends = [(feats[lo].contiguous(), rank - 1)] if send_first else []
            recvs = []
            if cross:
                ref_rows = next(iter(feats.values()))
                buf = torch.empty_like(ref_rows)
                feats[hi] = buf
                recvs = [(buf, rank + 1)]
            self.comm.exchange(sends, recvs)
        dev = px_dino_local_halo.device
        local = e.pair_sims(feats, [(i, i + 1) for i in mine]) if mine else torch.zeros(0, dtype=torch.float32, device=dev)
        counts = [sum(1 for i in band if l <= i < h) for (l, h) in ranges]
        return self._all_gather_var(local.to(torch.float32), counts).tolist()

    def encode_video(self, px_siglip_local, px_dino_local_halo, T, image_size, n_text_tokens, prompt_ids, audio=None,
                     sample_indices=None, recompute_halo=False, cache=None, info=None):
        """px_siglip_local: frames [lo,hi) of the T frames that survive a1 (frame_plan); px_dino_local_halo: the same frames for
        the DINOv2 tower (the boundary frame's features are then exchanged), or frames [lo, hi + 1) - the next rank's first
        frame appended (none on the last rank) - with recompute_halo=True (on EVERY rank), to re-encode that frame here instead.  audio: as in the serial path - a full [T, 50, 768] token tensor, or a dict
        with "audio_tokens" / "beats_windows" (all windows) / "audio_wav" (raw 16 kHz waveform: BEATs runs here, on this
        rank's windows only); sample_indices: frame_plan's per-second vector (all ones when a1 did not cap).
        cache: a FrameCache (new_cache) of this rank's own frames - the result is bit for bit that of cache=None
        (_encode_cached); info then receives info["cache"].  cache=None: no collective besides those listed above.
        {"audio_pcm": audio.PcmAudio} becomes the waveform here, on every rank (encode.normalize_audio)."""
        audio = normalize_audio(self.e, audio)
        if cache is not None:
            return self._encode_cached(cache, px_siglip_local, px_dino_local_halo, T, image_size, n_text_tokens, prompt_ids,
                                       audio, sample_indices, recompute_halo, info)
        e, rank, world = self.e, self.rank, self.world
        ranges = seg.shard_ranges(T, world)
        lo, hi = ranges[rank]
        Tl = hi - lo
        cfg = e.cfg
        # 1. DINO (+halo) -> similarities -> identical segmentation everywhere
        n_d = px_dino_local_halo.shape[0]
        assert n_d == Tl + (1 if (recompute_halo and lo < hi < T) else 0) and px_siglip_local.shape[0] == Tl
        if Tl == 0:
            return self._pass_through(T, image_size, n_text_tokens, audio, ranges, px_siglip_local.device)
        side_sig = start_side_tower(e, px_siglip_local)
        dino_all = e.tower("dino", px_dino_local_halo)
        P = dino_all.shape[0] // n_d
        sig = None
        if T <= cfg.get("max_num_segments", 24) + 1:
            seg_idx = list(range(T))
        else:
            # T > 25 >= 3 * world: every rank owns frames
            if not recompute_halo:
                first = dino_all[:P].contiguous()
                halo_rows = torch.empty_like(first) if rank < world - 1 else None
                self.comm.exchange([(first, rank - 1)] if rank > 0 else [],
                                   [(halo_rows, rank + 1)] if rank < world - 1 else [])
                sims_local = self._local_sims(dino_all, Tl, P, halo_rows)
            else:                             # the halo frame is the last of the n_d frames encoded here
                sims_local = self._local_sims(dino_all, n_d, P, None)
            # the local SigLIP tower is enqueued before the exchange: the device works while the similarities travel - on a
            # side stream that waits only for the similarity kernels (engine.mark / after), so neither the collective nor
            # the host read queues behind the tower (with a host-side transport - gloo - the device is synchronised anyway)
            ev = e.mark() if (hasattr(e, "mark") and sims_local.is_cuda and not getattr(self.comm, "_host_side_now", lambda: True)()) \
                else None
            if side_sig is None:
                sig = e.tower("siglip", px_siglip_local)
            counts = [(h - l) - (0 if r < world - 1 else 1) for r, (l, h) in enumerate(ranges)]
            if ev is not None:
                with e.after(ev):
                    sims_local.record_stream(torch.cuda.current_stream(sims_local.device))
                    sims = self._all_gather_var(sims_local, counts).tolist()
            else:
                sims = self._all_gather_var(sims_local, counts).tolist()
            assert len(sims) == T - 1         # the same list on every rank: every rank joins the refinement's exchanges
            seg_idx = select_segments_with(e, sims, lambda b: self._refined_sims(b, px_dino_local_halo, ranges, recompute_halo))
        dino = dino_all[: Tl * P]
        # 2. local towers + connector (+ audio rows of the local frames)
        if sig is None:
            sig = join_side_tower(e, side_sig, px_siglip_local)
        X, sizes = e.connector(sig, dino, Tl, [tuple(image_size)] * Tl)
        N = X.shape[0] // Tl
        if sample_indices is None:
            sample_indices = [1] * T
        Xf, Nf = e.with_audio(X, Tl, N, e.local_audio(audio, sample_indices, T, lo, hi))
        return self._compress_gather(Xf, N, Nf, T, ranges, seg_idx, n_text_tokens, prompt_ids, X.device)

    def _local_sims(self, dino_all, n, P, halo_rows):
        """this rank's share of the T - 1 similarities from the DINOv2 rows of its n frames: the local pairs, then the pair
        across the right-hand boundary (halo_rows: the right neighbour's first frame, None on the last rank)"""
        parts = [self.e.sims_tensor(dino_all, n)] if n >= 2 else []
        if halo_rows is not None:
            parts.append(self.e.sims_tensor(torch.cat([dino_all[(n - 1) * P: n * P], halo_rows], 0), 2))
        return torch.cat(parts, 0) if parts else torch.zeros(0, dtype=torch.float32, device=dino_all.device)

    def _pass_through(self, T, image_size, n_text_tokens, audio, ranges, device):
        """a rank without frames: more ranks than frames (T < world <= 8 < max_num_segments + 1: the pass-through case, no
        similarities, no Q-Former) - this rank only takes part in the final all-gather"""
        e, cfg = self.e, self.e.cfg
        assert T <= cfg.get("max_num_segments", 24) + 1
        Nf = self._tokens_per_frame(image_size, audio)
        plan, learned = emission_plan(e, T, Nf, list(range(T)), visual_budget(cfg, n_text_tokens))
        pairs, _ = split_plan(plan, ranges, Nf, e.K)
        if not learned:
            self.comm.exchange([], [])
        return self._gather_tokens(lambda out: None, [len(p) for p in pairs], e.H, e.dtype, device)

    def _compress_gather(self, Xf, N, Nf, T, ranges, seg_idx, n_text_tokens, prompt_ids, device):
        """steps 3-4 on the local frames' rows Xf [Tl * Nf, Hp] (N visual rows per frame): the shared plan, the query hand-off,
        the Q-Former, the local emission and the token all-gather -> the whole stream"""
        e, rank, cfg = self.e, self.rank, self.e.cfg
        lo, hi = ranges[rank]
        K = e.K
        # 3. shared plan, query hand-off
        plan, learned = emission_plan(e, T, Nf, seg_idx, visual_budget(cfg, n_text_tokens))
        pairs, comp_local = split_plan(plan, ranges, Nf, K)
        keys = plan["key_frames"]
        my_comp = [gi for gi, f in enumerate(plan["comp_frames"]) if lo <= f < hi]
        pid = text_prompt(cfg, prompt_ids)
        comp = None
        if learned:
            if my_comp:
                comp = e.compress_frames(Xf, Nf, [plan["comp_frames"][gi] - lo for gi in my_comp], e.learned_queries(),
                                         [0] * len(my_comp), pid)
        else:
            need = sorted(set(plan["comp_chunk"][gi] for gi in my_comp))
            owned = [c for c, s in enumerate(keys) if lo <= s < hi]
            q_owned = e.make_queries(Xf, N, Nf, [keys[c] - lo for c in owned]) if owned else None
            users = {}                               # chunk -> ranks that hold compressed frames of it
            for gi, f in enumerate(plan["comp_frames"]):
                users.setdefault(plan["comp_chunk"][gi], set()).add(owner_of(f, ranges))
            sends, recvs, recv_buf = [], [], {}
            for ci, c in enumerate(owned):                   # ascending chunk id on both sides: pairwise order matches
                for r in sorted(users.get(c, ())):
                    if r != rank:
                        sends.append((q_owned[ci * K:(ci + 1) * K].contiguous(), r))
            for c in need:
                if not (lo <= keys[c] < hi):
                    buf = torch.empty((K, e.query_width()), dtype=e.dtype, device=device)
                    recv_buf[c] = buf
                    recvs.append((buf, owner_of(keys[c], ranges)))
            self.comm.exchange(sends, recvs)
            if my_comp:
                blocks = []
                for c in need:
                    if c in recv_buf:
                        blocks.append(recv_buf[c])
                    else:
                        ci = owned.index(c)
                        blocks.append(q_owned[ci * K:(ci + 1) * K])
                qtable = torch.cat(blocks, 0)
                qsrc = [need.index(plan["comp_chunk"][gi]) for gi in my_comp]
                comp = e.compress_frames(Xf, Nf, [plan["comp_frames"][gi] - lo for gi in my_comp], qtable, qsrc, pid)
        # 4. local emission + all-gather
        mine = pairs[rank]

        def emit_local(out):
            if getattr(e, "emit_into", None) is not None:
                e.emit_into(Xf, comp, mine, out)              # the a19 gather writes the send buffer directly
            else:
                out[: len(mine)].copy_(e.emit(Xf, comp, mine))
        return self._gather_tokens(emit_local, [len(p) for p in pairs], e.H, e.dtype, device)

    # ---- the frame cache ----------------------------------------------------------------------
    # Every rank caches its own frames in its own FrameCache.  Hits, misses, evictions and budget bypasses differ from rank
    # to rank; they change what a rank computes, never which collectives and point-to-point operations it issues: a skip that
    # would need a neighbour's cache state is agreed first through a small all-gather that every rank reads alike.
    AGREE_FIELDS = ("T", "n_text_tokens", "image_size[0]", "image_size[1]", "prompt length", "prompt fingerprint[0]",
                    "prompt fingerprint[1]", "audio", "seconds", "sample_indices fingerprint[0]",
                    "sample_indices fingerprint[1]", "pixel geometry fingerprint[0]", "pixel geometry fingerprint[1]",
                    "cache refuses the engine")

    def _agree(self, T, n_text_tokens, image_size, prompt_ids, audio, sample_indices, px_s, px_d, refused):
        """step 1 of the cached path: one all-gather of what must be the same sample on every rank (T, text length, image
        size, prompt ids, audio kind, the per-second vector - which carries T0 and the a1 cap -, the pixel geometry); a
        mismatch raises ValueError on every rank alike (all of them read the same gathered vectors), so none waits forever
        on a collective the others never reach"""
        def fp(b):
            b = np.frombuffer(bytes(b), dtype=np.uint8)
            return [int(v) for v in fingerprint_rows_host(b).view(np.int64)[0]] if b.size else [0, 0]
        pid = None if prompt_ids is None else np.asarray([int(v) for v in prompt_ids], dtype="<i8")
        kind = 0 if audio is None else 1 + sum(1 << i for i, k in enumerate(("audio_tokens", "beats_windows", "audio_wav"))
                                               if isinstance(audio, dict) and audio.get(k) is not None)
        geom = repr((str(px_s.dtype), tuple(px_s.shape[1:]), str(px_d.dtype), tuple(px_d.shape[1:]))).encode()
        vec = [T, n_text_tokens, int(image_size[0]), int(image_size[1]), -1 if pid is None else len(pid)] + \
            (fp(b"") if pid is None else fp(pid.tobytes())) + [kind, len(sample_indices)] + \
            fp(np.asarray([int(v) for v in sample_indices], dtype=np.int8).tobytes()) + fp(geom) + [int(refused is not None)]
        got = [g.tolist() for g in self.comm.all_gather(torch.tensor(vec, dtype=torch.int64, device=px_s.device))]
        if any(g[-1] for g in got):
            raise ValueError("ShardedVideoEncoder.encode_video(cache=...): the frame cache of rank(s) %s was made for other "
                             "engine settings%s" % ([r for r, g in enumerate(got) if g[-1]],
                                                    "" if refused is None else " (%s)" % (refused,)))
        bad = sorted({self.AGREE_FIELDS[j] for g in got for j in range(len(vec)) if g[j] != got[0][j]})
        if bad:
            raise ValueError("ShardedVideoEncoder.encode_video(cache=...): the ranks were given different samples (%s differ); "
                             "every rank must be called with the same video and prompt" % ", ".join(bad))

    def _refined_sims_cached(self, band, px_d, ranges, cache, dk, stats):
        """_refined_sims with this rank's cache (None: a bypassing rank): band pairs whose precise value the cache holds are not
        re-encoded.  Whether the right neighbour must send the precise rows of its first frame depends on this rank's cache:
        one all-gather of per-rank "my boundary pair is in the band and not cached" flags gives every rank the same
        send / receive list (no flag set: no exchange, on every rank).  dk: the DINOv2 keys of the local frames and, last, of
        the right neighbour's first frame.  -> the refined values of the whole band in band order, on every rank."""
        e, rank, world = self.e, self.rank, self.world
        lo, hi = ranges[rank]
        dev = px_d.device
        mine = [i for i in band if lo <= i < hi]

        def pk(i):
            return ("precise", dk[i - lo], dk[i - lo + 1])
        vals = {i: (None if cache is None else cache.pair_get(pk(i))) for i in mine}
        todo = [i for i in mine if vals[i] is None]
        cross = rank < world - 1 and (hi - 1) in todo
        flags = torch.cat(self.comm.all_gather(torch.tensor([int(cross)], dtype=torch.int64, device=dev))).tolist()
        send_first = rank > 0 and flags[rank - 1] == 1
        frames = {f for i in todo for f in (i, i + 1) if f < hi}
        if send_first:
            frames.add(lo)
        feats = precise_features(e, px_d, sorted(frames), lo) if frames else {}
        stats["precise_frames_computed"] += len(frames)
        if any(flags):
            sends = [(feats[lo].contiguous(), rank - 1)] if send_first else []
            recvs = []
            if cross:
                buf = torch.empty_like(next(iter(feats.values())))
                feats[hi] = buf
                recvs = [(buf, rank + 1)]
            self.comm.exchange(sends, recvs)
        if todo:
            for i, v in zip(todo, e.pair_sims(feats, [(i, i + 1) for i in todo]).tolist()):
                vals[i] = float(v)
                if cache is not None:
                    cache.put_computed(pk(i), v)
        local = torch.tensor([vals[i] for i in mine], dtype=torch.float32, device=dev)
        counts = [sum(1 for i in band if l <= i < h) for (l, h) in ranges]
        return self._all_gather_var(local, counts).tolist()

    def _encode_cached(self, cache, px_s, px_d, T, image_size, n_text_tokens, prompt_ids, audio, sample_indices,
                       recompute_halo, info):
        """encode_video through this rank's FrameCache, bit for bit the uncached result (encode.encode_video_cached, per
        rank): 1. sample agreement (_agree); 2. the local frames are fingerprinted where they lie, only those the cache lacks
        run through the towers and the connector (a rank whose frames exceed its budget runs them uncached and stores
        nothing); 3. local similarities from the cache / the slab, the boundary exchange as in the uncached path plus the
        128-bit DINOv2 key of the first frame, so the left rank can look the pair across the boundary up; 4. the refinement
        through the cache (_refined_sims_cached); 5. connector rows out of the slab, BEATs windows through the cache; 6. the
        prompt-dependent steps as in the uncached path."""
        e, rank, world = self.e, self.rank, self.world
        if recompute_halo:
            raise ValueError("ShardedVideoEncoder.encode_video: recompute_halo=True does not combine with a frame cache "
                             "(the cached path exchanges the boundary frame's DINOv2 rows and key)")
        refused = None
        try:
            cache.bind(e)
        except ValueError as ex:           # raised on every rank by _agree: no rank is left waiting in a collective
            refused = ex
        cfg = e.cfg
        ranges = seg.shard_ranges(T, world)
        lo, hi = ranges[rank]
        Tl = hi - lo
        if sample_indices is None:
            sample_indices = [1] * T
        dev = px_s.device
        self._agree(T, n_text_tokens, image_size, prompt_ids, audio, sample_indices, px_s, px_d, refused)  # 1.
        assert px_s.shape[0] == Tl and px_d.shape[0] == Tl
        before = cache.stats()
        stats = dict(rank=rank, bypassed=False, frames=Tl, frames_hit=0, frames_encoded=0, pairs_computed=0, evictions=0,
                     bytes=before["bytes"], windows_encoded=0, precise_frames_computed=0)
        if Tl == 0:
            if info is not None:
                info["cache"] = stats
            return self._pass_through(T, image_size, n_text_tokens, audio, ranges, dev)
        # 2. keys, the frames this rank lacks
        idx = list(range(Tl))
        keys, dkeys = cache.frame_keys(e, px_s, px_d, idx, image_size)
        segmented = T > cfg.get("max_num_segments", 24) + 1
        early = {}                             # local pairs of two new frames, enqueued BEFORE the SigLIP tower
        new = encode_missing(e, cache, keys, px_s, px_d, idx, image_size, lambda new, dino: early.update(
            cache.early_sims(e, keys, dkeys, new, dino, segmented))) if cache.fits(keys) else None
        bypass = new is None
        if bypass:                             # over this rank's budget: its towers run uncached, nothing is stored
            early.clear()
            side_sig = start_side_tower(e, px_s)
            dino_all = e.tower("dino", px_d)
            sig = join_side_tower(e, side_sig, px_s)
            P = dino_all.shape[0] // Tl
        # 3. similarities
        if not segmented:
            seg_idx = list(range(T))
        else:
            first = dino_all[:P] if bypass else cache.dino_rows(keys[0])
            Pr, Dp = first.shape
            sends, recvs = [], []
            if rank > 0:
                u = [(v - (1 << 64)) if v >= 1 << 63 else v for v in dkeys[0][0]]
                sends = [(first, rank - 1), (torch.tensor(u, dtype=torch.int64, device=dev), rank - 1)]
            pair_buf = key_buf = None
            if rank < world - 1:
                pair_buf = torch.empty(2, Pr, Dp, dtype=first.dtype, device=first.device)   # [my last frame, the halo]
                key_buf = torch.empty(2, dtype=torch.int64, device=dev)
                recvs = [(pair_buf[1], rank + 1), (key_buf, rank + 1)]
            self.comm.exchange(sends, recvs)
            right = None
            if key_buf is not None:
                right = (tuple(v & 0xFFFFFFFFFFFFFFFF for v in key_buf.tolist()), dkeys[0][1])
            if bypass:
                sims_local = self._local_sims(dino_all, Tl, P, None if pair_buf is None else pair_buf[1])
            else:
                local = cache.adjacent_sims(e, keys, dkeys, early)
                if right is not None:
                    pkey = (dkeys[-1], right)
                    v = cache.pair_get(pkey)
                    if v is None:
                        pair_buf[0].copy_(cache.dino_rows(keys[-1]))
                        v = float(e.slot_sims(pair_buf, [(0, 1)])[0])
                        cache.put_computed(pkey, v)
                    local.append(v)
                sims_local = torch.tensor(local, dtype=torch.float32, device=dev)
            counts = [(h - l) - (0 if r < world - 1 else 1) for r, (l, h) in enumerate(ranges)]
            sims = self._all_gather_var(sims_local, counts).tolist()
            assert len(sims) == T - 1
            # 4. the selection refinement
            dk = list(dkeys) + ([right] if right is not None else [])
            seg_idx = select_segments_with(e, sims, lambda b: self._refined_sims_cached(b, px_d, ranges, None if bypass else cache,
                                                                                       dk, stats))
        # 5. connector rows and audio rows of the local frames
        if bypass:
            X, _ = e.connector(sig, dino_all[: Tl * P], Tl, [tuple(image_size)] * Tl)
            N = X.shape[0] // Tl
            a_local = e.local_audio(audio, sample_indices, T, lo, hi)
        else:
            X = cache.assemble(e, keys)
            N = cache.rows_per_frame
            a_local = None if audio is None else cached_audio(e, cache, audio, sample_indices, T, lo, hi)
        Xf, Nf = e.with_audio(X, Tl, N, a_local)
        out = self._compress_gather(Xf, N, Nf, T, ranges, seg_idx, n_text_tokens, prompt_ids, dev)        # 6.
        if info is not None:
            stats.update(cache.call_info(before, cache.stats(), keys, new or ()))
            if bypass:
                stats.update(bypassed=True, frames_hit=0, frames_encoded=Tl)
            info["cache"] = stats
        return out
