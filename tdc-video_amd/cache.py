"""Content-keyed frame cache: encode a video once, answer many prompts (encode.encode_video_cached).

Everything from the pixels up to the connector rows (a3/a4 towers, a5 similarities, a6-a10 connector) depends on the frame
pixels and image_size alone, and frames are independent through it, bit for bit.  FrameCache keeps, per frame content:

  (fp_siglip, fp_dino, image_size, pixel types / shapes)  ->  the frame's connector rows X [N, Hp] and DINOv2 rows [P, Dp]
  (dino key a, dino key b)                                ->  the a5 similarity of the pair (a host float)
  ("precise", dino key a, dino key b)                     ->  the refined (fp16-tower) similarity of the pair
  (BEATs window: fingerprints of its waveform and mask slices) -> that window's features [1, L_w, C]

Keys are 128-bit content fingerprints (tdc_fingerprint_rows on the device, fingerprint_rows_host here), so a caller that
decodes the same video again hits, and identical frames share one slot.  The fingerprint is not cryptographic: keys are assumed
collision-free for honest inputs, not against crafted collisions.  The frame rows live in two slabs of fixed-size slots
([slots, N, Hp] and [slots, P, Dp]) that grow up to the byte budget; frames are evicted least recently used first, never one
the running call needs, and the stored bytes never exceed the budget.  BEATs window features take at most 1/16 of the budget
(AUDIO_SHARE), the frames the rest.

Kept cross-attention K/V (kv_bytes > 0): the Q-Former's stacked K/V projection of a call's compressed
frames reads their connector rows alone, so it is a property of the (video, a1 selection), not of the prompt.  One entry per
such selection - a device buffer [U * Nf, n_cross * 2 * dim] under a key made of the frames' content keys (encode.kv_key) -
lives in a budget of its own (kv_bytes), least recently used entries leaving first.  Its counters are kv_stats(); stats(),
bytes and the frame budget do not know about it.
"""
from collections import OrderedDict

import numpy as np
import torch

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_S1 = np.uint64(0x243F6A8885A308D3)
_S2 = np.uint64(0x13198A2E03707344)


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fingerprint_rows_host(rows):
    """The 128-bit fingerprint of tdc_fingerprint_rows in numpy.  rows: a 2-D uint8 array [n, row_bytes] (or anything
    np.asarray makes one of; a 1-D byte row counts as one row) -> uint64 [n, 2].
    Words w_i = the row as little-endian u64 (tail zero-padded); x_i = w_i ^ (i * golden); h_k = mix(sum_i mix(x_i ^ S_k) ^
    row_bytes), sums mod 2^64, mix = the splitmix64 finaliser."""
    a = np.asarray(rows, dtype=np.uint8)
    if a.ndim == 1:
        a = a[None]
    n, nb = a.shape
    nw = (nb + 7) // 8
    if nw * 8 != nb:
        a = np.concatenate([a, np.zeros((n, nw * 8 - nb), dtype=np.uint8)], 1)
    w = np.ascontiguousarray(a).view("<u8").astype(np.uint64, copy=False)
    with np.errstate(over="ignore"):
        x = w ^ (np.arange(nw, dtype=np.uint64) * _GOLDEN)[None]
        h1 = _mix(x ^ _S1).sum(1, dtype=np.uint64)
        h2 = _mix(x ^ _S2).sum(1, dtype=np.uint64)
        ln = np.uint64(nb)
        return np.stack([_mix(h1 ^ ln), _mix(h2 ^ ln)], 1)


def tensor_rows_host(x, rows):
    """the bytes of x[r] for r in rows as a uint8 array [len(rows), bytes per x[0]] (host tensors; the CPU engine double)"""
    b = x.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().reshape(x.shape[0], -1)
    return b[np.asarray(list(rows), dtype=np.int64)]


def engine_signature(e):
    """the engine settings that change the cached rows: 16-bit types, fp8 levels, LayerNorm folding, native composites"""
    towers = getattr(e, "towers", {}) or {}
    tw = tuple(sorted((k, str(t.get("dtype") if hasattr(t, "get") else None), int(getattr(t, "fp8", 0) or 0),
                       bool(getattr(t, "fused", False))) for k, t in towers.items()))
    return (type(e).__name__, str(getattr(e, "dtype", None)), str(getattr(e, "tower_dtype", None)),
            str(getattr(e, "tower_res_dtype", None)), tw, bool(getattr(e, "native_towers", True)),
            bool(getattr(e, "native_connector", True)), getattr(e, "selection_eps", None))


class KeptKV:
    """compress_frames' kv= value: the kept K/V buffer of a call's compressed frames and whether an earlier pass filled it"""
    __slots__ = ("buf", "ready")

    def __init__(self, buf, ready):
        self.buf, self.ready = buf, bool(ready)


class FrameCache:
    """Connector rows, DINOv2 rows and similarities of frames already encoded, keyed by content (module docstring).
    max_bytes: budget of the stored rows (slab slots actually allocated never exceed it either).  kv_bytes: budget of the
    kept cross-attention K/V entries, 0 = none are kept."""
    AUDIO_SHARE = 16                             # BEATs windows: at most max_bytes // AUDIO_SHARE

    def __init__(self, max_bytes, signature=None, kv_bytes=0):
        self.max_bytes = int(max_bytes)
        if self.max_bytes <= 0:
            raise ValueError("FrameCache needs a positive byte budget, got %r" % (max_bytes,))
        self.kv_max_bytes = int(kv_bytes)
        if self.kv_max_bytes < 0:
            raise ValueError("FrameCache needs a K/V byte budget >= 0, got %r" % (kv_bytes,))
        self.signature = signature
        self._pairs = OrderedDict()              # (dkey a, dkey b) / ("precise", ...) -> float
        self.clear()

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def clear(self):
        """empty the store (and release its device slabs); the counters restart"""
        self._clear_rows()
        self._pairs.clear()
        self._audio = OrderedDict()              # window key -> features, least recently used first
        self._audio_bytes = 0
        self._counts = dict(hits=0, misses=0, frames_encoded=0, pairs_computed=0, evictions=0, windows_encoded=0,
                            windows_hit=0)
        self._kv = OrderedDict()                 # encode.kv_key -> (buffer, bytes), least recently used first
        self._kv_bytes = 0
        self._kv_counts = dict(hits=0, misses=0, fills=0, evictions=0, bypassed=0)

    def _clear_rows(self):
        self._slots = OrderedDict()              # key -> slot, least recently used first
        self._final = {}                         # key -> the connector's final size of the frame
        self._free = []
        self._geom = None                        # (N, Hp, X dtype, P, Dp, DINOv2 dtype, device)
        self._X = self._D = None

    def bind(self, e):
        """refuse an engine whose row-changing settings differ from those the cache was made for"""
        sig = engine_signature(e)
        if self.signature is None:
            self.signature = sig
        elif sig != self.signature:
            raise ValueError("FrameCache was made for engine settings %r, not %r" % (self.signature, sig))

    @property
    def frame_bytes(self):
        if self._geom is None:
            return 0
        N, Hp, xdt, P, Dp, ddt, _ = self._geom
        return N * Hp * torch.empty(0, dtype=xdt).element_size() + P * Dp * torch.empty(0, dtype=ddt).element_size()

    @property
    def capacity(self):
        """frames the budget holds at the current geometry (None before the first frame is stored)"""
        return None if self._geom is None else (self.max_bytes - self.audio_budget) // self.frame_bytes

    @property
    def audio_budget(self):
        return self.max_bytes // self.AUDIO_SHARE

    @property
    def bytes(self):
        return len(self._slots) * self.frame_bytes + self._audio_bytes

    @property
    def reserved_bytes(self):
        return (0 if self._X is None else self._X.shape[0] * self.frame_bytes) + self._audio_bytes

    def stats(self):
        return dict(self._counts, frames=len(self._slots), bytes=self.bytes, reserved_bytes=self.reserved_bytes,
                    max_bytes=self.max_bytes, pairs=len(self._pairs), windows=len(self._audio), audio_bytes=self._audio_bytes)

    def __len__(self):
        return len(self._slots)

    def __contains__(self, key):
        return key in self._slots

    # ------------------------------------------------------------------------------------------------ keys
    @staticmethod
    def frame_keys(e, px_siglip, px_dino, idx, image_size):
        """-> (frame keys, DINOv2 keys) of the frames idx of the two pixel tensors, from one fingerprint launch per tensor"""
        fs = e.fingerprint(px_siglip, idx)
        fd = e.fingerprint(px_dino, idx)
        gs = (str(px_siglip.dtype), tuple(px_siglip.shape[1:]))
        gd = (str(px_dino.dtype), tuple(px_dino.shape[1:]))
        dkeys = [(tuple(d), gd) for d in fd]
        keys = [(tuple(s), gs, dk, tuple(image_size)) for s, dk in zip(fs, dkeys)]
        return keys, dkeys

    # ------------------------------------------------------------------------------------------------ frames
    def lookup(self, keys):
        """-> the keys among `keys` not stored (unique, in first-appearance order); the stored ones become most recent"""
        new, seen = [], set()
        for k in keys:
            if k in self._slots:
                self._slots.move_to_end(k)
                self._counts["hits"] += 1
            else:
                self._counts["misses"] += 1
                if k not in seen:
                    seen.add(k)
                    new.append(k)
        return new

    def fits(self, keys):
        """whether the distinct frames of one call fit the budget at the current geometry (unknown geometry: assumed)"""
        cap = self.capacity
        return cap is None or len(set(keys)) <= cap

    def store(self, keys, X, D, final_sizes, pinned):
        """the rows of the new frames `keys` (X [n * N, Hp], D [n * P, Dp], one block per key) into free or evicted slots.
        pinned: the keys the running call still reads - never evicted.  -> False (nothing stored) when the call's frames do
        not fit the budget."""
        n = len(keys)
        if n == 0:
            return True
        geom = (X.shape[0] // n, X.shape[1], X.dtype, D.shape[0] // n, D.shape[1], D.dtype, X.device)
        if self._geom != geom:
            if self._geom is not None:           # another row geometry (another image size): one geometry at a time
                self._counts["evictions"] += len(self._slots)
                self._clear_rows()
            self._geom = geom
        cap = self.capacity
        if len(set(pinned) | set(keys)) > cap:
            return False
        while len(self._slots) + n > cap:
            victim = next(k for k in self._slots if k not in pinned)
            self._free.append(self._slots.pop(victim))
            self._final.pop(victim, None)
            self._counts["evictions"] += 1
        need = len(self._slots) + n
        self._grow(need)
        slots = [self._free.pop() for _ in range(n)]
        N, Hp, _, P, Dp, _, dev = geom
        st = torch.tensor(slots, dtype=torch.long).to(dev, non_blocking=True)
        self._X.index_copy_(0, st, X.view(n, N, Hp))
        self._D.index_copy_(0, st, D.view(n, P, Dp))
        for k, s, f in zip(keys, slots, final_sizes):
            self._slots[k] = s
            self._final[k] = f
        self._counts["frames_encoded"] += n
        return True

    def _grow(self, need):
        have = 0 if self._X is None else self._X.shape[0]
        if need <= have:
            return
        N, Hp, xdt, P, Dp, ddt, dev = self._geom
        new = min(self.capacity, max(need, 2 * have, 16))
        X = torch.empty(new, N, Hp, dtype=xdt, device=dev)
        D = torch.empty(new, P, Dp, dtype=ddt, device=dev)
        if have:
            X[:have].copy_(self._X)
            D[:have].copy_(self._D)
        self._X, self._D = X, D
        self._free = list(range(new - 1, have - 1, -1)) + self._free

    def slots(self, keys):
        return [self._slots[k] for k in keys]

    def final_sizes(self, keys):
        return [self._final[k] for k in keys]

    @property
    def rows_per_frame(self):
        return self._geom[0]

    def dino_rows(self, key):
        """the DINOv2 rows [P, Dp] of a stored frame: a view of its slab slot (contiguous)"""
        return self._D[self._slots[key]]

    def assemble(self, e, keys):
        """the connector rows of the frames `keys`, in order -> [len(keys) * N, Hp] (one row gather out of the slab)"""
        N, Hp = self._geom[0], self._geom[1]
        s = np.asarray(self.slots(keys), dtype=np.int64)
        idx = np.zeros((len(keys) * N, 2), dtype=np.int32)
        idx[:, 1] = (s[:, None] * N + np.arange(N)[None]).reshape(-1)       # slots < capacity: rows inside the slab
        src = torch.from_numpy(idx).to(self._X.device, non_blocking=True)
        return e.compact_rows(self._X.view(-1, Hp), src, Hp)

    # ------------------------------------------------------------------------------------------------ similarities
    def _pair_cap(self):
        return 16 * (self.capacity or 0) + 4096

    def pair_get(self, key):
        v = self._pairs.get(key)
        if v is not None:
            self._pairs.move_to_end(key)
        return v

    def pair_put(self, key, value):
        self._pairs[key] = float(value)
        self._pairs.move_to_end(key)
        while len(self._pairs) > self._pair_cap():
            self._pairs.popitem(last=False)

    def put_computed(self, key, value):
        """pair_put of a similarity this call computed (counted in pairs_computed)"""
        self.pair_put(key, value)
        self._counts["pairs_computed"] += 1

    def early_sims(self, e, keys, dkeys, new, dino, segmented=True):
        """encode_missing's after_dino: a5 of the adjacent pairs of `keys` whose frames are both `new`, from their fresh DINOv2
        rows, enqueued BEFORE the SigLIP tower and read while it runs (as encode.towers_and_selection does); pairs with a
        stored frame come from the slab later.  -> the `early` dict of adjacent_sims ({}: not segmented, or no such pair)"""
        pos = {k: j for j, k in enumerate(new)}
        todo = [i for i in range(len(keys) - 1) if keys[i] in pos and keys[i + 1] in pos and
                self.pair_get((dkeys[i], dkeys[i + 1])) is None]
        if not (segmented and todo):
            return {}
        slab = dino.view(len(new), dino.shape[0] // len(new), dino.shape[1])
        return dict(pairs=todo, read=e.slot_sims(slab, [(pos[keys[i]], pos[keys[i + 1]]) for i in todo], defer=True))

    @staticmethod
    def call_info(before, after, keys, new):
        """info["cache"] of one call over the frames `keys`, of which it encoded the `new` ones: stats() before and after it"""
        fresh = set(new)
        return dict(bypassed=False, frames=len(keys), frames_hit=sum(1 for k in keys if k not in fresh),
                    frames_encoded=after["frames_encoded"] - before["frames_encoded"],
                    pairs_computed=after["pairs_computed"] - before["pairs_computed"],
                    evictions=after["evictions"] - before["evictions"], bytes=after["bytes"],
                    windows_encoded=after["windows_encoded"] - before["windows_encoded"])

    def adjacent_sims(self, e, keys, dkeys, early=None):
        """a5: the T - 1 adjacent-frame similarities of the frames `keys` - stored values, those already enqueued (early:
        {"pairs": pair indices, "read": function -> their values}), the rest from the DINOv2 slab (tdc_pair_cossim on the
        slots, one launch)"""
        pk = [(dkeys[i], dkeys[i + 1]) for i in range(len(keys) - 1)]
        sims = [self.pair_get(k) for k in pk]
        if early and early.get("pairs"):
            for i, v in zip(early["pairs"], early["read"]()):
                sims[i] = float(v)
                self.pair_put(pk[i], v)
            self._counts["pairs_computed"] += len(early["pairs"])
        todo = [i for i, v in enumerate(sims) if v is None]
        if todo:
            s = self.slots(keys)
            vals = e.slot_sims(self._D, [(s[i], s[i + 1]) for i in todo])
            for i, v in zip(todo, vals):
                sims[i] = float(v)
                self.pair_put(pk[i], v)
            self._counts["pairs_computed"] += len(todo)
        return sims

    def precise_sims(self, band, dkeys, compute):
        """refine(band) of select_segments_with: the fp16-tower similarities of the pairs (i, i + 1) in band - stored values,
        the rest from compute(pairs) (a list of floats)"""
        pk = [("precise", dkeys[i], dkeys[i + 1]) for i in band]
        vals = [self.pair_get(k) for k in pk]
        todo = [j for j, v in enumerate(vals) if v is None]
        if todo:
            got = compute([band[j] for j in todo])
            for j, v in zip(todo, got):
                vals[j] = float(v)
                self.pair_put(pk[j], v)
            self._counts["pairs_computed"] += len(todo)
        return vals

    # ------------------------------------------------------------------------------------------------ kept K/V
    @property
    def kv_enabled(self):
        return self.kv_max_bytes > 0

    def kv_stats(self):
        return dict(self._kv_counts, entries=len(self._kv), bytes=self._kv_bytes, max_bytes=self.kv_max_bytes)

    def kv_clear(self):
        """drop the kept K/V entries (and release their device memory); the frames and every counter stay"""
        self._kv.clear()
        self._kv_bytes = 0

    def kv_get(self, key):
        """the buffer kept under `key` (it becomes the most recent entry), or None"""
        hit = self._kv.get(key)
        if hit is None:
            self._kv_counts["misses"] += 1
            return None
        self._kv.move_to_end(key)
        self._kv_counts["hits"] += 1
        return hit[0]

    def kv_room(self, nbytes, pinned=()):
        """make room for a new entry of nbytes BEFORE the caller allocates it: least recently used entries leave until it
        fits, never one of `pinned` (the keys the running call has used).  -> False (nothing evicted) when the entry exceeds
        the budget, or what the pinned entries leave of it."""
        held = sum(nb for k, (_, nb) in self._kv.items() if k in pinned)
        if nbytes + held > self.kv_max_bytes:
            self._kv_counts["bypassed"] += 1
            return False
        while self._kv_bytes + nbytes > self.kv_max_bytes:
            victim = next(k for k in self._kv if k not in pinned)
            self._kv_bytes -= self._kv.pop(victim)[1]
            self._kv_counts["evictions"] += 1
        return True

    def kv_put(self, key, buf, nbytes):
        """keep the filled buffer under `key` (kv_room(nbytes) said it fits)"""
        assert key not in self._kv and self._kv_bytes + nbytes <= self.kv_max_bytes
        self._kv[key] = (buf, nbytes)
        self._kv_bytes += nbytes
        self._kv_counts["fills"] += 1

    # ------------------------------------------------------------------------------------------------ BEATs windows
    def windows(self, keys, encode):
        """{w: features} of the BEATs windows keyed keys = {w: key}: stored ones, the rest from encode(windows) -> {w: features}
        (stored while they fit the audio share, least recently used windows evicted first, never one of this call)"""
        out, todo = {}, []
        for w, k in keys.items():
            f = self._audio.get(k)
            if f is None:
                todo.append(w)
            else:
                self._audio.move_to_end(k)
                out[w] = f
        self._counts["windows_hit"] += len(out)
        if todo:
            got = encode(todo)
            self._counts["windows_encoded"] += len(todo)
            pinned = set(keys.values())
            for w in todo:
                f = got[w]
                nb = f.numel() * f.element_size()
                while self._audio_bytes + nb > self.audio_budget:
                    victim = next((k for k in self._audio if k not in pinned), None)
                    if victim is None:
                        break
                    self._audio_bytes -= self._nbytes(self._audio.pop(victim))
                    self._counts["evictions"] += 1
                if self._audio_bytes + nb <= self.audio_budget:
                    self._audio[keys[w]] = f
                    self._audio_bytes += nb
                out[w] = f
        return out

    @staticmethod
    def _nbytes(t):
        return t.numel() * t.element_size()
