"""CPU: the frame cache of the frame-sharded path (dist.ShardedVideoEncoder.encode_video(cache=...), config.tdc_shard_cache_bytes)
on the cache-capable CPU engine doubles of test_video_cache.py.  Every rank caches its own frames; the cached result must be
bit for bit the uncached sharded one (itself the serial one) whatever each rank's cache holds, and no cache state may make
the ranks issue different collectives: the thread worlds join with a bound, so a hang fails the test."""
import os
import threading

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import tdc_video_amd  # noqa: F401
from tdc_video_amd import pipeline
from tdc_video_amd.cache import FrameCache, engine_signature
from tdc_video_amd.dist import ShardedVideoEncoder
from tdc_video_amd import segment as seg
from test_dist_gloo import MixinEngine, _free_port, make_video
from test_video_cache import CFake, _CacheMixin, _ccase, _enc
from util import ThreadComm

BIG = 1 << 30
NAMES = ["plain61", "audio61", "learned61", "refine61", "passthrough20", "cap90_audio"]


def _new_cache(eng, nbytes=BIG):
    return FrameCache(nbytes, engine_signature(eng))


def _rank_call(eng, vid, audio, cap, rank, world, comm, cache, btl=4, prompt=(1, 2), info=None):
    sh = ShardedVideoEncoder(eng, rank, world, comm=comm)
    fp = sh.frame_plan(vid.shape[0], budget_text_len=btl, frame_cap=cap)
    return sh.encode_video(vid[fp["siglip_frames"]], vid[fp["dino_frames"]], fp["T"], (384, 384), n_text_tokens=4 + len(prompt),
                           prompt_ids=list(prompt), audio=audio, sample_indices=fp["sample_indices"], cache=cache, info=info)


def _run_world(world, fn, timeout=60, abort_on_error=True):
    """rank r runs fn(r, comm) on its own thread -> (results, errors by rank); a rank still running after `timeout` seconds
    fails the test (the peers are released through the barrier).  abort_on_error=False: an error does not break the barrier
    (where every rank is to raise its own error - a broken barrier would hand the slower ranks BrokenBarrierError)."""
    hub = ThreadComm.Hub(world)
    out, err = [None] * world, {}

    def run(r):
        try:
            out[r] = fn(r, ThreadComm(hub, r))
        except BaseException as ex:      # noqa: BLE001 - release the peers, report in the main thread
            err[r] = ex
            if abort_on_error:
                hub.bar.abort()
    ts = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    hung = [r for r, t in enumerate(ts) if t.is_alive()]
    if hung:
        hub.bar.abort()
        pytest.fail("ranks %s did not finish within %d s (a collective out of step)" % (hung, timeout))
    return out, err


class World:
    """`world` ranks, each with its own engine double and cache, kept across calls (as the processes of a serving job)"""

    def __init__(self, name, world, budgets=None, eng=None, vid=None):
        self.world = world
        self.ranks = []
        for r in range(world + 1):                   # the last one: the serial reference's own engine
            e, v, a, c = _ccase(name)
            if eng is not None:
                e = eng()
            self.ranks.append([e, v if vid is None else vid, a, c])
        self.ref = self.ranks.pop()
        self.caches = [_new_cache(rk[0], (budgets or {}).get(r, BIG)) for r, rk in enumerate(self.ranks)]

    def call(self, btl=4, prompt=(1, 2), cached=True, prompts=None):
        infos = [{} for _ in range(self.world)]

        def fn(r, comm):
            e, v, a, c = self.ranks[r]
            return _rank_call(e, v, a, c, r, self.world, comm, self.caches[r] if cached else None, btl,
                              prompts[r] if prompts else prompt, infos[r])
        out, err = _run_world(self.world, fn)
        if err:
            raise next(iter(err.values()))
        return out, [i.get("cache") for i in infos]

    def towers(self):
        return [getattr(rk[0], "tower_frames", 0) for rk in self.ranks]

    def serial(self, btl=4, prompt=(1, 2)):
        e, v, a, c = self.ref
        return _enc(e, v, a, c, btl=btl, prompt=prompt)


def _all_equal(outs, want):
    for r, o in enumerate(outs):
        assert o.shape == want.shape and torch.equal(o, want), "rank %d differs" % r


# ------------------------------------------------------------------------------------------------ thread worlds
@pytest.mark.parametrize("world", [3, 4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_cold_and_second_question(name, world):
    w = World(name, world)
    want = w.serial()
    unc, _ = w.call(cached=False)
    _all_equal(unc, want)
    cold, ci = w.call()
    _all_equal(cold, want)
    assert all(not c["bypassed"] and c["frames_encoded"] == c["frames"] for c in ci)
    assert sorted(c["rank"] for c in ci) == list(range(world)) and sum(c["frames"] for c in ci) == len(w.ranks[0][1]) \
        or name.startswith("cap")
    towers = w.towers()
    want2 = w.serial(prompt=(5, 6, 7))
    warm, wi = w.call(prompt=(5, 6, 7))
    _all_equal(warm, want2)
    assert w.towers() == towers, "a tower ran on a warm call"
    for c in wi:
        assert c["frames_encoded"] == 0 and c["frames_hit"] == c["frames"] and c["pairs_computed"] == 0
        assert c["precise_frames_computed"] == 0 and c["windows_encoded"] == 0


def test_more_ranks_than_frames():
    """T = 5 < world = 8: three ranks own no frame (the pass-through case) and still take part in every collective"""
    e, v, a, c = _ccase("passthrough20")
    w = World("passthrough20", 8, vid=v[:5])
    want = w.serial()
    for _ in range(2):
        got, info = w.call()
        _all_equal(got, want)
    assert [i["frames"] for i in info] == [1, 1, 1, 1, 1, 0, 0, 0] and all(i["frames_encoded"] == 0 for i in info)


def test_prompt_that_changes_the_frame_count_moves_the_shards():
    """btl 4 keeps 60 frames of 90, btl 40 keeps 58 (a1 budget): the shard ranges move, each rank encodes only the frames
    new to it"""
    _, vid, _, _ = _ccase("plain61")
    vid = torch.cat([vid, vid[:29] + 100.0])
    world = 4
    w = World("plain61", world, eng=lambda: CFake(max_len=16 + 4 + 20 * 60), vid=vid)
    for rk in w.ranks + [w.ref]:
        rk[3] = 10 ** 6
    eng = w.ranks[0][0]
    seen = []
    for btl, prompt in ((4, (1, 2)), (40, (5, 6, 7, 8, 9))):
        want = w.serial(btl, prompt)
        got, info = w.call(btl, prompt)
        _all_equal(got, want)
        idx = pipeline.frame_indices(eng.cfg, 90, btl, 10 ** 6)
        seen.append([set(idx[lo:hi]) for lo, hi in seg.shard_ranges(len(idx), world)])
    assert len(idx) == 58
    new = [len(b - a) for a, b in zip(*seen)]
    assert [i["frames_encoded"] for i in info] == new and 0 < sum(new) < 58


@pytest.mark.parametrize("world", [3, 4, 8])
@pytest.mark.parametrize("name", ["plain61", "refine61", "audio61", "learned61"])
def test_asymmetric_cache_states(name, world):
    # rank 0 warm, the others cleared
    w = World(name, world)
    want = w.serial()
    _all_equal(w.call()[0], want)
    for c in w.caches[1:]:
        c.clear()
    got, info = w.call()
    _all_equal(got, want)
    assert info[0]["frames_encoded"] == 0 and all(i["frames_encoded"] == i["frames"] for i in info[1:])
    # one rank with a budget below its shard: it bypasses its cache, the others cache
    small = world // 2
    fb = (5 * 8 + 4 * 8) * 4
    w = World(name, world, budgets={small: 2 * fb})
    for _ in range(2):
        got, info = w.call()
        _all_equal(got, want)
        assert info[small]["bypassed"] and not any(i["bypassed"] for r, i in enumerate(info) if r != small)
    assert w.caches[small].bytes <= w.caches[small].max_bytes
    assert all(i["frames_encoded"] == 0 for r, i in enumerate(info) if r != small)
    # one rank loses part of its frames between calls (evicted by other content)
    r = world - 1 if world > 3 else 1
    lo, hi = seg.shard_ranges(61, world)[r]
    w = World(name, world, budgets={r: ((hi - lo + 1) * fb * 16) // 15 + 16})       # room for one frame more than the shard
    _all_equal(w.call()[0], want)
    c = w.caches[r]
    assert c.capacity == hi - lo + 1 and len(c) == hi - lo
    k0 = next(iter(c._slots))
    xr, dr = c.assemble(w.ranks[r][0], [k0]), c.dino_rows(k0)
    c.store(["other-a", "other-b", "other-c"], torch.zeros(3 * xr.shape[0], xr.shape[1]), torch.zeros(3 * dr.shape[0], dr.shape[1]),
            [(1, 4)] * 3, pinned=set())
    assert c.stats()["evictions"] >= 2
    got, info = w.call()
    _all_equal(got, want)
    assert 0 < info[r]["frames_encoded"] < info[r]["frames"]
    assert all(i["frames_encoded"] == 0 for q, i in enumerate(info) if q != r)


@pytest.mark.parametrize("world", [4, 8])
def test_refinement_band_across_a_rank_boundary(world):
    name = "refine61"
    w = World(name, world)
    e, v, _, _ = w.ranks[0]
    band = set(seg.selection_band(e.sims_tensor(e.tower("dino", v), 61).tolist(), 24, e.selection_eps))
    ranges = seg.shard_ranges(61, world)
    assert any((h - 1) in band for (l, h) in ranges[:-1]), "the case must refine a pair across a rank boundary"
    want = w.serial()
    got, cold = w.call()
    _all_equal(got, want)
    assert sum(i["precise_frames_computed"] for i in cold) > 0
    got, warm = w.call(prompt=(7, 8))
    _all_equal(got, w.serial(prompt=(7, 8)))
    assert all(i["precise_frames_computed"] == 0 and i["pairs_computed"] == 0 for i in warm)
    # the left rank of a band boundary pair cleared, its right neighbour warm: the neighbour sends the precise rows again
    r = next(q for q, (l, h) in enumerate(ranges[:-1]) if (h - 1) in band)
    w.caches[r].clear()
    got, info = w.call()
    _all_equal(got, want)
    assert info[r]["precise_frames_computed"] > 0 and info[r + 1]["precise_frames_computed"] == 1


def test_sample_mismatch_raises_on_every_rank():
    world = 4
    w = World("plain61", world)
    _, v, a, c = w.ranks[0]
    for prompts in ([(1, 2)] * 3 + [(1, 3)], [(1, 2), (1, 2, 3), (1, 2), (1, 2)]):
        def fn(r, comm):
            return _rank_call(w.ranks[r][0], v, a, c, r, world, comm, w.caches[r], prompt=prompts[r])
        out, err = _run_world(world, fn, abort_on_error=False)
        assert sorted(err) == list(range(world)) and all(isinstance(x, ValueError) for x in err.values()), err
    # a cache made for other engine settings on one rank: refused on every rank
    other = CFake()
    other.dtype = torch.float16
    w.caches[2] = _new_cache(other)
    out, err = _run_world(world, lambda r, comm: _rank_call(w.ranks[r][0], v, a, c, r, world, comm, w.caches[r]),
                          abort_on_error=False)
    assert sorted(err) == list(range(world)) and all(isinstance(x, ValueError) for x in err.values()), err


def test_recompute_halo_with_cache_is_refused():
    e, v, a, c = _ccase("plain61")
    sh = ShardedVideoEncoder(e, 0, 2, comm=object())
    fp = sh.frame_plan(61, 4, c, halo=True)
    with pytest.raises(ValueError):
        sh.encode_video(v[fp["siglip_frames"]], v[fp["dino_frames"]], fp["T"], (384, 384), 6, [1, 2],
                        sample_indices=fp["sample_indices"], recompute_halo=True, cache=_new_cache(e))


def test_new_cache_delegates_to_the_engine():
    e = _ccase("plain61")[0]
    e.new_cache = lambda n: _new_cache(e, n)
    c = ShardedVideoEncoder(e, 0, 2, comm=object()).new_cache(12345)
    assert isinstance(c, FrameCache) and c.max_bytes == 12345 and c.signature == engine_signature(e)


# ------------------------------------------------------------------------------------------------ gloo processes
def _gloo_worker(rank, world, port, name, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        e, v, a, c = _ccase(name)
        cache = _new_cache(e)
        res = []
        for step, prompt in (("cold", (1, 2)), ("warm", (5, 6, 7)), ("other_cleared", (1, 2))):
            if step == "other_cleared" and rank != 0:
                cache.clear()
            info = {}
            out = _rank_call(e, v, a, c, rank, world, None, cache, prompt=prompt, info=info)
            res.append((step, out.numpy(), info["cache"]))
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", ["plain61", "audio61", "learned61", "refine61", "passthrough20"])
def test_world2_gloo_processes(name):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, name, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    e, v, a, c = _ccase(name)
    want = {"cold": _enc(e, v, a, c), "warm": _enc(e, v, a, c, prompt=(5, 6, 7))}
    want["other_cleared"] = want["cold"]
    for r in range(world):
        for step, out, info in res[r]:
            assert torch.equal(torch.from_numpy(out), want[step]), "rank %d, %s call differs" % (r, step)
            if step == "warm":
                assert info["frames_encoded"] == 0
            if step == "other_cleared":
                assert info["frames_encoded"] == (0 if r == 0 else info["frames"])


# ------------------------------------------------------------------------------------------------ boundary: config key
class CMixinEngine(_CacheMixin, MixinEngine):
    def new_cache(self, nbytes):
        return _new_cache(self, nbytes)


def _mixin_lm(**cfg):
    from test_host_logic import build_stub_lm, tiny_config
    torch.manual_seed(3)
    lm = build_stub_lm(tiny_config(hidden_size=8, context_token_num=3, tdc_frame_cap=37, tokenizer_model_max_length=10 ** 9, **cfg))
    lm.get_model()._tdc_encoder = CMixinEngine(K=3, H=8)
    return lm


def _mixin_run(lm, prompt):
    vid = make_video(90)
    ids = torch.tensor([[11, 12, -200, 13, 14, 15]])
    with torch.inference_mode():
        return lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [vid[None], vid[None]],
                                                       image_sizes=[(384, 384)], video_indices=[None], prompts=[list(prompt)],
                                                       audios=[None])


def test_config_key_validation_and_off_states():
    def m(**cfg):
        return _mixin_lm(**cfg).get_model()
    assert m().tdc_shard_cache() is None and m(tdc_shard_frames=True).tdc_shard_cache() is None         # absent: off
    assert m(tdc_shard_cache_bytes=0, tdc_shard_frames=True).tdc_shard_cache() is None
    assert m(tdc_shard_cache_bytes=BIG).tdc_shard_cache() is None                                          # not sharded
    for bad in (-1, 1.5, "1GB", True):
        with pytest.raises(ValueError):
            m(tdc_shard_cache_bytes=bad, tdc_shard_frames=True).tdc_shard_cache()
    mm = m(tdc_shard_cache_bytes=BIG, tdc_shard_frames=True)
    c = mm.tdc_shard_cache()
    assert isinstance(c, FrameCache) and c.max_bytes == BIG and mm.tdc_shard_cache() is c
    mm._tdc_encoder = CMixinEngine(K=3, H=8)                                                               # a new engine
    assert mm.tdc_shard_cache() is not c and len(mm.tdc_shard_cache()) == 0
    mm.tdc_shard_cache_clear()
    m().tdc_shard_cache_clear()                                                                            # off: a no-op
    # the serial cache keeps its contract under sharding
    assert m(tdc_video_cache_bytes=BIG, tdc_shard_cache_bytes=BIG, tdc_shard_frames=True).tdc_video_cache() is None


def _mixin_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lm = _mixin_lm(tdc_shard_frames=True, tdc_shard_cache_bytes=BIG)
        outs = [_mixin_run(lm, p) for p in ((1, 2), (3, 4, 5))]
        st = lm.get_model().tdc_shard_cache().stats()
        q.put((rank, [(o[4].numpy(), o[8]) for o in outs], st["frames_encoded"], st["frames"],
               lm.get_model()._tdc_encoder.tower_frames))
    finally:
        dist.destroy_process_group()


def test_mixin_shard_cache_world2_equals_serial():
    want = [_mixin_run(_mixin_lm(), p) for p in ((1, 2), (3, 4, 5))]
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mixin_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        outs, encoded, frames, tower_frames = res[r]
        for (emb, fs), w in zip(outs, want):
            assert torch.equal(torch.from_numpy(emb), w[4]), "rank %d differs" % r
            assert [tuple(x) for x in fs] == [tuple(x) for x in w[8]]
        assert encoded == frames and frames in (18, 19)          # 37 frames over 2 ranks, encoded once for two questions
        assert tower_frames == 2 * frames                        # one SigLIP and one DINOv2 pass over them, on the first call
