"""GPU (-m gpu): the frame cache of the frame-sharded path (dist.ShardedVideoEncoder.encode_video(cache=...),
config.tdc_shard_cache_bytes) at the full architecture (SigLIP-so400m + DINOv2-giant, H = 3584, K = 144, bf16 - the engine of
test_hip_dist_full), 16 frames per rank.  Every comparison is torch.equal against the uncached serial encode: cold, a second
question (no tower on any rank), and ranks whose caches hold different things (cleared, over budget).  World 2 runs as
processes on cuda:0 over gloo (nccl: one GPU per rank, skipped on a smaller box), world 4 and 8 as threads of one process."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROMPT_B = [101, 3000, 3001, 3002, 102]
PER_RANK = 16


def _call(enc, wav, T, rank, world, comm, cache, prompt, n_text=64, info=None, dino=None):
    from test_hip_dist_full import _video
    from tdc_video_amd.dist import ShardedVideoEncoder
    sh = ShardedVideoEncoder(enc, rank, world, comm=comm)
    fp = sh.frame_plan(T, budget_text_len=64, frame_cap=T)
    lo, hi = fp["lo"], fp["hi"]
    vd = _video(lo, hi, 378, 4321) if dino is None else dino(lo, hi, T)
    return sh.encode_video(_video(lo, hi, 384, 1234), vd, T, (384, 384), n_text, prompt,
                           audio={"audio_wav": wav} if wav is not None else None, sample_indices=fp["sample_indices"],
                           cache=cache, info=info)


def _serial(enc, wav, T, prompt, n_text=64, dino=None):
    from test_hip_dist_full import _video
    return enc.encode_video(_video(0, T, 384, 1234), _video(0, T, 378, 4321) if dino is None else dino(0, T, T), (384, 384),
                            budget_text_len=64, n_text_tokens=n_text, prompt_ids=prompt, frame_cap=T,
                            audio={"audio_wav": wav} if wav is not None else None)


@pytest.fixture(scope="module")
def engines():
    from test_hip_dist_full import _engine
    es = [_engine(8 * PER_RANK)[0] for _ in range(8)]
    yield es
    del es
    torch.cuda.empty_cache()


def _world(engines, world, T, caches, prompt, n_text=64, dino=None):
    from test_hip_dist2 import run_threads
    infos = [{} for _ in range(world)]
    out = run_threads(world, lambda r, comm: _call(engines[r], None, T, r, world, comm, caches[r], prompt, n_text, infos[r],
                                                   dino))
    return out, [i["cache"] for i in infos]


def _equal(outs, want):
    for r, o in enumerate(outs):
        assert o.shape == want.shape and torch.equal(o, want), "rank %d of %d differs" % (r, len(outs))


@pytest.mark.parametrize("world", [4, 8])
def test_threads_cold_second_question_asymmetric(engines, world):
    from test_hip_dist_full import PROMPT
    T = PER_RANK * world
    es = engines[:world]
    want_a, want_b = _serial(es[0], None, T, PROMPT), _serial(es[0], None, T, PROMPT_B, 40)
    caches = [e.new_cache(1 << 30) for e in es]
    got, info = _world(es, world, T, caches, PROMPT)                                    # cold
    _equal(got, want_a)
    assert all(i["frames_encoded"] == PER_RANK and not i["bypassed"] for i in info)
    got, info = _world(es, world, T, caches, PROMPT_B, 40)                               # a second question
    _equal(got, want_b)
    assert all(i["frames_encoded"] == 0 and i["frames_hit"] == PER_RANK and i["pairs_computed"] == 0 for i in info)
    for c in caches[1:]:                                                                 # rank 0 warm, the others cleared
        c.clear()
    got, info = _world(es, world, T, caches, PROMPT)
    _equal(got, want_a)
    assert info[0]["frames_encoded"] == 0 and all(i["frames_encoded"] == PER_RANK for i in info[1:])
    small = world // 2                                                                   # one rank over its budget
    caches[small] = es[small].new_cache(caches[0].frame_bytes * 4)
    for _ in range(2):
        got, info = _world(es, world, T, caches, PROMPT_B, 40)
        _equal(got, want_b)
        assert info[small]["bypassed"] and all(i["frames_encoded"] == 0 for r, i in enumerate(info) if r != small)
    del caches
    torch.cuda.empty_cache()


def test_threads_near_tied_refinement_across_a_boundary(engines):
    """the near-tied drift video of test_hip_dist_full at world 4 (32 frames per rank): the band holds a pair across a rank boundary; cold equals
    the serial encode, and the warm call runs no precise tower on any rank"""
    from test_hip_dist_full import PROMPT, _drift
    from tdc_video_amd import segment as seg
    world, T = 4, 128                          # the band of test_hip_dist_full's refinement case: a pair across a boundary
    es = engines[:world]
    saved = [e.selection_max_fraction for e in es]
    for e in es:
        e.selection_max_fraction = 1.0
    try:
        info = {}
        from test_hip_dist_full import _video
        want = es[0].encode_video(_video(0, T, 384, 1234), _drift(0, T, T), (384, 384), budget_text_len=64, n_text_tokens=64,
                                  prompt_ids=PROMPT, frame_cap=T, info=info)
        band = info["refined_pairs"]
        ranges = seg.shard_ranges(T, world)
        crossing = [r for r, (l, h) in enumerate(ranges[:-1]) if (h - 1) in band]
        print("band: %d pairs, across a rank boundary at ranks %s" % (len(band), crossing))
        assert band and crossing
        caches = [e.new_cache(1 << 30) for e in es]
        got, cold = _world(es, world, T, caches, PROMPT, dino=_drift)
        _equal(got, want)
        assert sum(i["precise_frames_computed"] for i in cold) > 0
        got, warm = _world(es, world, T, caches, PROMPT, dino=_drift)
        _equal(got, want)
        assert all(i["precise_frames_computed"] == 0 and i["frames_encoded"] == 0 for i in warm)
        caches[crossing[0]].clear()                             # the left rank of a boundary pair cold, its neighbour warm
        got, info = _world(es, world, T, caches, PROMPT, dino=_drift)
        _equal(got, want)
        assert info[crossing[0] + 1]["precise_frames_computed"] == 1
    finally:
        for e, s in zip(es, saved):
            e.selection_max_fraction = s
    del caches
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ processes
def _worker(rank, world, port, audio, q, backend):
    import torch.distributed as dist
    from test_hip_dist_full import PROMPT, _engine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev_index = rank if backend == "nccl" else 0
    torch.cuda.set_device(dev_index)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        T = PER_RANK * world
        enc, wav = _engine(T, audio, dev_index)
        cache = enc.new_cache(1 << 30)
        res = []
        for step, prompt, n_text in (("cold", PROMPT, 64), ("second", PROMPT_B, 40), ("other_cleared", PROMPT, 64)):
            if step == "other_cleared" and rank != 0:
                cache.clear()
            info = {}
            out = _call(enc, wav, T, rank, world, None, cache, prompt, n_text, info)
            ok = None
            if rank == 0:
                want = _serial(enc, wav, T, prompt, n_text)
                ok = bool(want.shape == out.shape and torch.equal(want, out))
            res.append((step, ok, out.float().sum().item(), info["cache"]))
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


def _n_gpus():
    try:
        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.parametrize("audio,backend", [(False, "gloo"), (True, "gloo"), (False, "nccl")])
def test_world2_processes(audio, backend):
    from test_hip_dist_full import _free_port
    world = 2
    if backend == "nccl" and _n_gpus() < world:
        pytest.skip("needs %d GPUs (RCCL: one GPU per rank)" % world)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, audio, q, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for j, (step, ok, s, info) in enumerate(res[0]):
        assert ok is True, "rank 0, %s call: sharded + cache != serial" % step
        assert res[1][j][2] == s, "rank 1 holds a different stream (%s)" % step
    for r in range(world):
        cold, second, cleared = (x[3] for x in res[r])
        assert cold["frames_encoded"] == PER_RANK and second["frames_encoded"] == 0
        assert cleared["frames_encoded"] == (0 if r == 0 else PER_RANK)
        if audio:
            assert cold["windows_encoded"] > 0 and second["windows_encoded"] == 0


def _mixin_worker(rank, world, port, q):
    try:
        _mixin_rank(rank, world, port, q)
    except BaseException as ex:          # noqa: BLE001 - reported by the parent instead of a wait on the queue
        q.put((rank, repr(ex), None, None, None))
        raise


def _mixin_rank(rank, world, port, q):
    import datetime
    import synth
    import torch.distributed as dist
    from test_hip_boundary import loaded_lm
    from test_hip_video_cache import _boundary_call
    from util import load_fixture
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    W, o = load_fixture("pipeline_T40.npz")
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    ids = torch.from_numpy(o["input_ids"])
    text = [j for j in range(ids.shape[1]) if int(ids[0, j]) != -200]
    ids2 = ids[:, [j for j in range(ids.shape[1]) if j not in text[-3:-1]]]          # a shorter question
    pid = [int(i) for i in o["prompt_ids"]]
    calls = ((ids, pid), (ids2, pid[:4] + pid[-1:]))
    want = None
    if rank == 0:
        off = loaded_lm(W, o)
        want = [_boundary_call(off, i, vid, o, p)[4].float().cpu().numpy() for i, p in calls]
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    try:
        lm = loaded_lm(W, o, tdc_shard_frames=True, tdc_shard_cache_bytes=1 << 30)
        got = [_boundary_call(lm, i, vid, o, p)[4].float().cpu().numpy() for i, p in calls]
        st = lm.get_model().tdc_shard_cache().stats()
        q.put((rank, got, want, st["frames_encoded"], st["frames"]))
    finally:
        dist.destroy_process_group()


def test_mixin_world2_shard_cache():
    """config.tdc_shard_frames + config.tdc_shard_cache_bytes: two gloo processes ask two questions about the 40-frame fixture
    video through the boundary; both return the serial inputs_embeds, and each rank encoded its frames once"""
    import numpy as np
    from test_hip_dist_full import _free_port
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mixin_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=300) for _ in range(world))}
    for p in procs:
        p.join(timeout=120)
    assert all(isinstance(res[r][0], list) for r in res), res
    assert all(p.exitcode == 0 for p in procs)
    want = res[0][1]
    for r in range(world):
        got, _, encoded, frames = res[r]
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), "rank %d differs" % r
        assert encoded == frames and 0 < frames <= 20             # every frame this rank stored was encoded once
