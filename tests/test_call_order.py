"""CPU: the ORDER in which the encode orchestration calls the engine (and, sharded, the transport) is pinned to a recorded
fixture.  The other CPU suites compare results; their engine doubles are pure functions, so they would not notice the SigLIP
tower being enqueued after the host read of the a5 similarities instead of before it - the order that keeps the device busy
while the host ranks them.  tests/golden/call_order.json holds the logs of the commit that introduced this test
(tests/golden/make_call_order.py wrote it); it is not regenerated when the orchestration is reorganised."""
import json
import os

import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
from tdc_video_amd import pipeline
from tdc_video_amd.cache import FrameCache, engine_signature
from test_dist_gloo import FakeEngine, MixinEngine, NoisyEngine, make_video
from test_multi_prompt import MultiEngine
from test_shard_cache import _rank_call, _run_world
from test_video_cache import CFake, _CacheMixin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_order.json")
RECORDED = ("tower", "sims_tensor", "mark", "fetch", "slot_sims", "pair_sims", "precise_dino", "fingerprint", "connector",
            "local_audio", "with_audio", "make_queries", "learned_queries", "compress_frames", "emit")
FRAME_BYTES = (5 * 8 + 4 * 8) * 4            # one cached frame of the doubles: X [5, 8] + DINOv2 [4, 8], fp32
SIZE = (384, 384)


class _OnDevice(torch.Tensor):
    """a host tensor that says it lives on the device: the orchestration then reads it through mark() / fetch(), as it does
    on the GPU, and the read shows up in the log"""
    is_cuda = True


def _describe(a):
    """tower names as they are, tensors and arrays by shape, lists / dicts by length, callables and events by kind"""
    if a is None or isinstance(a, (str, bool, int, float)):
        return a
    if torch.is_tensor(a) or isinstance(a, np.ndarray):
        return list(a.shape)
    if isinstance(a, (list, tuple, dict, set)):
        return {"len": len(a)}
    return "callable" if callable(a) else type(a).__name__


def record(eng, log, names=RECORDED):
    """the recording proxy: every engine-protocol method of `eng` among `names` logs (name, arguments, keyword arguments)
    before it runs; mark / fetch are supplied (the doubles have none) and sims_tensor's result counts as a device tensor"""
    eng.mark = lambda: "event"
    eng.fetch = lambda t, ev: t.tolist()
    for name in names:
        fn = getattr(eng, name, None)
        if fn is None:
            continue

        def spy(*a, _fn=fn, _name=name, **kw):
            log.append([_name, [_describe(x) for x in a], {k: _describe(v) for k, v in sorted(kw.items())}])
            out = _fn(*a, **kw)
            return out.as_subclass(_OnDevice) if _name == "sims_tensor" else out
        setattr(eng, name, spy)
    return eng


class RecordingComm:
    """a transport that logs this rank's collectives and point-to-point operations into the rank's engine log"""

    def __init__(self, comm, log):
        self.comm, self.log, self.rank, self.world = comm, log, comm.rank, comm.world

    def all_gather(self, t):
        self.log.append(["comm.all_gather", list(t.shape)])
        return self.comm.all_gather(t)

    def all_gather_into(self, out, t):
        self.log.append(["comm.all_gather_into", list(out.shape), list(t.shape)])
        return self.comm.all_gather_into(out, t)

    def exchange(self, sends, recvs):
        self.log.append(["comm.exchange", [[list(t.shape), d] for t, d in sends], [[list(b.shape), s] for b, s in recvs]])
        return self.comm.exchange(sends, recvs)


class CMulti(_CacheMixin, MultiEngine):
    pass


def _serial(eng, T, **kw):
    log = []
    vid = make_video(T)
    pipeline.encode_video_with(record(eng, log), vid, vid, SIZE, budget_text_len=4, n_text_tokens=6, prompt_ids=[1, 2], **kw)
    return log


def _cached():
    out = {}
    vid = make_video(30)
    for name, nbytes in (("", 1 << 30), ("_bypass", 2 * FRAME_BYTES)):
        log = []
        eng = record(CFake(N=5), log)
        cache = FrameCache(nbytes, engine_signature(eng))
        for state in ("cold", "warm"):
            info = {}
            pipeline.encode_video_cached(eng, cache, vid, vid, SIZE, 4, 6, [1, 2], info=info)
            assert info["cache"]["bypassed"] == bool(name)
            if not name:
                assert info["cache"]["frames_encoded"] == (30 if state == "cold" else 0)
            out["cached_T30_" + state + name] = list(log)
            del log[:]
            if name:
                break
    return out


def _batch():
    log = []
    eng = record(MixinEngine(K=3, H=8), log)

    def sample(v, **kw):
        return dict(px_siglip=v, px_dino=v + 0.5, image_size=SIZE, budget_text_len=4, n_text_tokens=4, prompt_ids=[1, 2],
                    audio=None, video_index=None, splice=None, **kw)
    pipeline.encode_batch_with(eng, [sample(make_video(1), image=True), sample(make_video(8)), sample(make_video(30) + 1.0)],
                               224, None)
    return log


def _prompts(cache):
    log = []
    eng = record(CMulti(K=3, H=8, N=5, max_len=16 + 4 + 20 * 33), log)
    vid = make_video(40)
    # the first two share the a1 selection (33 of 40 frames); the third's text is long enough to leave fewer frames
    prompts = [dict(budget_text_len=4, n_text_tokens=6, prompt_ids=[1, 2]),
               dict(budget_text_len=4, n_text_tokens=7, prompt_ids=[3, 4, 5]),
               dict(budget_text_len=44, n_text_tokens=8, prompt_ids=[6])]
    infos = [{} for _ in prompts]
    c = FrameCache(1 << 30, engine_signature(eng)) if cache else None
    pipeline.encode_video_prompts_with(eng, vid, vid, SIZE, prompts, None, 224, None, infos, c, 8, 1.0)
    assert [len(i["frame_indices"]) for i in infos] == [33, 33, 31]
    assert [i["prompts"]["group_size"] for i in infos] == [2, 2, 1]
    return log


def _sharded(cached, budgets=None, calls=1):
    world = 2
    vid = make_video(30)
    logs = [[] for _ in range(world)]
    engs = [record(CFake(N=5), logs[r]) for r in range(world)]
    caches = [FrameCache((budgets or {}).get(r, 1 << 30), engine_signature(engs[r])) if cached else None for r in range(world)]
    out = []
    for _ in range(calls):
        for lg in logs:
            del lg[:]
        infos = [{} for _ in range(world)]
        _, err = _run_world(world, lambda r, comm: _rank_call(engs[r], vid, None, 10 ** 6, r, world,
                                                              RecordingComm(comm, logs[r]), caches[r], info=infos[r]))
        if err:
            raise next(iter(err.values()))
        if budgets:
            assert [bool(i["cache"]["bypassed"]) for i in infos] == [r in budgets for r in range(world)]
        out.append({"rank%d" % r: list(lg) for r, lg in enumerate(logs)})
    return out


def run_cases():
    """-> {case: call log}; the cases are the smallest at which each branch of the orchestration exists (max_num_segments is
    24, so a5 segments from T = 26)"""
    out = {}
    out["serial_T8_passthrough"] = _serial(FakeEngine(N=5), 8)
    out["serial_T30_segmented"] = _serial(FakeEngine(N=5), 30)
    info = {}
    out["serial_T30_refined"] = _serial(NoisyEngine(N=5), 30, info=info)
    assert info["refined_pairs"], "the case must refine a band"
    info = {}
    out["serial_T40_a1_drops_frames"] = _serial(FakeEngine(N=5, max_len=16 + 4 + 20 * 33), 40, info=info)
    assert len(info["frame_indices"]) == 33
    out.update(_cached())
    out["batch_image_T8_T30"] = _batch()
    out["prompts_3"] = _prompts(False)
    out["prompts_3_cached"] = _prompts(True)
    out["sharded2_T30"] = _sharded(False)[0]
    cold, warm = _sharded(True, calls=2)
    out["sharded2_T30_cached_cold"], out["sharded2_T30_cached_warm"] = cold, warm
    out["sharded2_T30_cached_rank1_bypasses"] = _sharded(True, budgets={1: 2 * FRAME_BYTES})[0]
    return json.loads(json.dumps(out))          # tuples -> lists, as the fixture holds them


@pytest.fixture(scope="module")
def logs():
    return run_cases()


with open(GOLDEN) as _f:
    WANT = json.load(_f)


def test_the_fixture_holds_every_case(logs):
    assert sorted(logs) == sorted(WANT)


def assert_same_log(case, got, want):
    """one case's log against the fixture's (a dict: one log per rank), naming the first call that differs"""
    if isinstance(want, dict):
        assert sorted(got) == sorted(want)
        for rank in sorted(want):
            assert got[rank] == want[rank], "%s %s: first difference at call %d" % (
                case, rank, next((i for i, (a, b) in enumerate(zip(got[rank], want[rank])) if a != b),
                                 min(len(got[rank]), len(want[rank]))))
    else:
        assert got == want, "%s: first difference at call %d" % (
            case, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))))


@pytest.mark.parametrize("case", sorted(WANT))
def test_call_order(logs, case):
    assert_same_log(case, logs[case], WANT[case])


def test_siglip_is_enqueued_before_the_host_read(logs):
    """what the fixture is for, said once in words: between sims_tensor and the fetch of its result lie mark() and the SigLIP
    tower"""
    names = [c[0] if c[0] != "tower" else "tower:" + c[1][0] for c in logs["serial_T30_segmented"]]
    i = names.index("sims_tensor")
    assert names[i:i + 4] == ["sims_tensor", "mark", "tower:siglip", "fetch"]
