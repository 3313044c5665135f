"""bench.py as the driver starts it.  `python bench.py --gpus N` (N > 1, no RANK in the environment) must start its own N ranks
(one per GPU, the reference's launch convention: /root/reference/eval/eval_mlvu.py:129-157), print rank 0's ONE JSON line and
return the worst child's code; under torch.distributed.run it must keep working as a rank."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_self_launch_propagates_a_failing_rank_without_hanging():
    """No GPU here: every child dies at torch.cuda.set_device - the launcher must come back with a non-zero code, print no
    JSON line, and never touch the GPU itself (it would raise in this process otherwise)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--frames", "8", "--steps", "1",
                        "--warmup", "0", "--no-cpu-baseline"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "stopping the other ranks" in r.stderr or "exited with code" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_world_size_mismatch_is_an_error_message_not_an_assert():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--no-cpu-baseline"],
                       env=_env(RANK="0", WORLD_SIZE="2", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr and "Traceback" not in r.stderr


_EMITTED = {}


@pytest.mark.gpu
@pytest.mark.parametrize("via_mixin", [False, True])
def test_plain_python_bench_gpus2_on_one_gpu(via_mixin):
    """The exact command of the driver's scaling run, two ranks sharing cuda:0 over gloo (TDC_BENCH_ONE_GPU / TDC_DIST_BACKEND
    are the test hooks of bench.py): one JSON line with the per-rank times.  via_mixin: the same through the drop-in boundary -
    every rank calls prepare_inputs_labels_for_multimodal with the whole video and config.tdc_shard_frames splits its frames
    over the ranks (model.py -> dist.ShardedVideoEncoder); the emitted stream has the same length either way."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--frames", "64", "--steps", "1",
                        "--warmup", "1", "--full"] + (["--via-mixin"] if via_mixin else []),
                       env=_env(TDC_BENCH_ONE_GPU="1", TDC_DIST_BACKEND="gloo"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 1 and res["value"] > 0
    rk = res["rank_ms_per_step"]
    assert len(rk["per_rank"]) == 2 and rk["max"] >= rk["min"] > 0
    assert res["roofline"]["frac"] > 0 and res["config"]["frames"] == 64
    assert res["ranks_seen"] == [0, 1] and res["rank_devices"] == [0, 0] and res["dist_backend"] == "gloo"
    assert res["config"]["entry"].startswith("mixin" if via_mixin else "engine")
    assert res["config"]["product_setting"]["tdc_frame_cap"] == 64
    _EMITTED[via_mixin] = res["config"]["emitted_tokens"]
    if len(_EMITTED) == 2:
        assert _EMITTED[False] == _EMITTED[True] > 64 * 17


def test_launch_guard_stops_a_rank_that_never_finishes():
    """One rank finishes, the other sleeps for ever (a peer stuck in a collective): the launcher must come back within its
    wall-clock guard with code 124, having stopped the sleeper - not hold the caller's lease."""
    import time
    sys.path.insert(0, ROOT)
    import bench
    child = [sys.executable, "-c", "import os, time\nif os.environ['RANK'] == '1':\n    time.sleep(10 ** 6)\n"]
    t0 = time.monotonic()
    rc = bench.self_launch(2, guard_s=3.0, cmd=child)
    dt = time.monotonic() - t0
    assert rc == 124
    assert dt < 40, dt


def test_launch_without_stragglers_is_unaffected_by_the_guard():
    sys.path.insert(0, ROOT)
    import bench
    ok = [sys.executable, "-c", "import os; assert os.environ['WORLD_SIZE'] == '2' and os.environ['MASTER_ADDR'] == '127.0.0.1'"]
    assert bench.self_launch(2, guard_s=60.0, cmd=ok) == 0
    bad = [sys.executable, "-c", "import os, sys, time\nif os.environ['RANK'] == '0':\n    sys.exit(7)\ntime.sleep(10 ** 6)\n"]
    assert bench.self_launch(2, guard_s=60.0, cmd=bad) == 7


def test_rank_guard_ends_a_stuck_rank_with_124():
    code = ("import sys, time; sys.path.insert(0, %r); import bench; bench.rank_guard(1.0); time.sleep(60)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 124 and "rank-timeout" in r.stderr


def test_steps_below_one_is_an_error_message():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--no-cpu-baseline"], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr and "Traceback" not in r.stderr


def test_profiled_step_outputs_need_full():
    """What reports on --full's profiled step is an argument error in a plain run, not a silently missing file."""
    for extra in (["--dump-gemm-shapes", "shapes.txt"], ["--gemm-shape-times", "times.txt"], ["--pmc-out", "pmc.json"],
                  ["--pmc", "on"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=_env(), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 2 and "--full" in r.stderr and "Traceback" not in r.stderr, (extra, r.stderr[-500:])


def test_dump_outputs_writes_the_whole_output_or_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 tokens.npy, the whole array when it fits DUMP_BYTES, otherwise every row at a seeded choice of
    columns (or, when too few columns fit, a seeded choice of rows at DUMP_MIN_COLS columns) - the same choice on every call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    small = torch.randn(10, 64, generator=g).half()
    got = np.load(bench.dump_outputs(small, str(tmp_path / "small")))
    assert got.dtype == np.float32 and np.array_equal(got, small.float().numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    for n, H, shape in ((300, 512, (300, 54)), (4096, 512, (1024, 16))):
        out = torch.randn(n, H, generator=g).half()
        a = np.load(bench.dump_outputs(out, str(tmp_path / ("a%d" % n))))
        b = np.load(bench.dump_outputs(out, str(tmp_path / ("b%d" % n))))
        assert a.dtype == np.float32 and a.shape == shape and a.nbytes <= bench.DUMP_BYTES and np.array_equal(a, b)
        full = out.float().numpy()
        if shape[0] == n:           # every row: each dumped column is a column of the output
            for j in range(a.shape[1]):
                assert any(np.array_equal(a[:, j], full[:, k]) for k in range(H))
        else:
            assert np.isin(a, full).all()


@pytest.mark.gpu
def test_bench_dump_outputs_and_steps(tmp_path):
    """bench.py --steps K times K steps and writes the last one's emitted tokens: one row per emitted token, float32."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", "64", "--steps", "2",
                        "--warmup", "1", "--no-cpu-baseline", "--pmc", "off", "--dump-outputs", str(tmp_path)],
                       env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    a = np.load(str(tmp_path / "tokens.npy"))
    assert a.dtype == np.float32 and a.shape[0] == res["config"]["emitted_tokens"] and 0 < a.shape[1] <= res["config"]["hidden"]
    assert np.isfinite(a).all() and a.nbytes <= 64 << 20


@pytest.mark.gpu
def test_bench_full_adds_the_roofline_and_leaves_the_steps_alone(tmp_path):
    """A plain run measures the headline alone; --full adds `roofline` from one extra profiled step after the timed ones, and
    the timed steps compute the same tokens either way."""
    import numpy as np
    got = {}
    for full in (False, True):
        d = tmp_path / ("full" if full else "plain")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", "64", "--steps", "1",
                            "--warmup", "1", "--dump-outputs", str(d)] + (["--full", "--no-cpu-baseline", "--pmc", "off"] if full else []),
                           env=_env(), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        got[full] = json.loads(lines[0]), np.load(str(d / "tokens.npy"))
    plain, full = got[False][0], got[True][0]
    assert "roofline" not in plain and "cpu_baseline" not in plain
    assert full["roofline"]["frac"] > 0 and full["roofline"]["launches"] > 0 and "cpu_baseline" not in full
    assert plain["config"] == full["config"] and np.array_equal(got[False][1], got[True][1])


@pytest.mark.gpu
def test_torchrun_form_of_the_drivers_scaling_run_on_one_gpu():
    """The driver's N > 1 command line - python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ... - with both ranks on cuda:0 over gloo (the bench's test hooks): bench.py must run as a
    rank (not launch ranks of its own), print ONE JSON line on rank 0 and leave the process group cleanly."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--frames", "64",
                        "--steps", "1", "--warmup", "1", "--no-cpu-baseline"],
                       env=_env(TDC_BENCH_ONE_GPU="1", TDC_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["ranks_seen"] == [0, 1] and res["value"] > 0 and res["scaling"] == "strong"
