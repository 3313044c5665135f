"""CPU: the launch sequences of the three C++ composites (csrc/api.cpp: tdc_vit_fwd, tdc_qformer_fwd, tdc_connector_fwd) are
pinned to a recorded fixture.  api.cpp holds no kernel, so a host compiler builds it; tests/api_trace/api_trace.cpp supplies
every library entry point it calls as a stub that prints the call - name, every non-zero descriptor field, workspace
pointers as offsets - and runs the composites over a matrix of tiny models (both residual streams x plain / LayerNorm-fold /
fp8 levels 1-3, the refusals, the Q-Former's three cross-attention forms with and without the prompt table, the connector).
The GPU suites compare the composites' RESULTS with the per-kernel Python sequence; this one sees every operand of every
launch, in order, without a GPU.  tests/golden/api_trace.txt holds the trace of the commit that introduced this test
(tests/golden/make_api_trace.py wrote it); it is not regenerated when api.cpp is reorganised."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "api_trace.txt")
SOURCES = [os.path.join(ROOT, "tdc-video_amd", "csrc", "api.cpp"), os.path.join(HERE, "api_trace", "api_trace.cpp")]


def _toolchain():
    """-> (host compiler or None, ROCm include directory or None)"""
    cxx = shutil.which(os.environ.get("CXX") or "g++")
    inc = os.path.join(os.environ.get("ROCM_PATH") or "/opt/rocm", "include")
    return cxx, inc if os.path.isdir(inc) else None


def run_trace(workdir):
    """builds the trace program in `workdir` (plain host compile: no HIP compiler, no HIP runtime library) and returns its stdout"""
    cxx, inc = _toolchain()
    assert cxx, "no host C++ compiler ($CXX, else g++)"
    assert inc, "no ROCm headers (hip/hip_runtime.h declares the one runtime call api.cpp makes)"
    exe = os.path.join(str(workdir), "api_trace")
    r = subprocess.run([cxx, "-std=c++17", "-O0", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-o", exe] + SOURCES,
                       capture_output=True, text=True)
    assert r.returncode == 0, "the trace program did not build:\n" + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, timeout=60)
    assert r.returncode == 0, "the trace program failed (%d):\n%s" % (r.returncode, r.stderr.decode()[-2000:])
    return r.stdout


def test_composites_launch_what_the_fixture_records(tmp_path):
    if _toolchain() == (None, None):
        pytest.skip("neither a host C++ compiler nor the ROCm headers")
    got = run_trace(tmp_path)
    with open(GOLDEN, "rb") as f:
        want = f.read()
    if got != want:
        g, w = got.decode().splitlines(), want.decode().splitlines()
        i = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        case = next((l for l in reversed(w[:i + 1]) if l.startswith("== ")), "?")
        pytest.fail("trace differs from tests/golden/api_trace.txt at line %d (%s)\n  want: %s\n  got:  %s" % (
            i + 1, case, w[i] if i < len(w) else "<end>", g[i] if i < len(g) else "<end>"))
