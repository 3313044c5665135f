"""GPU (-m gpu): the C-ABI calls preprocess_selected issues for every kind of frames input are pinned to a recorded fixture.
The bit-exactness tests of the test_hip_*_inputs.py files compare pixels; they would not notice a source that was read in
place being gathered into a copy first (or the reverse), a scratch query at another size, or the towers being run in another
order.  tests/golden/preprocess_trace.json holds the logs of the commit BEFORE preprocess_selected became one plan and one loop
(tests/golden/make_preprocess_trace.py wrote it there); it is not regenerated when the orchestration is reorganised.

A case is the log of every tdc_* call in order - its name, every integer argument that is no pointer and, of a struct passed
by reference, every integer field that is no pointer (strides, steps, bits, format, coefficients, sitings; a null reference
is logged as null) - plus the stats dict.  No pointer and no float is logged."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from test_hip_frame_inputs import frames_of, towers
from test_hip_interlaced_inputs import H0, IDX, W0, surfaces
from test_hip_orient_inputs import _Traced

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preprocess_trace.json")
T0 = 16
INTEGERS = (C.c_int, C.c_uint, C.c_long, C.c_ulong, C.c_longlong, C.c_ulonglong, C.c_size_t)
_SKIP = object()


def _struct_of(argtype):
    inner = getattr(argtype, "_type_", None)
    return inner if isinstance(inner, type) and issubclass(inner, C.Structure) else None


def _logged(arg, argtype):
    """what the log keeps of one argument: an integer, [struct name, its integer fields ...], None for a null reference, or
    _SKIP for a pointer or a float"""
    if argtype in INTEGERS:
        return int(arg)
    if _struct_of(argtype) is None:
        return _SKIP
    if arg is None:
        return None
    s = arg._obj                                   # the struct behind ctypes.byref
    assert isinstance(s, _struct_of(argtype)), (type(s), argtype)
    out = [type(s).__name__]
    for field, ftype in s._fields_:
        if ftype in INTEGERS:
            out.append(int(getattr(s, field)))
        elif issubclass(ftype, C.Array) and ftype._type_ in INTEGERS:
            out.append([int(v) for v in getattr(s, field)])
    return out


class _TracedArguments(_Traced):
    """_Traced with every non-pointer integer of every tdc_* call, by the signatures of tdc_video_amd.lib"""

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("tdc_"):
            return fn
        from tdc_video_amd import lib as L
        argtypes = L.SIGNATURES[name][1]

        def call(*a):
            assert len(a) == len(argtypes), name
            self._log.append([name] + [v for v in map(_logged, a, argtypes) if v is not _SKIP])
            return fn(*a)
        return call


def sources():
    """name -> build(device) -> 16 frames of 88 x 160: the seven surfaces of test_hip_interlaced_inputs, three with interpolated
    chroma (planar 4:2:0, which an Interlaced refuses, planar 4:2:2 from three planes, and packed) and an identity RgbFrames"""
    from tdc_video_amd import preprocess as pp
    f = frames_of(H0, W0).numpy()[:T0]
    y8 = np.ascontiguousarray(f[..., 1])
    u8, v8 = f[:, ::2, ::2, 0], f[:, ::2, ::2, 2]
    uv8 = np.ascontiguousarray(np.stack([u8, v8], -1).reshape(T0, H0 // 2, W0))
    u422, v422 = np.ascontiguousarray(f[:, :, ::2, 0]), np.ascontiguousarray(f[:, :, ::2, 2])
    uyvy = np.ascontiguousarray(np.stack([f[:, :, ::2, 0], y8[:, :, 0::2], f[:, :, ::2, 2], y8[:, :, 1::2]], -1).reshape(T0, H0, 2 * W0))

    def dev(a, device):
        t = torch.from_numpy(a)
        return t.cuda() if device == "cuda" else t

    out = {name: (lambda d, build=build: build(d)[:T0]) for name, (build, _, _) in surfaces().items()}
    out["nv12_linear"] = lambda d: pp.YuvFrames.nv12(dev(y8, d), dev(uv8, d), matrix="bt709", upsample="linear", siting="topleft")
    out["i422_linear"] = lambda d: pp.YuvFrames.i420(dev(y8, d), dev(u422, d), dev(v422, d), subsampling="422", full_range=True,
                                                     upsample="linear", siting="center")
    out["uyvy_linear"] = lambda d: pp.YuvFrames.uyvy(dev(uyvy, d), matrix="bt709", upsample="linear", siting="center")
    out["rgb_identity"] = lambda d: pp.RgbFrames(dev(f, d))
    return out


def wrappings():
    from tdc_video_amd import preprocess as pp
    return {"bare": lambda s: s,
            "interlaced": lambda s: pp.Interlaced(s, "bottom", "cubic"),
            "oriented": lambda s: pp.Oriented(s, 90, True),
            "oriented_interlaced": lambda s: pp.Oriented(pp.Interlaced(s), 270),
            "identity": lambda s: pp.Oriented(s, 0, False)}


SELECTIONS = {"idx10_slab4": (IDX, 4), "all_slab7": (None, 7)}


def run_cases():
    """"surface/device/wrapping/selection" -> {"log": ..., "stats": ...} as the checked-out tree produces them"""
    from tdc_video_amd import lib as L, preprocess as pp
    real = L.load()
    log, cases = [], {}
    L._lib = _TracedArguments(real, log)
    try:
        for name, build in sources().items():
            for device in ("host", "cuda"):
                for wrap, make in wrappings().items():
                    try:
                        src = make(build(device))
                    except ValueError:
                        assert "interlaced" in wrap        # only an Interlaced refuses a surface (linear chroma on 4:2:0)
                        continue
                    for sel, (idx, slab) in SELECTIONS.items():
                        del log[:]
                        stats = {}
                        pp.preprocess_selected(src, idx, towers(), torch.float16, slab, stats=stats)
                        cases["%s/%s/%s/%s" % (name, device, wrap, sel)] = {"log": list(log), "stats": stats}
        torch.cuda.synchronize()
    finally:
        L._lib = real
    return json.loads(json.dumps(cases))


def test_every_kind_issues_the_recorded_calls():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = run_cases()
    assert sorted(got) == sorted(want) and len(want) >= 200
    entries = {c[0] for case in want.values() for c in case["log"]}
    assert {"tdc_yuv_linear_to_rgb", "tdc_yuv_packed_linear_to_rgb", "tdc_pack_rgb", "tdc_field_to_frame", "tdc_orient_frames",
            "tdc_yuv420_to_rgb", "tdc_yuv_hdr_to_rgb", "tdc_yuv_packed_to_rgb", "tdc_preprocess_scratch_bytes"} <= entries
    differing = [k for k in sorted(want) if got[k] != want[k]]
    for k in differing[:3]:
        print(k, "\n  got ", got[k], "\n  want", want[k])
    assert not differing, "%d of %d cases differ from the recorded calls: %s" % (len(differing), len(want), differing[:8])
