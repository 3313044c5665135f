"""GPU (-m gpu): encode from interlaced video.  tdc_field_to_frame against the numpy restatement of
the field rebuild (interlace_cases) - the shapes where clamping, runs and blocks can go wrong, every column form, its memory
contract, designed values, offsets past 2^32 and its refusals - and the frames funnel on the tiny fixture engine of
test_hip_frame_inputs: everything behind the rebuild is the frames path that exists, so every comparison is bit for bit
against the same call on the frames a host rebuilt beforehand with the restatement.

The forms.  A thread owns a column of 16 bytes when src, both strides, dst and 3 W are multiples of 16, of 4 bytes when they
are multiples of 4, one byte otherwise, and walks RUN = 16 field rows (interlace_cases.RUN; a workgroup is THREADS = 256
columns, so a row of the widest form spans more than one workgroup above 4096 bytes).  Of SHAPES (4, 16), (9, 80), (3, 1376)
and (31, 16) can take the 16-byte form and (3, 4), (17, 4) and (37, 92) the 4-byte form, at pointer offset 0 of src and of dst;
every other offset and shape takes bytes.  Hf = 17 is RUN + 1 (a second run of one row), Hf = 31 is 2 RUN - 1 (a ragged second run)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import interlace_cases as ic
import memcheck
import test_hip_memory_contract as contract
from test_hip_frame_inputs import R, _call, _same, frames_of, fx, reference_pixels, towers  # noqa: F401  (fx: the engine fixture)
from test_hip_boundary import loaded_lm
from test_hip_orient_inputs import _Traced, rgb_of
import orient_cases as oc

pytestmark = pytest.mark.gpu

assert ic.RUN == 16 and ic.THREADS * ic.WIDEST == 4096
SHAPES = [(1, 1),                                   # every tap clamps to one row
          (2, 1), (2, 7), (3, 4),                   # fewer rows than the cubic window; (3, 4): 12 bytes per row, the 4-byte form
          (4, 16), (9, 80),                         # 3 W a multiple of 16
          (5, 17), (37, 91),                        # odd everything; three runs
          (17, 4), (37, 92),                        # the 4-byte form (12 and 276 bytes per row) over a second run of one row and over three runs, the last ragged
          (3, 1376),                                # 4128 bytes per row: two workgroups of the widest form
          (ic.RUN + 1, 6), (2 * ic.RUN - 1, 16)]    # 17 and 31 field rows
PF = [(p, f) for p in (0, 1) for f in ic.FILLS]


def restated(F, parity, fill):
    return torch.from_numpy(ic.rebuild(F, parity, fill))


def pitch_pad(W):
    """pitch padding that keeps the form a dense row would take: 16, 4 or 5 bytes"""
    return 16 if 3 * W % 16 == 0 else (4 if 3 * W % 4 == 0 else 5)


def field_source(F, kind, parity, pattern):
    """the field picture F [T, Hf, W, 3] laid out in host memory as `kind` -> (the bytes, the offset of field pixel (0, 0, 0),
    frame_stride, row_stride).  "dense": F as it is.  "interleaved": the field of frames [T, 2 Hf, pitch] on rows parity,
    parity + 2, ...; the other field's rows and the pitch padding hold `pattern`."""
    T, Hf, W, _ = F.shape
    if kind == "dense":
        return F.reshape(-1).copy(), 0, Hf * W * 3, W * 3
    pitch = 3 * W + pitch_pad(W)
    buf = np.full((T, 2 * Hf, pitch), pattern, np.uint8)
    buf[:, parity::2, :3 * W] = F.reshape(T, Hf, 3 * W)
    return buf.reshape(-1), parity * pitch, 2 * Hf * pitch, 2 * pitch


# ---------------------------------------------------------------------------------------------------- the kernel
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  tdc_field_to_frame's is the function below: it is
# entered there under its own name (not a test_ name: that module collects nothing new).
@contract.covers("tdc_field_to_frame")
def field_to_frame_memory_contract(T, Hf, W, offsets=range(4)):
    """tdc_field_to_frame for both parities and both fills, from src / dst pointers 0 .. 3 bytes into a larger allocation
    (every column form), src dense and as the field of an interleaved pitched frame: dst in a guarded arena - nothing outside
    its 6 T Hf W bytes changes; src between poisoned bytes, the other field's rows and the pitch padding included, holding
    0x00, then 0xFF - the output is the restatement's either way."""
    from tdc_video_amd import ops
    F = ic.random_fields(T, Hf, W)
    nd = 2 * F.size
    want = {pf: restated(F, *pf).cuda() for pf in PF}
    for pattern in memcheck.PATTERNS:
        for kind in ("dense", "interleaved"):
            for parity in (0, 1):
                data, at, fs, rs = field_source(F, kind, parity, pattern)
                flat, n = torch.from_numpy(data).cuda(), data.size
                for so in offsets:
                    held, _ = memcheck.poisoned(flat, 64, 64, fill=pattern, rows=torch.arange(so, so + n), total_rows=n + 3)
                    src = held[so + at:].as_strided((T, Hf, W, 3), (fs, rs, 3, 1))
                    assert src.data_ptr() % 4 == (so + at) % 4 and held.data_ptr() % 16 == 0
                    for do in offsets:
                        room, arena = memcheck.guarded((nd + 3,), torch.uint8, "cuda", 64, 64, fill=pattern)
                        written = torch.zeros(nd + 3, dtype=torch.bool)
                        written[do:do + nd] = True
                        for fill in ic.FILLS:
                            arena.buf.fill_(pattern)
                            dst = room[do:do + nd].view(T, 2 * Hf, W, 3)
                            assert dst.data_ptr() % 16 == do
                            ops.field_to_frame(src, parity, fill, out=dst)
                            torch.cuda.synchronize()
                            memcheck.assert_untouched(arena, written)
                            assert torch.equal(dst, want[parity, fill]), (T, Hf, W, kind, parity, fill, so, do, pattern)


contract.field_to_frame_memory_contract = field_to_frame_memory_contract


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("Hf,W", SHAPES)
def test_both_parities_and_fills_every_form_inside_guards_and_poison(Hf, W, T):
    field_to_frame_memory_contract(T, Hf, W)


def test_ops_allocates_the_frame_and_takes_codes_or_names():
    from tdc_video_amd import ops
    F = ic.random_fields(2, 9, 80)
    src = torch.from_numpy(F).cuda()
    for p, f in PF:
        got = ops.field_to_frame(src, p, f)
        assert tuple(got.shape) == (2, 18, 80, 3) and torch.equal(got.cpu(), restated(F, p, f))
        assert torch.equal(ops.field_to_frame(src, p, ic.FILLS.index(f)), got)
    # a device-resident interleaved video read where it lies: no copy of the field in front
    frames = torch.from_numpy(ic.weave(F, ic.random_fields(2, 9, 80, seed=5), "interleaved")).cuda()
    assert torch.equal(ops.field_to_frame(frames[:, 0::2], 0, "cubic").cpu(), restated(F, 0, "cubic"))
    assert torch.equal(ops.field_to_frame(frames[1:, 0::2], 0, "cubic").cpu(), restated(F[1:], 0, "cubic"))      # one frame


def widened(F, W):
    """F [T, Hf, w, 3] with zero columns appended up to W pixels: the rebuild is per byte column, so the forms differ only in
    which thread makes a byte"""
    out = np.zeros(F.shape[:2] + (W, 3), np.uint8)
    out[:, :, :F.shape[2]] = F
    return out


def test_designed_values():
    from tdc_video_amd import ops
    alt = ic.alternating()
    for p, f in PF:
        got = ops.field_to_frame(torch.from_numpy(alt).cuda(), p, f).cpu()
        assert torch.equal(got, restated(alt, p, f)), (p, f)
        if f == "cubic":                                          # clips at both ends
            made = got[:, 1 - p::2]
            assert int(made.min()) == 0 and int(made.max()) == 255
        for v in (0, 1, 128, 255):                                # a constant picture stays constant
            c = ic.constant(v, 2, 5, 16)
            assert torch.equal(ops.field_to_frame(torch.from_numpy(c).cuda(), p, f).cpu(), torch.full((2, 10, 16, 3), v, dtype=torch.uint8))
    # every (a, b) pair and every pair of cubic sums, in the byte form (the frames' own widths) and in the 16-byte form
    lin, cub = ic.linear_pairs(), ic.cubic_pairs()
    for F, f, W16 in ((lin, "linear", 21856), (cub, "cubic", 21776)):
        assert 3 * F.shape[2] % 4 != 0 and 3 * W16 % 16 == 0
        for G in (F, widened(F, W16)):
            assert torch.equal(ops.field_to_frame(torch.from_numpy(G).cuda(), 0, f).cpu(), restated(G, 0, f)), (f, G.shape)
    wide4 = widened(cub, 21764)                                   # 65292 bytes per row: the 4-byte form
    assert 3 * 21764 % 16 == 12
    assert torch.equal(ops.field_to_frame(torch.from_numpy(wide4).cuda(), 0, "cubic").cpu(), restated(wide4, 0, "cubic"))


def torch_rebuild(F, parity, cubic):
    """the restatement on the device for one frame [Hf, W, 3] (int16 sums: at most 4598), for the one case too large for numpy"""
    Hf = F.shape[0]
    m = torch.arange(Hf, device=F.device) - parity

    def rows(i):
        return F[i.clamp(0, Hf - 1)].to(torch.int16)

    if cubic:
        made = ((9 * (rows(m) + rows(m + 1)) - rows(m - 1) - rows(m + 2) + 8) >> 4).clamp(0, 255)
    else:
        made = (rows(m) + rows(m + 1) + 1) >> 1
    out = torch.empty((2 * Hf,) + tuple(F.shape[1:]), dtype=torch.uint8, device=F.device)
    out[parity::2] = F
    out[1 - parity::2] = made.to(torch.uint8)
    return out


def test_offsets_past_2_to_the_32():
    """T = 41 fields of 3000 x 6000: 2.2 GB in, 4.43 GB out - the last frame starts 4.32 GB into dst"""
    from tdc_video_amd import ops
    small = ic.random_fields(1, 7, 5)
    for p, f in PF:                                               # the device restatement is the numpy one
        assert torch.equal(torch_rebuild(torch.from_numpy(small[0]).cuda(), p, f == "cubic").cpu(), restated(small, p, f)[0])
    T, Hf, W = 41, 3000, 6000
    assert (T - 1) * 6 * Hf * W > 1 << 32
    src = torch.empty((T, Hf, W, 3), dtype=torch.uint8, device="cuda").random_(0, 256)
    out = torch.empty((T, 2 * Hf, W, 3), dtype=torch.uint8, device="cuda")
    ops.field_to_frame(src, 1, "cubic", out=out)
    for t in (0, T - 1):
        assert torch.equal(out[t], torch_rebuild(src[t], 1, True)), t
    del src, out
    torch.cuda.empty_cache()


def test_badarg_before_any_launch():
    from tdc_video_amd import lib as L
    lib = L.load()
    T, Hf, W = 2, 4, 6
    n = T * Hf * W * 3
    F = ic.random_fields(T, Hf, W)
    both = torch.from_numpy(np.concatenate([F.reshape(-1)] * 3)).cuda()      # the dense src, then 2 n more bytes
    out, arena = memcheck.guarded((2 * n,), torch.uint8, "cuda", 64, 64)
    sp = both.data_ptr()

    def rc(src=sp, fs=Hf * W * 3, rs=W * 3, dims=(T, Hf, W), parity=0, fill=1, dst=out.data_ptr()):
        return lib.tdc_field_to_frame(C.c_void_p(src), fs, rs, *dims, parity, fill, C.c_void_p(dst),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [rc(src=0), rc(dst=0)]
    for i, over in enumerate((65536, 32768, 65536)):
        for v in (0, -1, over):
            dims = [T, Hf, W]
            dims[i] = v
            bad.append(rc(dims=tuple(dims), fs=1 << 30, rs=1 << 20))
    bad += [rc(parity=-1), rc(parity=2), rc(fill=-1), rc(fill=2)]
    bad += [rc(fs=-1), rc(rs=-1), rc(fs=(1 << 40) + 1), rc(fs=(1 << 40) + 1, rs=(1 << 40) + 1)]
    bad += [rc(dims=(1, 1, W), fs=W * 3, rs=(1 << 40) + 1)]       # one row of one frame: every other check passes, the row_stride bound alone refuses
    bad += [rc(rs=W * 3 - 1), rc(fs=Hf * W * 3 - 1), rc(rs=2 * W * 3, fs=Hf * W * 3)]      # rows, then frames, running into each other
    bad += [rc(dst=sp), rc(dst=sp + 1), rc(dst=sp + n - 1), rc(src=sp + n - 1, dst=sp), rc(src=sp + 2 * n - 1, dst=sp),
            rc(src=sp + 2 * n, dst=sp + 1)]                                               # overlapping
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]} and bad[0] == -2, bad        # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(2 * n, dtype=torch.bool))
    assert torch.equal(both[:n], both[n:2 * n]) and torch.equal(both[:n], both[2 * n:])   # nothing was written into the refused dst ranges
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_field_to_frame")
    # ranges that touch without overlapping are taken, and after the refusals a good call still works
    assert rc(dst=sp + n) == 0
    torch.cuda.synchronize()
    assert torch.equal(both[n:].cpu().view(T, 2 * Hf, W, 3), restated(F, 0, "cubic"))
    assert rc() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(T, 2 * Hf, W, 3), restated(F, 0, "cubic"))
    assert rc(dims=(1, 1, W), fs=W * 3, rs=1 << 40) == 0          # AT the row_stride bound a call is taken (one row: the stride is never applied)
    torch.cuda.synchronize()
    assert torch.equal(out[:6 * W].cpu().view(1, 2, W, 3), restated(F[:1, :1], 0, "cubic"))


# ---------------------------------------------------------------------------------------------------- the sources
H0, W0 = 88, 160          # H % 4 == 0: a 4:2:0 surface splits into two 4:2:0 fields


def _np16(a):
    """numpy uint16 -> the torch.int16 bit pattern over the same memory"""
    return torch.from_numpy(a.view(np.int16))


@functools.lru_cache(maxsize=None)
def surfaces():
    """name -> (build(device) -> the surface as the frames entries take it, fields(src, parity, layout) -> the same kind over the
    field's rows copied dense by the host, or None for the RGB kinds).  40 frames of 88 x 160 cut from one seeded video with a
    new scene every five frames."""
    from tdc_video_amd import ops, preprocess as pp
    f = frames_of(H0, W0).numpy()
    T0 = f.shape[0]
    rng = np.random.RandomState(11)
    y8 = np.ascontiguousarray(f[..., 1])
    u8, v8 = f[:, ::2, ::2, 0], f[:, ::2, ::2, 2]
    uv8 = np.ascontiguousarray(np.stack([u8, v8], -1).reshape(T0, H0 // 2, W0))
    y10, uv10 = (y8.astype(np.uint16) << 8) | 0x2a, (uv8.astype(np.uint16) << 8) | 0x15        # P010: the sample in the high 10 bits, junk below
    yuy2 = np.ascontiguousarray(np.stack([y8[:, :, 0::2], f[:, :, ::2, 0], y8[:, :, 1::2], f[:, :, ::2, 2]], -1).reshape(T0, H0, 2 * W0))
    words = ops.yuv_packed_words("v210", W0)
    scene = rng.randint(0, 1 << 30, (T0 // 5, 1, H0, words)).astype(np.uint32)
    v210 = np.ascontiguousarray(((scene + np.arange(5, dtype=np.uint32)[None, :, None, None] * 3) & 0x3fffffff).reshape(T0, H0, words))
    bgra = np.full((T0, H0, W0 + 8, 4), 7, np.uint8)               # pitched: 8 pixels of padding per row
    bgra[:, :, :W0, :3] = f[..., ::-1]
    chw = np.ascontiguousarray(f.transpose(0, 3, 1, 2))

    def dev(a, device):
        t = a if torch.is_tensor(a) else torch.from_numpy(a)
        return t.cuda() if device == "cuda" else t

    def dense_fields(planes, parity, layout):
        return [ic.field_of(p, parity, layout) for p in planes]

    return {
        "uint8": (lambda d: dev(f, d), None, lambda: f),
        "chw": (lambda d: pp.RgbFrames.chw(dev(chw, d)), None, lambda: f),
        "bgra_pitched": (lambda d: pp.RgbFrames(dev(bgra, d)[:, :, :W0], "hwc", "bgra"), None, lambda: f),
        "nv12": (lambda d: pp.YuvFrames.nv12(dev(y8, d), dev(uv8, d), matrix="bt709"),
                 lambda p, l: pp.YuvFrames.nv12(*dense_fields((y8, uv8), p, l), matrix="bt709"), None),
        "p010_pq": (lambda d: pp.YuvFrames.p010(dev(_np16(y10), d), dev(_np16(uv10), d), matrix="bt2020", transfer="pq"),
                    lambda p, l: pp.YuvFrames.p010(*dense_fields((y10, uv10), p, l), matrix="bt2020", transfer="pq"), None),
        "yuy2": (lambda d: pp.YuvFrames.yuy2(dev(yuy2, d)), lambda p, l: pp.YuvFrames.yuy2(*dense_fields((yuy2,), p, l)), None),
        "v210": (lambda d: pp.YuvFrames.v210(dev(torch.from_numpy(v210.view(np.int32)), d), W0, matrix="bt709"),
                 lambda p, l: pp.YuvFrames.v210(dense_fields((v210,), p, l)[0], W0, matrix="bt709"), None),
    }


@functools.lru_cache(maxsize=None)
def host_rebuilt(name, field="top", fill="linear", layout="interleaved"):
    """the uint8 frames [40, 88, 160, 3] a host rebuilds with the restatement from the kept field of surface `name`: the RGB
    kinds' field rows cut on the host; the YUV kinds' field planes copied dense by the host and converted by the launch that
    exists (rgb_of), then restated"""
    _, fields, rgb = surfaces()[name]
    p = ic.FIELDS.index(field)
    F = ic.field_of(rgb(), p, layout) if fields is None else rgb_of(fields(p, layout)).numpy()
    assert F.shape == (40, H0 // 2, W0, 3)
    return torch.from_numpy(ic.rebuild(F, p, fill))


FUNNEL = [("uint8", "host", "top", "linear", "interleaved"), ("uint8", "cuda", "top", "linear", "interleaved"),
          ("uint8", "cuda", "bottom", "cubic", "interleaved"), ("chw", "host", "top", "cubic", "interleaved"),
          ("bgra_pitched", "cuda", "bottom", "linear", "interleaved"), ("nv12", "host", "top", "linear", "interleaved"),
          ("nv12", "cuda", "bottom", "cubic", "sequential_tb"), ("p010_pq", "host", "top", "linear", "interleaved"),
          ("yuy2", "cuda", "top", "cubic", "interleaved"), ("v210", "host", "bottom", "cubic", "interleaved"),
          ("uint8", "host", "top", "linear", "sequential_tb"), ("uint8", "cuda", "bottom", "linear", "sequential_bt")]


def interlaced(name, device, field="top", fill="linear", layout="interleaved"):
    from tdc_video_amd import preprocess as pp
    return pp.Interlaced(surfaces()[name][0](device), field, fill, layout)


@pytest.mark.parametrize("name,device,field,fill,layout", FUNNEL)
def test_encode_frames_equals_the_call_on_host_rebuilt_frames(fx, name, device, field, fill, layout):  # noqa: F811
    enc, pid = fx["enc"], fx["pid"]
    y = host_rebuilt(name, field, fill, layout)
    x = interlaced(name, device, field, fill, layout)
    assert x.shape == (40, H0, W0, 3) and x.is_cuda == (device == "cuda")
    wi, gi = {}, {}
    want = enc.encode_frames(y, 9, 8, pid, frame_cap=30, info=wi)              # T0 = 40 above the cap: a1 sub-samples
    got = enc.encode_frames(x, 9, 8, pid, frame_cap=30, info=gi)
    assert torch.equal(got, want) and gi == wi and gi["frames_resized"] == 30 == len(gi["frame_indices"])
    assert torch.equal(enc.encode_frames(x, 9, 8, pid), enc.encode_frames(y, 9, 8, pid))          # every frame kept


def test_prompts_export_image_and_oriented(fx):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc, pid = fx["enc"], fx["pid"]
    for name, device, field, fill in (("uint8", "host", "bottom", "cubic"), ("nv12", "cuda", "top", "linear")):
        y, x = host_rebuilt(name, field, fill), interlaced(name, device, field, fill)
        qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid),
              dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:])]
        i1, i2 = [{} for _ in qs], [{} for _ in qs]
        for a, b in zip(enc.encode_frames_prompts(x, qs, frame_cap=30, pad_fraction=1.0, infos=i1),
                        enc.encode_frames_prompts(y, qs, frame_cap=30, pad_fraction=1.0, infos=i2)):
            assert torch.equal(a, b)
        assert i1 == i2
        w, g = enc.export_features_from_frames(y, slab=16), enc.export_features_from_frames(x, slab=16)
        assert g.signature == w.signature and g.image_size == w.image_size == (H0, W0) and g.frames == 40
        assert memcheck.same_bits(g.siglip, w.siglip) and memcheck.same_bits(g.dino, w.dino)
        i1, i2 = {}, {}                                             # the image form: one frame, sliced out of the wrapper
        assert torch.equal(enc.encode_frames(x[3:4], None, 8, None, image=True, info=i1),
                           enc.encode_frames(y[3:4], None, 8, None, image=True, info=i2)) and i1 == i2
        assert i1["frames_in"] == i1["frames_resized"] == 1
        # inside an Oriented: the field is rebuilt first, then the frame is turned
        upright = torch.from_numpy(oc.orient(y.numpy(), 90, False))
        wi, gi = {}, {}
        want = enc.encode_frames(upright, 9, 8, pid, frame_cap=30, info=wi)
        assert torch.equal(enc.encode_frames(pp.Oriented(x, 90), 9, 8, pid, frame_cap=30, info=gi), want) and gi == wi
        assert gi["final_size"] == wi["final_size"]
        assert torch.equal(enc.encode_frames(pp.Oriented(x, 0), 9, 8, pid, frame_cap=30), enc.encode_frames(y, 9, 8, pid, frame_cap=30))


def test_frame_cache_hits_after_the_video_was_asked_through_host_rebuilt_frames(fx):  # noqa: F811
    enc, pid = fx["enc"], fx["pid"]
    y, x = host_rebuilt("uint8", "top", "cubic"), interlaced("uint8", "host", "top", "cubic")
    want = enc.encode_frames(y, 9, 8, pid, frame_cap=30)
    c = enc.new_cache(1 << 30)
    i1, i2, i3 = {}, {}, {}
    assert torch.equal(enc.encode_frames(y, 9, 8, pid, frame_cap=30, info=i1, cache=c), want)
    assert i1["cache"]["frames_encoded"] == 30
    assert torch.equal(enc.encode_frames(x, 9, 8, pid, frame_cap=30, info=i2, cache=c), want)
    assert i2["cache"]["frames_encoded"] == 0 and i2["cache"]["frames_hit"] == i2["cache"]["frames"] == 30
    assert torch.equal(enc.encode_frames(interlaced("uint8", "cuda", "top", "cubic"), 9, 8, pid, frame_cap=30, info=i3, cache=c), want)
    assert i3["cache"]["frames_encoded"] == 0 and i3["frame_indices"] == i1["frame_indices"]


def test_mixin_interlaced_inputs_equal_the_host_rebuilt_call(fx):  # noqa: F811
    y = host_rebuilt("uint8", "bottom", "linear")
    lm = loaded_lm(fx["W"], fx["o"], tdc_frame_cap=30)
    ids = torch.from_numpy(fx["o"]["input_ids"])
    lm.get_model().tdc_engine().frame_towers = towers()
    lm.get_model().config.tdc_frame_inputs = True
    want = _call(lm, ids, [[y], None], (W0, H0), [fx["pid"]])
    _same(_call(lm, ids, [[interlaced("uint8", "host", "bottom")], None], (W0, H0), [fx["pid"]]), want)
    _same(_call(lm, ids, [[interlaced("uint8", "cuda", "bottom")], [None]], (W0, H0), [fx["pid"]]), want)
    want_im = _call(lm, ids, [y[:2], None], (W0, H0), [fx["pid"]] * 2, 2)                  # single images: sliced per sample
    _same(_call(lm, ids, [interlaced("uint8", "host", "bottom")[:2], None], (W0, H0), [fx["pid"]] * 2, 2), want_im)


# ---------------------------------------------------------------------------------------------------- preprocess_selected
IDX = [0, 2, 3, 5, 8, 9, 10, 13, 14, 15]          # 10 of 16: 4 + 4 + 2 at slab 4


def test_preprocess_selected_bits_and_bytes_uploaded():
    from tdc_video_amd import preprocess as pp
    Hf = H0 // 2
    for name, field, fill, layout, host_bytes in (("uint8", "top", "linear", "interleaved", Hf * W0 * 3),
                                                  ("uint8", "bottom", "cubic", "sequential_tb", Hf * W0 * 3),
                                                  ("nv12", "top", "cubic", "interleaved", Hf * W0 + Hf // 2 * W0),
                                                  ("bgra_pitched", "top", "linear", "interleaved", Hf * W0 * 4)):
        want = reference_pixels(host_rebuilt(name, field, fill, layout)[:16][IDX])
        for device in ("host", "cuda"):
            for slab in (4, 64):
                stats = {}
                got = pp.preprocess_selected(interlaced(name, device, field, fill, layout)[:16], IDX, towers(), torch.float16, slab, stats=stats)
                assert all(memcheck.same_bits(g, w) for g, w in zip(got, want)), (name, device, slab)
                # exactly the kept frames' field bytes: half of what the woven frames would upload
                assert stats == dict(frames_in=16, frames_resized=10, bytes_uploaded=0 if device == "cuda" else 10 * host_bytes)
    want = reference_pixels(host_rebuilt("uint8", "top", "linear")[:16], torch.bfloat16)          # idx=None, bfloat16, pinned and numpy
    f = frames_of(H0, W0)[:16]
    for src in (f.clone().pin_memory(), f.numpy(), f.cuda()):
        got = pp.preprocess_selected(pp.Interlaced(src), None, towers(), torch.bfloat16, 7)
        assert all(memcheck.same_bits(g, w) for g, w in zip(got, want))


def test_device_frames_whose_pixels_are_not_dense(monkeypatch):
    """uint8 [T0, H, W, 3] views that check_frames takes but whose pixels are not three adjacent bytes - a permuted channel-first
    tensor, rgba[..., :3], an identity RgbFrames over either: read in place they would be other bytes, so with every frame kept
    on the device their field rows are gathered dense first, as under a selection and on the host; ops.field_to_frame refuses
    such a view by ValueError, not by an assert"""
    from tdc_video_amd import lib as L, ops, preprocess as pp
    f = frames_of(H0, W0)[:16]
    chw = f.permute(0, 3, 1, 2).contiguous()
    rgba = torch.cat([f, torch.full((16, H0, W0, 1), 9, dtype=torch.uint8)], 3)
    views = {"permuted_chw": lambda t: t(chw).permute(0, 2, 3, 1), "rgba_cut": lambda t: t(rgba)[..., :3]}
    for name, view in views.items():
        v = view(lambda a: a.cuda())
        assert torch.equal(v.cpu(), f) and not v.is_contiguous() and not ops.field_pixels_dense(v[:, 0::2])
        with pytest.raises(ValueError, match="dense"):
            ops.field_to_frame(v[:, 0::2], 0, "linear")
    log = []
    monkeypatch.setattr(L, "_lib", _TracedFields(L.load(), log))
    for field, fill, layout in (("top", "linear", "interleaved"), ("bottom", "cubic", "sequential_tb")):
        p, c = ic.FIELDS.index(field), ic.FILLS.index(fill)
        rebuilt = torch.from_numpy(ic.rebuild(ic.field_of(f.numpy(), p, layout), p, fill))
        want_all, want_idx = reference_pixels(rebuilt), reference_pixels(rebuilt[IDX])
        for name, view in views.items():
            for where in (lambda a: a.cuda(), lambda a: a):
                for wrap in (lambda x: x, lambda x: pp.RgbFrames(x)):
                    src = wrap(view(where))
                    del log[:]
                    got = pp.preprocess_selected(pp.Interlaced(src, field, fill, layout), None, towers(), torch.float16, 7)      # every frame kept
                    assert all(memcheck.same_bits(g, w) for g, w in zip(got, want_all)), (name, field)
                    assert [k for k in log if k[0] == "tdc_field_to_frame"] == [("tdc_field_to_frame", n, H0 // 2, W0, p, c) for n in (7, 7, 2)]
                    got = pp.preprocess_selected(pp.Interlaced(src, field, fill, layout), IDX, towers(), torch.float16, 7)
                    assert all(memcheck.same_bits(g, w) for g, w in zip(got, want_idx)), (name, field)
        turned = reference_pixels(torch.from_numpy(oc.orient(rebuilt.numpy(), 90, False)))
        got = pp.preprocess_selected(pp.Oriented(pp.Interlaced(views["permuted_chw"](lambda a: a.cuda()), field, fill, layout), 90), None,
                                     towers(), torch.float16, 7)
        assert all(memcheck.same_bits(g, w) for g, w in zip(got, turned))


def test_preprocess_selected_memory_contract(monkeypatch):
    """outputs in guarded arenas, every scratch allocated through torch.empty and guarded, dropped frames AND the other field's
    rows holding 0x00, then 0xFF: bit-identical outputs, nothing written outside out[0:len(idx)] or outside a scratch"""
    import importlib
    pp = importlib.import_module("tdc_video_amd.preprocess")      # under the name memcheck.poison_empty looks for
    frames = frames_of(H0, W0)[:16]
    want = reference_pixels(host_rebuilt("uint8", "bottom", "cubic")[:16][IDX])
    T = len(IDX)
    results = []
    for pattern in memcheck.PATTERNS:
        src = torch.full((16, H0, W0, 3), pattern, dtype=torch.uint8)
        src[IDX, 1::2] = frames[IDX, 1::2]                         # only the kept frames' bottom field is there
        outs = [memcheck.guarded((T + 2, 3, R, R), torch.float16, "cuda", 1, 1) for _ in range(2)]
        with monkeypatch.context() as mp:
            inner = memcheck.poison_empty(mp, pattern, guard_bytes=4096)
            got = pp.preprocess_selected(pp.Interlaced(src.cuda(), "bottom", "cubic"), IDX, towers(), torch.float16, 3, out=[v for v, _ in outs])
        torch.cuda.synchronize()
        rows = torch.zeros(T + 2, dtype=torch.bool)
        rows[:T] = True
        for (_, arena), g, w in zip(outs, got, want):
            memcheck.assert_untouched(arena, rows)
            assert memcheck.same_bits(g, w) and memcheck.all_finite(g)
        assert len(inner) >= 2, "the scratches were not allocated through torch.empty"
        for a in inner:
            memcheck.assert_untouched(a, what="scratch")
        results.append([g.clone() for g in got])
        host = pp.preprocess_selected(pp.Interlaced(src, "bottom", "cubic"), IDX, towers(), torch.float16, 3)      # the same from host memory
        assert all(memcheck.same_bits(g, w) for g, w in zip(host, want))
    assert all(memcheck.same_bits(a, b) for a, b in zip(*results))


# ---------------------------------------------------------------------------------------------------- the launch trace
class _TracedFields(_Traced):
    SIZES = dict(_Traced.SIZES, tdc_field_to_frame=slice(3, 8))       # (n, Hf, W, parity, fill)


def test_launch_trace(fx, monkeypatch):  # noqa: F811
    from tdc_video_amd import lib as L, preprocess as pp
    log = []
    monkeypatch.setattr(L, "_lib", _TracedFields(L.load(), log))
    LAUNCHES = ("tdc_yuv420_to_rgb", "tdc_yuv_to_rgb", "tdc_yuv_hdr_to_rgb", "tdc_yuv_packed_to_rgb", "tdc_pack_rgb",
                "tdc_field_to_frame", "tdc_orient_frames", "tdc_preprocess_frames")

    def trace(src, slab=4):
        del log[:]
        pp.preprocess_selected(src, IDX, towers(), torch.float16, slab)
        return [c for c in log if c[0] in LAUNCHES]

    Hf = H0 // 2
    resize = [("tdc_preprocess_frames", n, H0, W0, R) for n in (4, 4, 2)]
    for name, front in (("uint8", None), ("chw", "tdc_pack_rgb"), ("bgra_pitched", "tdc_pack_rgb"), ("nv12", "tdc_yuv420_to_rgb"),
                        ("p010_pq", "tdc_yuv_hdr_to_rgb"), ("yuy2", "tdc_yuv_packed_to_rgb"), ("v210", "tdc_yuv_packed_to_rgb")):
        for device in ("host", "cuda"):
            plain = trace(surfaces()[name][0](device)[:16])
            assert not any(c[0] == "tdc_field_to_frame" for c in plain) and sum(c[0] == "tdc_preprocess_frames" for c in plain) == 6
            for field, fill in (("top", "linear"), ("bottom", "cubic")):
                p, f = ic.FIELDS.index(field), ic.FILLS.index(fill)
                got = trace(interlaced(name, device, field, fill)[:16])
                want = []
                for n, r in zip((4, 4, 2), resize):          # per slab: the conversion / pack, ONE rebuild, the towers
                    want += ([(front,)] if front else []) + [("tdc_field_to_frame", n, Hf, W0, p, f), r, r]
                assert got == want, (name, device, field, fill)
                turned = trace(pp.Oriented(interlaced(name, device, field, fill)[:16], 90))
                want = []
                for n in (4, 4, 2):
                    r = ("tdc_preprocess_frames", n, W0, H0, R)
                    want += ([(front,)] if front else []) + [("tdc_field_to_frame", n, Hf, W0, p, f), ("tdc_orient_frames", n, H0, W0, 1, 0), r, r]
                assert turned == want, (name, device, field, fill)
    # through the engine: a call without an Interlaced issues exactly the calls it issued - none of this section's
    enc, pid = fx["enc"], fx["pid"]
    del log[:]
    enc.encode_frames(host_rebuilt("uint8"), 9, 8, pid, frame_cap=30)
    plain = list(log)
    assert len(plain) > 10 and not any(c[0] == "tdc_field_to_frame" for c in plain)
    del log[:]
    enc.encode_frames(interlaced("uint8", "host"), 9, 8, pid, frame_cap=30)
    assert [c for c in log if c[0] != "tdc_field_to_frame"] == plain
    assert [c for c in log if c[0] == "tdc_field_to_frame"] == [("tdc_field_to_frame", 30, Hf, W0, 0, 0)]      # one slab of 30
