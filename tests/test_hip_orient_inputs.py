"""GPU (-m gpu): encode from rotated video.  tdc_orient_frames against the numpy restatement of the
orientation (orient_cases) - the shapes where tiling can go wrong, every load / store form, its memory contract, offsets past
2^32 and its refusals - and the frames funnel on the tiny fixture engine of test_hip_frame_inputs: everything behind the
orientation is the frames path that exists, so every comparison is bit for bit against the same call on the frames a host
turned upright beforehand.

The forms.  The transposing cases (quarters 1, 3) load with 4-byte words when src and 3 W are multiples of 4 and store with
4-byte words when dst and 3 H are, each on its own, bytes otherwise; the others move 12-byte groups when src, dst and 3 W are
multiples of 4, pixels otherwise.  Of SHAPES only (64, 64), (68, 132), (4, 6) and (6, 4) can take a word form, and the pointer
offsets 0 .. 3 of src and of dst then reach every combination: (0, 0) word / word, (k, 0) byte / word, (0, k) word / byte,
(k, k') byte / byte; (4, 6) and (6, 4) mix them at offset 0."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import memcheck
import orient_cases as oc
import test_hip_memory_contract as contract
from test_hip_boundary import loaded_lm
from test_hip_frame_inputs import R, _call, _same, frames_of, fx, reference_pixels, towers  # noqa: F401  (fx: the engine fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (5, 1), (37, 91), (63, 65), (64, 64), (66, 130),      # single pixels, rows, ragged tiles, one whole tile, several
          (68, 132), (4, 6), (6, 4)]          # both sides multiples of 4 with ragged edge tiles; one side a multiple of 4
QH = [(q, h) for q in range(4) for h in (0, 1)]


def restated(S, q, h):
    return torch.from_numpy(oc.orient(S, 90 * q, bool(h)))


# ---------------------------------------------------------------------------------------------------- the kernel
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  tdc_orient_frames's is the function below: it is entered
# there under its own name (not a test_ name: that module collects nothing new).
@contract.covers("tdc_orient_frames")
def orient_frames_memory_contract(T, H, W, offsets=range(4)):
    """tdc_orient_frames for all eight (quarters, hflip), from src / dst pointers 0 .. 3 bytes into a larger allocation (every
    load / store form): dst in a guarded arena - nothing outside its 3 T H W bytes changes; src between poisoned bytes holding
    0x00, then 0xFF - the output is the restatement's either way."""
    from tdc_video_amd import ops
    S = oc.random_frames(T, H, W)
    n = S.size
    flat = torch.from_numpy(S).reshape(-1).cuda()
    want = {qh: restated(S, *qh).cuda() for qh in QH}
    for pattern in memcheck.PATTERNS:
        for so in offsets:
            held, _ = memcheck.poisoned(flat, 64, 64, fill=pattern, rows=torch.arange(so, so + n), total_rows=n + 3)
            src = held[so:so + n].view(T, H, W, 3)
            assert src.data_ptr() % 4 == so
            for do in offsets:
                room, arena = memcheck.guarded((n + 3,), torch.uint8, "cuda", 64, 64, fill=pattern)
                written = torch.zeros(n + 3, dtype=torch.bool)
                written[do:do + n] = True
                for q, h in QH:
                    arena.buf.fill_(pattern)
                    dst = room[do:do + n].view(want[q, h].shape)
                    assert dst.data_ptr() % 4 == do
                    ops.orient_frames(src, q, h, out=dst)
                    torch.cuda.synchronize()
                    memcheck.assert_untouched(arena, written)
                    assert torch.equal(dst, want[q, h]), (T, H, W, q, h, so, do, pattern)


contract.orient_frames_memory_contract = orient_frames_memory_contract


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_all_eight_orientations_every_form_inside_guards_and_poison(H, W, T):
    orient_frames_memory_contract(T, H, W)


def test_identity_is_a_plain_copy_and_ops_allocates_the_upright_shape():
    from tdc_video_amd import ops
    S = oc.random_frames(2, 37, 91)
    src = torch.from_numpy(S).cuda()
    assert torch.equal(ops.orient_frames(src, 0, 0), src)
    for q, h in QH:
        got = ops.orient_frames(src, q, h)
        assert tuple(got.shape) == ((2, 91, 37, 3) if q & 1 else (2, 37, 91, 3)) and torch.equal(got.cpu(), restated(S, q, h))


def test_offsets_past_2_to_the_32():
    """T = 40 frames of 6000 x 6000: 4.32 GB in, 4.32 GB out - the last frame starts 4.2 GB into both"""
    from tdc_video_amd import ops
    T, H, W = 40, 6000, 6000
    src = torch.empty((T, H, W, 3), dtype=torch.uint8, device="cuda").random_(0, 256)
    out = torch.empty_like(src)
    ops.orient_frames(src, 1, 0, out=out)
    for t in (0, T - 1):
        assert torch.equal(out[t], torch.rot90(src[t], -1, dims=(0, 1))), t
    out.zero_()
    ops.orient_frames(src, 2, 1, out=out)                         # the vertical flip
    assert torch.equal(out[T - 1], src[T - 1].flip(0))
    del src, out
    torch.cuda.empty_cache()


def test_badarg_before_any_launch():
    from tdc_video_amd import lib as L
    lib = L.load()
    T, H, W = 2, 4, 6
    n = T * H * W * 3
    both = torch.from_numpy(np.concatenate([oc.random_frames(T, H, W).reshape(-1)] * 2)).cuda()      # src, then n more bytes
    out, arena = memcheck.guarded((n,), torch.uint8, "cuda", 64, 64)
    sp = both.data_ptr()

    def rc(src=sp, dims=(T, H, W), q=1, h=0, dst=out.data_ptr()):
        return lib.tdc_orient_frames(C.c_void_p(src), *dims, q, h, C.c_void_p(dst), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [rc(src=0), rc(dst=0)]
    for i in range(3):
        for v in (0, -1, 65536):
            dims = [T, H, W]
            dims[i] = v
            bad.append(rc(dims=tuple(dims)))
    bad += [rc(q=-1), rc(q=4), rc(q=90), rc(h=-1), rc(h=2)]
    bad += [rc(dst=sp), rc(dst=sp + 1), rc(dst=sp + n - 1), rc(src=sp + n - 1, dst=sp), rc(src=sp + n, dst=sp + 1)]     # overlapping
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad      # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(n, dtype=torch.bool))
    assert torch.equal(both[:n], both[n:])                            # and nothing was written into the refused dst ranges
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_orient_frames")
    # ranges that touch without overlapping are taken, either way round
    assert rc(dst=sp + n, q=2) == 0 and rc(src=sp + n, dst=sp, q=2) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- preprocess_selected
IDX = [0, 2, 3, 5, 8, 9, 10, 13, 14, 15]          # 10 of 16: 7 + 3 at slab 7


@pytest.mark.parametrize("H,W", [(90, 160), (126, 126), (45, 81)])
def test_preprocess_selected_on_oriented_equals_process_images_of_the_upright_frames(H, W):
    from tdc_video_amd import preprocess as pp
    frames = frames_of(H, W)[:16]
    sources = {"cuda": frames.cuda(), "pageable": frames, "pinned": frames.clone().pin_memory(), "numpy": frames.numpy()}
    for rotate, hflip in oc.ALL:
        want = reference_pixels(torch.from_numpy(oc.orient(frames.numpy()[IDX], rotate, hflip)))
        for name, src in sources.items():
            for slab in (7, 64) if name != "cuda" else (1, 7, 64):
                stats = {}
                got = pp.preprocess_selected(pp.Oriented(src, rotate, hflip), IDX, towers(), torch.float16, slab, stats=stats)
                assert len(got) == 2
                for g, w in zip(got, want):
                    assert g.is_cuda and tuple(g.shape) == (10, 3, R, R) and memcheck.same_bits(g, w), (rotate, hflip, name, slab)
                assert stats == dict(frames_in=16, frames_resized=10, bytes_uploaded=0 if name == "cuda" else 10 * H * W * 3)
    want = reference_pixels(torch.from_numpy(oc.orient(frames.numpy(), 270, False)), torch.bfloat16)      # idx=None, bfloat16
    got = pp.preprocess_selected(pp.Oriented(sources["pinned"], 270), None, towers(), torch.bfloat16, 7)
    assert all(memcheck.same_bits(g, w) for g, w in zip(got, want))


def test_preprocess_selected_on_oriented_memory_contract(monkeypatch):
    """outputs in guarded arenas, every scratch allocated through torch.empty and guarded, dropped frames holding 0x00, then
    0xFF: bit-identical outputs, nothing written outside out[0:len(idx)] or outside a scratch"""
    import importlib
    pp = importlib.import_module("tdc_video_amd.preprocess")      # under the name memcheck.poison_empty looks for
    H, W = 90, 160
    frames = frames_of(H, W)[:16].cuda()
    want = reference_pixels(torch.from_numpy(oc.orient(frames.cpu().numpy()[IDX], 90, False)))
    T = len(IDX)
    results = []
    for pattern in memcheck.PATTERNS:
        src, _ = memcheck.poisoned(frames[IDX], 1, 1, fill=pattern, rows=IDX, total_rows=16)
        outs = [memcheck.guarded((T + 2, 3, R, R), torch.float16, "cuda", 1, 1) for _ in range(2)]
        with monkeypatch.context() as mp:
            inner = memcheck.poison_empty(mp, pattern, guard_bytes=4096)
            got = pp.preprocess_selected(pp.Oriented(src, 90), IDX, towers(), torch.float16, 3, out=[v for v, _ in outs])
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
    assert all(memcheck.same_bits(a, b) for a, b in zip(*results))


# ---------------------------------------------------------------------------------------------------- the launch trace
class _Traced:
    """the loaded library with every C-ABI call logged: its name and, of the two calls that see the frames' shape, the sizes"""
    SIZES = {"tdc_preprocess_frames": slice(1, 5), "tdc_preprocess_scratch_bytes": slice(0, 4), "tdc_orient_frames": slice(1, 6)}

    def __init__(self, real, log):
        self.__dict__.update(_real=real, _log=log)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("tdc_"):
            return fn

        def call(*a):
            self._log.append((name,) + tuple(a[self.SIZES[name]]) if name in self.SIZES else (name,))
            return fn(*a)
        return call


def _turned(call):
    """a logged call with the H and W of its sizes exchanged"""
    if call[0] == "tdc_preprocess_frames":
        return call[:2] + (call[3], call[2]) + call[4:]
    if call[0] == "tdc_preprocess_scratch_bytes":
        return call[:2] + (call[3], call[2]) + call[4:]
    return call


def test_launch_trace(fx, monkeypatch):  # noqa: F811
    from tdc_video_amd import lib as L, preprocess as pp
    from test_hip_yuv_inputs import video as nv12_video
    frames = frames_of(90, 160)[:16].clone().pin_memory()
    nv12 = nv12_video()[0][:16]
    log = []
    monkeypatch.setattr(L, "_lib", _Traced(L.load(), log))

    def trace(src, slab=4):
        del log[:]
        stats = {}
        pp.preprocess_selected(src, IDX, towers(), torch.float16, slab, stats=stats)
        return list(log), stats

    for inner in (frames, nv12):
        base, base_stats = trace(inner)
        assert sum(c[0] == "tdc_preprocess_frames" for c in base) == 6 and not any(c[0] == "tdc_orient_frames" for c in base)
        # the identity: exactly the calls the wrapped frames issue, in their order
        assert trace(pp.Oriented(inner, 0, False)) == (base, base_stats)
        for rotate, hflip in oc.NON_IDENTITY:
            got, stats = trace(pp.Oriented(inner, rotate, hflip))
            q = rotate // 90
            turns = [c for c in got if c[0] == "tdc_orient_frames"]
            assert turns == [("tdc_orient_frames", n, 90, 160, q, int(hflip)) for n in (4, 4, 2)]      # one per slab of 10 kept frames
            rest = [c for c in got if c[0] != "tdc_orient_frames"]
            want = [_turned(c) for c in base] if q & 1 else base
            # RGB frames: the tower-outer loop becomes slab-outer, the same calls in another order; YUV is slab-outer already
            assert (sorted(rest) == sorted(want)) if inner is frames else (rest == want), (rotate, hflip)
            assert stats == base_stats and stats["bytes_uploaded"] > 0
            # every slab is turned before the towers read it
            at = [i for i, c in enumerate(got) if c[0] in ("tdc_orient_frames", "tdc_preprocess_frames")]
            assert [got[i][0] for i in at] == ["tdc_orient_frames", "tdc_preprocess_frames", "tdc_preprocess_frames"] * 3
    # through the engine: the identity wrapper changes no call of a whole encode either
    enc, pid = fx["enc"], fx["pid"]
    video = frames_of(90, 160)
    del log[:]
    a = enc.encode_frames(video, 9, 8, pid, frame_cap=30)
    plain = list(log)
    del log[:]
    b = enc.encode_frames(pp.Oriented(video, 0, False), 9, 8, pid, frame_cap=30)
    assert log == plain and len(plain) > 10 and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- the engine
ORIENTATIONS = [(90, False), (270, True), (180, False)]


@functools.lru_cache(maxsize=None)
def stored_and_upright(rotate, hflip, H=90, W=160):
    """a landscape video of 40 frames as stored, and the contiguous frames a host turns upright beforehand"""
    stored = frames_of(H, W)
    return stored, torch.from_numpy(oc.orient(stored.numpy(), rotate, hflip))


@pytest.mark.parametrize("rotate,hflip", ORIENTATIONS)
def test_encode_frames_prompts_export_and_image(fx, rotate, hflip):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc, pid = fx["enc"], fx["pid"]
    stored, upright = stored_and_upright(rotate, hflip)
    size = oc.out_hw(90, 160, rotate)
    wi = {}
    want = enc.encode_frames(upright, 9, 8, pid, frame_cap=30, info=wi)                # T0 = 40 above the cap: a1 sub-samples
    assert wi["frames_resized"] == 30 == len(wi["frame_indices"])
    for src in (stored, stored.cuda(), stored.numpy()):                                # host, device: the same bits
        gi = {}
        got = enc.encode_frames(pp.Oriented(src, rotate, hflip), 9, 8, pid, frame_cap=30, info=gi)
        assert torch.equal(got, want) and gi == wi
        assert all(gi[k] == wi[k] for k in ("frame_indices", "final_size", "frames_resized"))
    o = pp.Oriented(stored, rotate, hflip)
    assert torch.equal(enc.encode_frames(o, 9, 8, pid), enc.encode_frames(upright, 9, 8, pid))        # every frame kept
    qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid),
          dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:])]
    i1, i2 = [{} for _ in qs], [{} for _ in qs]
    for a, b in zip(enc.encode_frames_prompts(o, qs, frame_cap=30, pad_fraction=1.0, infos=i1),
                    enc.encode_frames_prompts(upright, qs, frame_cap=30, pad_fraction=1.0, infos=i2)):
        assert torch.equal(a, b)
    assert i1 == i2
    for store in ("f16", "e4m3"):
        w = enc.export_features_from_frames(upright, store=store, slab=16)
        g = enc.export_features_from_frames(o, store=store, slab=16)
        assert g.signature == w.signature and g.image_size == w.image_size == size and g.frames == 40
        assert memcheck.same_bits(g.siglip, w.siglip) and memcheck.same_bits(g.dino, w.dino)
        if store == "e4m3":
            assert torch.equal(g.siglip_scale, w.siglip_scale) and torch.equal(g.dino_scale, w.dino_scale) and torch.equal(g.sims, w.sims)


def test_one_image_from_an_exif_orientation(fx):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc = fx["enc"]
    stored, upright = stored_and_upright(90, False)                 # EXIF 6 is (90, False)
    i1, i2 = {}, {}
    got = enc.encode_frames(pp.Oriented.exif(stored[3:4], 6), None, 8, None, image=True, info=i1)
    assert torch.equal(got, enc.encode_frames(upright[3:4], None, 8, None, image=True, info=i2)) and i1 == i2
    assert i1["frames_in"] == i1["frames_resized"] == 1
    for orientation, (rotate, hflip) in oc.EXIF.items():            # all eight, on the device
        up = torch.from_numpy(oc.orient(stored[3:4].numpy(), rotate, hflip))
        assert torch.equal(enc.encode_frames(pp.Oriented.exif(stored[3:4].cuda(), orientation), None, 8, None, image=True),
                           enc.encode_frames(up, None, 8, None, image=True)), orientation


def test_frame_cache_hits_whichever_way_the_video_was_first_asked(fx):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc, pid = fx["enc"], fx["pid"]
    stored, upright = stored_and_upright(270, True)
    o = pp.Oriented(stored, 270, True)
    want = enc.encode_frames(upright, 9, 8, pid, frame_cap=30)
    c = enc.new_cache(1 << 30)
    i1, i2, i3, i4 = {}, {}, {}, {}
    assert torch.equal(enc.encode_frames(o, 9, 8, pid, frame_cap=30, info=i1, cache=c), want)
    assert i1["cache"]["frames_encoded"] == 30
    assert torch.equal(enc.encode_frames(o, 9, 8, pid, frame_cap=30, info=i2, cache=c), want)      # the second question hits
    assert i2["cache"]["frames_encoded"] == 0 and i2["cache"]["frames_hit"] == i2["cache"]["frames"] == 30
    assert i2["frame_indices"] == i1["frame_indices"] and i2["frames_resized"] == 30
    # first asked through host-rotated frames, then through the wrapper: all hits
    c2 = enc.new_cache(1 << 30)
    assert torch.equal(enc.encode_frames(upright, 9, 8, pid, frame_cap=30, info=i3, cache=c2), want)
    assert i3["cache"]["frames_encoded"] == 30
    assert torch.equal(enc.encode_frames(o, 9, 8, pid, frame_cap=30, info=i4, cache=c2), want)
    assert i4["cache"]["frames_encoded"] == 0 and i4["cache"]["frames_hit"] == 30


def rgb_of(f):
    """the RGB frames the planes of the YuvFrames f convert to, by the existing YuvFrames.to_rgb -> host uint8 [T0, H, W, 3]"""
    from tdc_video_amd import preprocess as pp
    planes, _ = pp.selected_planes(f, None, torch.device("cuda"))
    out = torch.empty(f.shape, dtype=torch.uint8, device="cuda")
    f.to_rgb(planes, out)
    return out.cpu()


def yuv_videos():
    """name -> the same kind of video as YuvFrames in several memories: NV12 8-bit, P010 SDR, P010 PQ"""
    from test_hip_yuv_hdr_inputs import sources as hdr_sources, video as hdr_video
    from test_hip_yuv_hibit_inputs import video as hibit_video
    from test_hip_yuv_inputs import video as nv12_video
    nv12 = nv12_video()[0]
    return {"nv12": {"host": nv12}, "p010": hibit_video("p010")[0], "p010_pq": hdr_sources(*hdr_video(), "p010_pq")}


@pytest.mark.parametrize("kind", ["nv12", "p010", "p010_pq"])
def test_oriented_yuv_equals_the_host_oriented_rgb_its_planes_convert_to(fx, kind):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc, pid = fx["enc"], fx["pid"]
    srcs = yuv_videos()[kind]
    rgb = rgb_of(next(iter(srcs.values())))
    assert tuple(rgb.shape) == (40, 90, 160, 3)
    for rotate, hflip in ORIENTATIONS[:2]:
        upright = torch.from_numpy(oc.orient(rgb.numpy(), rotate, hflip))
        wi = {}
        want = enc.encode_frames(upright, 9, 8, pid, frame_cap=30, info=wi)
        for name, src in srcs.items():
            assert pp.is_yuv_frames(src) and (kind != "p010_pq" or src.transfer == "pq")
            gi = {}
            got = enc.encode_frames(pp.Oriented(src, rotate, hflip), 9, 8, pid, frame_cap=30, info=gi)
            assert torch.equal(got, want) and gi == wi and gi["frames_resized"] == 30, (kind, name, rotate, hflip)
    i1, i2 = {}, {}
    src = next(iter(srcs.values()))
    assert torch.equal(enc.encode_frames(pp.Oriented.exif(src[3:4], 8), None, 8, None, image=True, info=i1),
                       enc.encode_frames(torch.from_numpy(oc.orient(rgb[3:4].numpy(), 270, False)), None, 8, None, image=True, info=i2))
    assert i1 == i2


def test_mixin_oriented_inputs_equal_the_host_oriented_call(fx):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    stored, upright = stored_and_upright(90, False)
    lm = loaded_lm(fx["W"], fx["o"], tdc_frame_cap=30)
    ids = torch.from_numpy(fx["o"]["input_ids"])
    lm.get_model().tdc_engine().frame_towers = towers()
    lm.get_model().config.tdc_frame_inputs = True
    want = _call(lm, ids, [[upright], None], (160, 90), [fx["pid"]])
    _same(_call(lm, ids, [[pp.Oriented(stored, 90)], None], (160, 90), [fx["pid"]]), want)
    _same(_call(lm, ids, [[pp.Oriented(stored.cuda(), 90)], [None]], (160, 90), [fx["pid"]]), want)
    want_im = _call(lm, ids, [upright[:2], None], (160, 90), [fx["pid"]] * 2, 2)             # single images: sliced per sample
    _same(_call(lm, ids, [pp.Oriented(stored[:2], 90), None], (160, 90), [fx["pid"]] * 2, 2), want_im)
