"""GPU (-m gpu): encode from channel-first, BGR, RGBA and gray frames.  tdc_pack_rgb against the numpy
restatement of the layouts (pixel_cases) - the shapes where grouping can go wrong, every form, its memory contract, offsets
past 2^32 and its refusals - and the frames funnel on the tiny fixture engine of test_hip_frame_inputs: everything behind the
pack is the frames path that exists, so every comparison is bit for bit against the same call on the [T0, H, W, 3] frames a
host converted beforehand.

The forms.  A word form needs W % 4 == 0 - of SHAPES (2, 4), (4, 8), (5, 64) and (6, 68) - dst and the source pointer on a
multiple of 4 (OFFSETS (0, 0); every other pair takes the BYTE form) and row and frame strides that are multiples of 4 (the
dense view and the pitch rounded up to 8; the pitch of W * ps + 5 forces the BYTE form).  Then
    chw rgb / bgr / rgba, gray of either layout, hwc l     PLANAR: three loads (rgba: plane 3 is not touched), gray one load
    hwc bgr                                                INTER3
    hwc rgba / bgra / argb / abgr / rgbx                   INTER4 as one 16-byte load (the strides are multiples of 16 too);
                                                           the crop's base is 4 bytes past a multiple of 16: four words
    hwc la (pixel stride 2), the crops of chw and hwc bgr (their base is 1 or 3 bytes off), every other shape: BYTE."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import memcheck
import pixel_cases as pc
import test_hip_memory_contract as contract
import test_hip_orient_inputs as hoi
from test_hip_boundary import loaded_lm
from test_hip_frame_inputs import R, _call, _same, frames_of, fx, reference_pixels, towers  # noqa: F401  (fx: the engine fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (2, 4), (5, 1), (3, 5), (4, 8), (7, 37), (5, 64), (6, 68)]      # single pixels, rows shorter than a group,
#                                                                exact groups, ragged tails, more than one workgroup row of groups
SOURCES = [("chw", "rgb"), ("chw", "bgr"), ("chw", "rgba"), ("chw", "l"),
           ("hwc", "bgr"), ("hwc", "rgba"), ("hwc", "bgra"), ("hwc", "argb"), ("hwc", "abgr"), ("hwc", "rgbx"), ("hwc", "l"), ("hwc", "la")]
OFFSETS = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3)]      # (src, dst) pointers modulo 4
BAND = 64


def views(W, ps):
    """name -> random_source's pitch / crop: dense, a pitch that forces bytes, a pitch that keeps words, a top-left crop"""
    return {"dense": dict(), "pitch+5": dict(pitch=5), "pitch8": dict(pitch=-(W * ps) % 8), "crop": dict(crop=(1, 1, 0, 0))}


def on_device(buf, view, so, pattern):
    """the host buffer `buf` copied so (+ a band) bytes into a device allocation that holds `pattern` around it, and `view`
    (a view into buf) as the same view of the device copy"""
    held = torch.full((BAND + so + buf.size + 3 + BAND,), pattern, dtype=torch.uint8, device="cuda")
    held[BAND + so:BAND + so + buf.size] = torch.from_numpy(buf).cuda()
    at = view.__array_interface__["data"][0] - buf.__array_interface__["data"][0]
    dev = held.as_strided(view.shape, view.strides, BAND + so + at)
    assert dev.data_ptr() % 4 == (so + at) % 4
    return dev


def window(view):
    """the bytes from a numpy view's first element to its last as a flat numpy view of the same memory"""
    n = sum((d - 1) * st for d, st in zip(view.shape, view.strides)) + 1
    return np.lib.stride_tricks.as_strided(view, (n,), (1,))


def device_copy(view, pattern=0x5A):
    """a numpy view - pitch and all - as the same view of a device copy of its window, `pattern` around it"""
    return on_device(window(view), view, 0, pattern)


def pinned_copy(view):
    flat = torch.from_numpy(window(view).copy()).pin_memory()
    return flat.as_strided(view.shape, view.strides, 0)


# ---------------------------------------------------------------------------------------------------- the kernel
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  tdc_pack_rgb's is the function below: it is entered there
# under its own name (not a test_ name: that module collects nothing new).
@contract.covers("tdc_pack_rgb")
def pack_rgb_memory_contract(T, H, W, sources=SOURCES, offsets=OFFSETS):
    """tdc_pack_rgb for every source layout over four views, from src / dst pointers 0 .. 3 bytes into larger allocations
    (every form): dst in a guarded arena - nothing outside its 3 T H W bytes changes; the source's samples between poisoned
    bytes - its ignored channels, pitch padding, cropped-away pixels and surroundings hold 0x00, then 0xFF - and the output is
    the restatement's either way."""
    from tdc_video_amd import preprocess as pp
    n = 3 * T * H * W
    for layout, order in sources:
        for name, kw in views(W, len(order) if layout == "hwc" else 1).items():
            for pattern in memcheck.PATTERNS:
                buf, view = pc.random_source(T, H, W, layout, order, junk=pattern, **kw)
                want = torch.from_numpy(pc.to_rgb(view, layout, order)).cuda()
                for so, do in offsets:
                    src = pp.RgbFrames(on_device(buf, view, so, pattern), layout, order)
                    room, arena = memcheck.guarded((n + 3,), torch.uint8, "cuda", BAND, BAND, fill=pattern)
                    written = torch.zeros(n + 3, dtype=torch.bool)
                    written[do:do + n] = True
                    dst = room[do:do + n].view(T, H, W, 3)
                    assert dst.data_ptr() % 4 == do
                    src.pack(dst)
                    torch.cuda.synchronize()
                    memcheck.assert_untouched(arena, written)
                    assert torch.equal(dst, want), (T, H, W, layout, order, name, so, do, pattern)


contract.pack_rgb_memory_contract = pack_rgb_memory_contract


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_every_source_every_form_inside_guards_and_poison(H, W, T):
    pack_rgb_memory_contract(T, H, W)


def test_ops_allocates_the_packed_frames_and_takes_every_order():
    from tdc_video_amd import ops, preprocess as pp
    for layout in pc.LAYOUTS:
        for order in pc.ORDERS:
            _, view = pc.random_source(2, 6, 8, layout, order, pitch=4)
            r = pp.RgbFrames(torch.from_numpy(view).cuda(), layout, order)
            _, fs, rs, ps, chan = r.descriptor()
            got = ops.pack_rgb(r.data, fs, rs, ps, chan, 2, 6, 8)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 6, 8, 3) and got.is_contiguous()
            assert torch.equal(got.cpu(), torch.from_numpy(pc.to_rgb(view, layout, order))), (layout, order)


def test_offsets_past_2_to_the_32():
    """one uninitialised buffer of 2^32 + 2^20 bytes; only the described bytes are filled.  BGRA: two frames whose second
    starts past 2^32 (a 16-byte, a 4-byte and a byte frame stride: the three interleaved-4 forms at W = 12 and 16, bytes at
    W = 9); planar: the B plane 2^32 + 128 past the R plane (bytes at W = 9, words at 12 and 16)."""
    from tdc_video_amd import preprocess as pp
    big = torch.empty((1 << 32) + (1 << 20), dtype=torch.uint8, device="cuda")
    for W in (9, 12, 16):
        data = torch.from_numpy(np.random.RandomState(W).randint(0, 256, (2, 5, W, 4)).astype(np.uint8))
        want = torch.from_numpy(pc.to_rgb(data.numpy(), "hwc", "bgra"))
        for fs in ((1 << 32) + 48, (1 << 32) + 52, (1 << 32) + 49):
            src = big.as_strided((2, 5, W, 4), (fs, 4 * W, 4, 1), 16)
            src.copy_(data)
            out = torch.zeros((2, 5, W, 3), dtype=torch.uint8, device="cuda")
            pp.RgbFrames(src, "hwc", "bgra").pack(out)
            assert torch.equal(out.cpu(), want), (W, fs)
        P = (1 << 31) + 64
        data = torch.from_numpy(np.random.RandomState(W + 1).randint(0, 256, (2, 3, 5, W)).astype(np.uint8))
        src = big.as_strided((2, 3, 5, W), (128, P, W, 1), 0)           # 128 >= 5 W: the frames of a plane do not overlap
        src.copy_(data)
        out = torch.zeros((2, 5, W, 3), dtype=torch.uint8, device="cuda")
        r = pp.RgbFrames(src, "chw", "rgb")
        assert r.descriptor()[4] == (0, P, 2 * P) and 2 * P > 1 << 32
        r.pack(out)
        assert torch.equal(out.cpu(), torch.from_numpy(pc.to_rgb(data.numpy(), "chw", "rgb"))), W
    del big, src
    torch.cuda.empty_cache()


def test_badarg_before_any_launch():
    from tdc_video_amd import lib as L
    lib = L.load()
    T, H, W = 2, 4, 6
    n, ns = T * H * W * 3, T * H * W * 4                    # dst bytes; the bytes of a dense BGRA source
    room = torch.from_numpy(np.random.RandomState(0).randint(0, 256, 1024).astype(np.uint8)).cuda()
    before = room.clone()
    sp = room.data_ptr() + 400                              # the source lies at [400, 400 + ns) of room
    out, arena = memcheck.guarded((n,), torch.uint8, "cuda", 64, 64)
    dense = dict(fs=H * W * 4, rs=W * 4, ps=4, chan=(2, 1, 0))

    def rc(src=sp, dims=(T, H, W), dst=out.data_ptr(), null=False, **kw):
        d = dict(dense, **kw)
        s = L.RgbSource(src, d["fs"], d["rs"], d["ps"], (C.c_longlong * 3)(*d["chan"]))
        return lib.tdc_pack_rgb(None if null else C.byref(s), *dims, C.c_void_p(dst), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [rc(null=True), rc(src=0), rc(dst=0)]
    for i in range(3):
        for v in (0, -1, 65536):
            dims = [T, H, W]
            dims[i] = v
            bad.append(rc(dims=tuple(dims)))
    for v in (-1, (1 << 40) + 1, -(1 << 62)):
        bad += [rc(fs=v), rc(rs=v), rc(ps=v), rc(chan=(v, 1, 0)), rc(chan=(2, v, 0)), rc(chan=(2, 1, v))]
    # dst [0, n) overlapping the source extent [sp, sp + ns)
    bad += [rc(dst=sp), rc(dst=sp + 1), rc(dst=sp + ns - 1), rc(dst=sp - n + 1), rc(dst=sp - 1)]
    bad += [rc(dst=sp - n + 2, chan=(1, 2, 3)),             # ARGB: the extent starts at src + min(chan) = src + 1
            rc(dst=sp + T * H * W * 2 - 2, fs=H * W * 2, rs=W * 2, ps=2, chan=(0, 0, 0))]      # LA: it ends with the last L sample
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad      # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(n, dtype=torch.bool))
    assert torch.equal(room, before)                                   # and nothing was written into the refused dst ranges
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_pack_rgb")
    # the limits themselves are taken: a stride that no address is formed with may be 2^40
    assert rc(dims=(1, H, W), fs=1 << 40) == 0 and rc(dims=(T, 1, W), rs=1 << 40, fs=W * 4) == 0
    # ranges that touch without overlapping are taken, on either side
    assert rc(dst=sp + ns) == 0 and rc(dst=sp - n) == 0
    assert rc(dst=sp - n + 1, chan=(1, 2, 3)) == 0                     # ends on ARGB's first ignored byte
    assert rc(dst=sp + T * H * W * 2 - 1, fs=H * W * 2, rs=W * 2, ps=2, chan=(0, 0, 0)) == 0      # starts on LA's last ignored byte
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- preprocess_selected
IDX = [0, 2, 3, 5, 8, 9, 10, 13, 14, 15]          # 10 of 16: 7 + 3 at slab 7
KINDS = {"chw/rgb": ("chw", "rgb", 3), "hwc/bgr": ("hwc", "bgr", 3), "hwc/bgra": ("hwc", "bgra", 4), "gray": ("hwc", "l", 1)}


def stored_as(rgb, kind, pitch=None, junk=None):
    """host RGB frames uint8 [T0, H, W, 3] (numpy) -> a numpy view in the layout of `kind` that stands for them (gray: for
    their G channel replicated); hwc/bgra is pitched (W * 4 + 12 bytes per row), its alpha and padding random or `junk`"""
    layout, order, _ = KINDS[kind]
    T0, H, W, _ = rgb.shape
    if kind == "gray":
        return np.ascontiguousarray(rgb[..., 1])
    _, view = pc.random_source(T0, H, W, layout, order, pitch=(12 if kind == "hwc/bgra" else 0) if pitch is None else pitch, junk=junk)
    for c, i in enumerate(pc.channel_index(order)):
        (view[..., i] if layout == "hwc" else view[:, i])[...] = rgb[..., c]
    return view


def wrap(pp, kind, data):
    layout, order, _ = KINDS[kind]
    return pp.RgbFrames(data, layout, order)


@functools.lru_cache(maxsize=None)
def stored_and_plain(kind, H=90, W=160, T0=40):
    """a video of T0 frames as stored (numpy view), and the contiguous [T0, H, W, 3] frames a host converts it to beforehand"""
    layout, order, _ = KINDS[kind]
    stored = stored_as(frames_of(H, W, T0).numpy(), kind)
    return stored, torch.from_numpy(pc.to_rgb(stored, layout, order))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("H,W", [(90, 160), (45, 81)])
def test_preprocess_selected_on_rgb_frames_equals_process_images_of_the_converted_frames(H, W, kind):
    from tdc_video_amd import preprocess as pp
    stored, plain = stored_and_plain(kind, H, W, 16)
    per_pixel = KINDS[kind][2]
    host, pinned = torch.from_numpy(stored), pinned_copy(stored)
    sources = {"cuda": device_copy(stored), "pageable": host, "pinned": pinned, "numpy": stored}
    assert pinned.is_pinned() and pinned.stride() == host.stride() and sources["cuda"].stride() == host.stride()
    want = reference_pixels(plain[IDX])
    for name, src in sources.items():
        for slab in (1, 7, 64):
            stats = {}
            got = pp.preprocess_selected(wrap(pp, kind, src), IDX, towers(), torch.float16, slab, stats=stats)
            assert len(got) == 2
            for g, w in zip(got, want):
                assert g.is_cuda and g.dtype == torch.float16 and tuple(g.shape) == (10, 3, R, R) and memcheck.same_bits(g, w), (name, slab)
            assert stats == dict(frames_in=16, frames_resized=10, bytes_uploaded=0 if name == "cuda" else 10 * H * W * per_pixel)
    # idx=None, bfloat16: the device view is read in place through its strides, host data is staged dense or uploaded as it lies
    want = reference_pixels(plain, torch.bfloat16)
    for name, src in sources.items():
        stats = {}
        got = pp.preprocess_selected(wrap(pp, kind, src), None, towers(), torch.bfloat16, 7, stats=stats)
        assert all(memcheck.same_bits(g, w) for g, w in zip(got, want)), name
        assert stats == dict(frames_in=16, frames_resized=16, bytes_uploaded=0 if name == "cuda" else 16 * H * W * per_pixel)


def test_preprocess_selected_on_rgb_frames_memory_contract(monkeypatch):
    """outputs in guarded arenas, every scratch allocated through torch.empty and guarded, dropped frames, alpha and pitch
    padding holding 0x00, then 0xFF: bit-identical outputs, nothing written outside out[0:len(idx)] or outside a scratch"""
    import importlib
    pp = importlib.import_module("tdc_video_amd.preprocess")      # under the name memcheck.poison_empty looks for
    H, W = 90, 160
    rgb = frames_of(H, W)[:16].numpy()
    want = reference_pixels(torch.from_numpy(rgb[IDX]))
    T = len(IDX)
    results = []
    for pattern in memcheck.PATTERNS:
        stored = stored_as(rgb, "hwc/bgra", junk=pattern)
        dropped = [t for t in range(16) if t not in IDX]
        stored[dropped] = pattern
        for src in (device_copy(stored, pattern), stored):
            outs = [memcheck.guarded((T + 2, 3, R, R), torch.float16, "cuda", 1, 1) for _ in range(2)]
            with monkeypatch.context() as mp:
                inner = memcheck.poison_empty(mp, pattern, guard_bytes=4096)
                got = pp.preprocess_selected(pp.RgbFrames(src, "hwc", "bgra"), IDX, towers(), torch.float16, 3, out=[v for v, _ in outs])
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
    assert all(memcheck.same_bits(a, b) for r in results[1:] for a, b in zip(results[0], r))


# ---------------------------------------------------------------------------------------------------- the launch trace
class _Traced(hoi._Traced):
    """test_hip_orient_inputs' logged library, with tdc_pack_rgb's T, H, W logged too"""
    SIZES = dict(hoi._Traced.SIZES, tdc_pack_rgb=slice(1, 4))


def test_launch_trace(fx, monkeypatch):  # noqa: F811
    from tdc_video_amd import lib as L, preprocess as pp
    plain = frames_of(90, 160)[:16].clone().pin_memory()
    log = []
    monkeypatch.setattr(L, "_lib", _Traced(L.load(), log))

    def trace(src, slab=4):
        del log[:]
        stats = {}
        pp.preprocess_selected(src, IDX, towers(), torch.float16, slab, stats=stats)
        return list(log), stats

    base, base_stats = trace(plain)
    assert sum(c[0] == "tdc_preprocess_frames" for c in base) == 6 and not any(c[0] == "tdc_pack_rgb" for c in base)
    # the identity: exactly the calls the wrapped tensor issues, in their order
    assert trace(pp.RgbFrames(plain)) == (base, base_stats) and trace(pp.RgbFrames(plain, "hwc", "RGB")) == (base, base_stats)
    launches = ("tdc_pack_rgb", "tdc_orient_frames", "tdc_preprocess_frames")
    for kind in KINDS:
        src = wrap(pp, kind, stored_as(plain.numpy(), kind))
        got, stats = trace(src)
        packs = [c for c in got if c[0] == "tdc_pack_rgb"]
        assert packs == [("tdc_pack_rgb", n, 90, 160) for n in (4, 4, 2)], kind      # one per slab of 10 kept frames
        # the tower-outer loop becomes slab-outer: the same calls in another order
        assert sorted(c for c in got if c[0] != "tdc_pack_rgb") == sorted(base)
        assert stats == dict(base_stats, bytes_uploaded=10 * 90 * 160 * KINDS[kind][2])
        # every slab is packed before the towers read it
        assert [c[0] for c in got if c[0] in launches] == ["tdc_pack_rgb", "tdc_preprocess_frames", "tdc_preprocess_frames"] * 3
        # inside an Oriented: pack, then orient, then the two resizes, per slab
        got, _ = trace(pp.Oriented(src, 90))
        assert [c[0] for c in got if c[0] in launches] == ["tdc_pack_rgb", "tdc_orient_frames", "tdc_preprocess_frames",
                                                           "tdc_preprocess_frames"] * 3
        assert [c for c in got if c[0] == "tdc_orient_frames"] == [("tdc_orient_frames", n, 90, 160, 1, 0) for n in (4, 4, 2)]
    # an Oriented around the identity RgbFrames: the calls of an Oriented around the tensor
    assert trace(pp.Oriented(pp.RgbFrames(plain), 90)) == trace(pp.Oriented(plain, 90))
    # through the engine: the identity wrapper changes no call of a whole encode either
    enc, pid = fx["enc"], fx["pid"]
    video = frames_of(90, 160)
    del log[:]
    a = enc.encode_frames(video, 9, 8, pid, frame_cap=30)
    want = list(log)
    del log[:]
    b = enc.encode_frames(pp.RgbFrames(video), 9, 8, pid, frame_cap=30)
    assert log == want and len(want) > 10 and torch.equal(a, b)


def test_oriented_rgb_frames_equal_the_host_converted_and_rotated_frames():
    import orient_cases as oc
    from tdc_video_amd import preprocess as pp
    for kind in ("chw/rgb", "hwc/bgra"):
        stored, plain = stored_and_plain(kind, 45, 81, 16)
        want = reference_pixels(torch.from_numpy(oc.orient(plain.numpy()[IDX], 270, True)))
        for src in (stored, torch.from_numpy(stored).cuda()):
            got = pp.preprocess_selected(pp.Oriented(wrap(pp, kind, src), 270, True), IDX, towers(), torch.float16, 7)
            assert all(memcheck.same_bits(g, w) for g, w in zip(got, want)), kind


# ---------------------------------------------------------------------------------------------------- the engine
ENGINE_KINDS = ["chw/rgb", "hwc/bgra", "gray"]


@pytest.mark.parametrize("kind", ENGINE_KINDS)
def test_encode_frames_prompts_export_and_image(fx, kind):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc, pid = fx["enc"], fx["pid"]
    stored, plain = stored_and_plain(kind)
    wi = {}
    want = enc.encode_frames(plain, 9, 8, pid, frame_cap=30, info=wi)                  # T0 = 40 above the cap: a1 sub-samples
    assert wi["frames_resized"] == 30 == len(wi["frame_indices"])
    for src in (torch.from_numpy(stored), torch.from_numpy(stored).cuda(), stored):    # host, device, numpy: the same bits
        gi = {}
        got = enc.encode_frames(wrap(pp, kind, src), 9, 8, pid, frame_cap=30, info=gi)
        assert torch.equal(got, want) and gi == wi
    r = wrap(pp, kind, stored)
    assert torch.equal(enc.encode_frames(r, 9, 8, pid), enc.encode_frames(plain, 9, 8, pid))          # every frame kept
    assert torch.equal(enc.encode_frames(wrap(pp, kind, torch.from_numpy(stored).cuda()), 9, 8, pid), enc.encode_frames(plain, 9, 8, pid))
    qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid),
          dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:])]
    i1, i2 = [{} for _ in qs], [{} for _ in qs]
    for a, b in zip(enc.encode_frames_prompts(r, qs, frame_cap=30, pad_fraction=1.0, infos=i1),
                    enc.encode_frames_prompts(plain, qs, frame_cap=30, pad_fraction=1.0, infos=i2)):
        assert torch.equal(a, b)
    assert i1 == i2
    for store in ("f16", "e4m3"):
        w = enc.export_features_from_frames(plain, store=store, slab=16)
        g = enc.export_features_from_frames(r, store=store, slab=16)
        assert g.signature == w.signature and g.image_size == w.image_size == (90, 160) and g.frames == 40
        assert memcheck.same_bits(g.siglip, w.siglip) and memcheck.same_bits(g.dino, w.dino)
        if store == "e4m3":
            assert torch.equal(g.siglip_scale, w.siglip_scale) and torch.equal(g.dino_scale, w.dino_scale) and torch.equal(g.sims, w.sims)
    # the image form
    for src in (stored, torch.from_numpy(stored).cuda()):
        i1, i2 = {}, {}
        got = enc.encode_frames(wrap(pp, kind, src)[3:4], None, 8, None, image=True, info=i1)
        assert torch.equal(got, enc.encode_frames(plain[3:4], None, 8, None, image=True, info=i2)) and i1 == i2
        assert i1["frames_in"] == i1["frames_resized"] == 1


@pytest.mark.parametrize("kind", ENGINE_KINDS)
def test_frame_cache_hits_whichever_way_the_video_was_first_asked(fx, kind):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    enc, pid = fx["enc"], fx["pid"]
    stored, plain = stored_and_plain(kind)
    r = wrap(pp, kind, stored)
    want = enc.encode_frames(plain, 9, 8, pid, frame_cap=30)
    c = enc.new_cache(1 << 30)
    i1, i2, i3, i4, i5 = {}, {}, {}, {}, {}
    assert torch.equal(enc.encode_frames(r, 9, 8, pid, frame_cap=30, info=i1, cache=c), want)
    assert i1["cache"]["frames_encoded"] == 30
    assert torch.equal(enc.encode_frames(r, 9, 8, pid, frame_cap=30, info=i2, cache=c), want)      # the second question hits
    assert i2["cache"]["frames_encoded"] == 0 and i2["cache"]["frames_hit"] == i2["cache"]["frames"] == 30
    assert torch.equal(enc.encode_frames(plain, 9, 8, pid, frame_cap=30, info=i5, cache=c), want)  # and so do the plain RGB frames
    assert i5["cache"]["frames_encoded"] == 0 and i5["cache"]["frames_hit"] == 30
    # first asked through plain RGB frames, then through the wrapper: all hits
    c2 = enc.new_cache(1 << 30)
    assert torch.equal(enc.encode_frames(plain, 9, 8, pid, frame_cap=30, info=i3, cache=c2), want)
    assert i3["cache"]["frames_encoded"] == 30
    assert torch.equal(enc.encode_frames(r, 9, 8, pid, frame_cap=30, info=i4, cache=c2), want)
    assert i4["cache"]["frames_encoded"] == 0 and i4["cache"]["frames_hit"] == 30


def test_mixin_rgb_frames_inputs_equal_the_host_converted_call(fx):  # noqa: F811
    from tdc_video_amd import preprocess as pp
    lm = loaded_lm(fx["W"], fx["o"], tdc_frame_cap=30)
    ids = torch.from_numpy(fx["o"]["input_ids"])
    lm.get_model().tdc_engine().frame_towers = towers()
    lm.get_model().config.tdc_frame_inputs = True
    for kind in ("chw/rgb", "hwc/bgra"):
        stored, plain = stored_and_plain(kind)
        want = _call(lm, ids, [[plain], None], (90, 160), [fx["pid"]])
        _same(_call(lm, ids, [[wrap(pp, kind, stored)], None], (90, 160), [fx["pid"]]), want)                  # a video entry
        _same(_call(lm, ids, [[wrap(pp, kind, torch.from_numpy(stored).cuda())], [None]], (90, 160), [fx["pid"]]), want)
        want_im = _call(lm, ids, [plain[:2], None], (90, 160), [fx["pid"]] * 2, 2)                             # single images: sliced per sample
        _same(_call(lm, ids, [wrap(pp, kind, stored[:2]), None], (90, 160), [fx["pid"]] * 2, 2), want_im)
    stored, _ = stored_and_plain("chw/rgb")
    for other, v in (("tdc_shard_frames", True), ("tdc_batch_frames", 512), ("tdc_batch_prompts", 4)):
        setattr(lm.get_model().config, other, v)
        with pytest.raises(ValueError, match=other):
            _call(lm, ids, [[wrap(pp, "chw/rgb", stored)], None], (90, 160), [fx["pid"]])
        setattr(lm.get_model().config, other, None)
