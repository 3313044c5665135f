"""CPU: encode from channel-first, BGR, RGBA and gray frames.  The numpy restatement of the layouts
(tests/pixel_cases.py, written from the index formula) against Pillow's .convert("RGB") and numpy fancy indexing, the host
logic of preprocess.RgbFrames - its descriptor from strides alone, slicing, recognition, refusals, the host gather - and the
frames funnel (encode.FrameSource) taking an RgbFrames where it takes frames, on the engine double of test_frame_inputs."""
import importlib

import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
import pixel_cases as pc
from tdc_video_amd import encode, preprocess
from test_features import FeatureEngine, Untouchable, feature_lm
from test_frame_inputs import _Frames, call, make_frames

RgbFrames = preprocess.RgbFrames


def storage_bytes(t):
    """the whole storage under a host tensor as a flat numpy uint8 array"""
    return torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage()).numpy()


# ------------------------------------------------------------------------------------------------ the definition
def test_restatement_equals_pillow_convert_rgb():
    from PIL import Image
    rng = np.random.RandomState(0)
    for mode, order in (("L", "l"), ("LA", "la"), ("RGB", "rgb"), ("RGBA", "rgba")):
        a = rng.randint(0, 256, (5, 7, len(order))).astype(np.uint8)
        want = np.asarray(Image.fromarray(a[..., 0] if mode == "L" else a, mode).convert("RGB"))      # alpha dropped, gray replicated
        got = pc.to_rgb(a[None], "hwc", order)
        assert got.shape == (1, 5, 7, 3) and got.flags["C_CONTIGUOUS"] and np.array_equal(got[0], want), mode
    g = rng.randint(0, 256, (2, 5, 7)).astype(np.uint8)               # a 3-D array is one gray channel under either layout
    for layout in pc.LAYOUTS:
        assert np.array_equal(pc.to_rgb(g, layout, "l"), np.stack([g] * 3, -1))


@pytest.mark.parametrize("order", pc.ORDERS)
def test_restatement_equals_numpy_fancy_indexing(order):
    C = len(order)
    a = np.random.RandomState(C).randint(0, 256, (3, 5, 7, C)).astype(np.uint8)
    pick = [order.index("l")] * 3 if "l" in order else [order.index(ch) for ch in "rgb"]
    assert np.array_equal(pc.to_rgb(a, "hwc", order), a[..., pick])
    assert np.array_equal(pc.to_rgb(a.transpose(0, 3, 1, 2), "chw", order), a[..., pick])
    assert np.array_equal(pc.to_rgb(a, "hwc", order.upper()), a[..., pick])
    if order == "bgr":
        assert np.array_equal(pc.to_rgb(a, "hwc", order), a[..., ::-1])
    if order == "rgba":
        assert np.array_equal(pc.to_rgb(a, "hwc", order), a[..., :3])
    assert preprocess.channel_order(order, C) == tuple(pick) == pc.channel_index(order)


# ------------------------------------------------------------------------------------------------ the descriptor
VIEWS = [dict(), dict(pitch=5), dict(pitch=3, crop=(1, 1, 0, 0)), dict(crop=(2, 3, 1, 2)), dict(pitch=8, crop=(0, 2, 3, 0))]


def addressed(r):
    """the bytes a descriptor names inside the storage under r.data -> [T, H, W, 3]"""
    base, fs, rs, ps, chan = r.descriptor()
    assert all(isinstance(v, int) and v >= 0 for v in (base, fs, rs, ps) + chan) and isinstance(chan, tuple) and len(chan) == 3
    T, H, W, _ = r.shape
    t, y, x, c = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    return storage_bytes(r.data)[base + t * fs + y * rs + x * ps + np.array(chan)[c]]


@pytest.mark.parametrize("layout", pc.LAYOUTS)
@pytest.mark.parametrize("order", pc.ORDERS)
def test_descriptor_addresses_the_restatements_bytes(layout, order):
    for kw in VIEWS:
        buf, view = pc.random_source(4, 3, 5, layout, order, **kw)
        want = pc.to_rgb(view, layout, order)
        for src in (view, torch.from_numpy(buf).as_strided(view.shape, view.strides,
                                                           view.__array_interface__["data"][0] - buf.__array_interface__["data"][0])):
            r = RgbFrames(src, layout, order)
            assert r.shape == (4, 3, 5, 3) and np.array_equal(addressed(r), want), kw
            assert np.array_equal(addressed(r[1:3]), want[1:3]) and r[1:3].shape == (2, 3, 5, 3)      # a slice of frames
            if torch.is_tensor(src):
                assert r.descriptor()[0] == src.storage_offset() and r.data.data_ptr() == src.data_ptr()       # not copied
    d = RgbFrames(np.zeros((4, 6, 10, 4), np.uint8), "hwc", "bgra").descriptor()
    assert d == (0, 240, 40, 4, (2, 1, 0))
    d = RgbFrames.chw(np.zeros((4, 3, 6, 10), np.uint8), "bgr").descriptor()
    assert d == (0, 180, 10, 1, (120, 60, 0))
    assert RgbFrames(np.zeros((4, 6, 10, 4), np.uint8), "hwc", "argb").descriptor()[3:] == (4, (1, 2, 3))
    assert RgbFrames(np.zeros((4, 6, 10, 2), np.uint8), "hwc", "la").descriptor()[3:] == (2, (0, 0, 0))


def test_gray_planes_under_either_layout():
    g = np.random.RandomState(3).randint(0, 256, (4, 3, 5)).astype(np.uint8)
    want = np.stack([g] * 3, -1)
    for r in (RgbFrames.gray(g), RgbFrames(g, "hwc", "l"), RgbFrames(g, "chw", "l"), RgbFrames(g[:, None], "chw", "L"),
              RgbFrames(g[..., None], "hwc", "l"), RgbFrames.gray(torch.from_numpy(g))):
        assert r.shape == (4, 3, 5, 3) and r.is_gray and np.array_equal(addressed(r), want)
        assert r.descriptor()[1:] == (15, 5, 1, (0, 0, 0))
    with pytest.raises(ValueError, match="order"):
        RgbFrames(g)                                                 # one stored channel is not "rgb"


# ------------------------------------------------------------------------------------------------ the container
def test_shape_slicing_and_recognition():
    _, view = pc.random_source(6, 4, 6, "chw", "rgb")
    t = torch.from_numpy(view)
    r = RgbFrames.chw(t)
    assert r.shape == (6, 4, 6, 3) and r.data.data_ptr() == t.data_ptr() and not r.is_cuda and not r.is_identity
    assert (r.layout, r.order, r.index) == ("chw", "rgb", (0, 1, 2))
    s = r[2:5]
    assert s.shape == (3, 4, 6, 3) and s.data.data_ptr() == t[2:5].data_ptr() and (s.layout, s.order) == ("chw", "rgb")
    assert r[1:2].shape[0] == 1
    assert encode.frames_size(r) == (6, (4, 6)) and encode.FrameSource(r).image_size == (4, 6)
    with pytest.raises(TypeError, match="slice"):
        r[0]
    with pytest.raises(TypeError, match="slice"):
        r[::2]
    assert RgbFrames(view, "chw").data.data_ptr() == view.__array_interface__["data"][0]        # a numpy array, not copied either
    assert preprocess.is_rgb_frames(r) and not preprocess.is_oriented(r) and not preprocess.is_yuv_frames(r)
    assert not preprocess.is_rgb_frames(t) and not preprocess.is_rgb_frames(view)
    hwc = np.ascontiguousarray(view.transpose(0, 2, 3, 1))
    assert RgbFrames(hwc).is_identity and RgbFrames(hwc, "hwc", "RGB").is_identity and not RgbFrames(hwc, "hwc", "bgr").is_identity
    o = preprocess.Oriented(r, 90, True)                              # an Oriented goes around an RgbFrames
    assert o.shape == (6, 6, 4, 3) and o.frames is r and o[1:3].frames.shape == (2, 4, 6, 3)
    assert preprocess.is_oriented(o) and not preprocess.is_rgb_frames(o)
    other = importlib.import_module("tdc_video_amd.preprocess")       # the class made under the package's second name
    for made_by, asked in ((other, preprocess), (preprocess, other)):
        x = made_by.RgbFrames(view, "chw", "bgr")
        assert asked.is_rgb_frames(x) and not asked.is_oriented(x) and not asked.is_yuv_frames(x)
        with pytest.raises(ValueError, match="RgbFrames"):
            asked.RgbFrames(x)


def test_refusals():
    a = np.zeros((2, 4, 6, 3), np.uint8)
    for bad in (a.astype(np.int16), a.astype(np.float32), torch.zeros(2, 4, 6, 3), torch.zeros(2, 4, 6, 3, dtype=torch.int16)):
        with pytest.raises(ValueError, match="uint8"):
            RgbFrames(bad)
    for bad in (a[0, 0], a[None], np.zeros((0, 4, 6, 3), np.uint8), np.zeros((2, 4, 0, 3), np.uint8), [a[0], a[1]], None):
        with pytest.raises(ValueError, match="data"):
            RgbFrames(bad)
    for order in ("rg", "rgba", "", "rgbl", "rrg", "rgq", "lll", "rga", None, 3, ("r", "g", "b")):
        with pytest.raises(ValueError, match="order"):
            RgbFrames(a, "hwc", order)
    for C, order in ((4, "rgb"), (4, "rgbb"), (4, "aaxl" + "l"), (4, "lrgb"), (2, "ll"), (2, "ax"), (1, "a"), (1, "r"), (4, "lall")):
        with pytest.raises(ValueError, match="order"):
            RgbFrames(np.zeros((2, 4, 6, C), np.uint8), "hwc", order)
    with pytest.raises(ValueError, match="order"):
        RgbFrames(np.zeros((2, 4, 6, 5), np.uint8), "hwc", "rgbax")    # 1 to 4 stored channels
    with pytest.raises(ValueError, match="order"):
        RgbFrames(a, "chw", "rgb")                                    # read as [T0, C = 4, H, W]: three letters for four planes
    for layout in ("HWC", "nchw", None, 0):
        with pytest.raises(ValueError, match="layout"):
            RgbFrames(a, layout)
    for flipped in (a[:, ::-1], a[:, :, ::-1], a[::-1], a[..., ::-1]):
        with pytest.raises(ValueError, match="negative stride"):
            RgbFrames(flipped, "hwc", "rgb")                          # refused, not silently copied
    with pytest.raises(ValueError, match="RgbFrames"):
        RgbFrames(RgbFrames(a, "hwc", "bgr"), "hwc", "bgr")
    with pytest.raises(ValueError, match="Oriented"):
        RgbFrames(preprocess.Oriented(a, 90), "hwc", "bgr")
    with pytest.raises(ValueError, match="65535"):
        RgbFrames(np.zeros((1, 1, 65536, 1), np.uint8), "hwc", "l")
    with pytest.raises(ValueError):
        RgbFrames.gray(a)


def test_preprocess_selected_checks_an_rgb_frames_on_the_host_before_any_launch():
    towers = (dict(R=2, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)),) * 2
    _, view = pc.random_source(6, 4, 6, "hwc", "bgra", pitch=4)
    for src in (RgbFrames(view, "hwc", "bgra"), preprocess.Oriented(RgbFrames(view, "hwc", "bgra"), 90)):
        for idx in ([0, 6], [-1, 2], [2, 1], []):
            with pytest.raises(ValueError, match="idx"):
                preprocess.preprocess_selected(src, idx, towers)       # no GPU here: raised before one would be needed
        with pytest.raises(ValueError, match="slab"):
            preprocess.preprocess_selected(src, None, towers, slab=0)
        with pytest.raises(ValueError, match="float16"):
            preprocess.preprocess_selected(src, None, towers, dtype=torch.float32)


def test_c_abi_entry_is_declared():
    import ctypes as C
    from tdc_video_amd import lib, ops
    res, args = lib.SIGNATURES["tdc_pack_rgb"]
    assert res is C.c_int and len(args) == 6 and args[0] is C.POINTER(lib.RgbSource)
    assert [n for n, _ in lib.RgbSource._fields_] == ["src", "frame_stride", "row_stride", "pixel_stride", "chan"]
    assert C.sizeof(lib.RgbSource) == 8 + 3 * 8 + 3 * 8 and callable(ops.pack_rgb)


# ------------------------------------------------------------------------------------------------ the host gather
IDX = [0, 2, 3, 5, 8, 9, 10, 13, 14, 15]          # 10 of 16


@pytest.mark.parametrize("layout,order,per_pixel", [("hwc", "bgra", 4), ("hwc", "argb", 4), ("hwc", "bgr", 3), ("hwc", "la", 2),
                                                    ("chw", "rgb", 3), ("chw", "bgra", 3), ("chw", "xrgb", 3),      # used planes only
                                                    ("hwc", "l", 1), ("chw", "l", 1), ("chw", "al", 1)])
def test_host_gather_stages_the_kept_frames_dense_in_their_own_layout(layout, order, per_pixel):
    T0, H, W = 16, 5, 7
    for kw in (dict(), dict(pitch=5, crop=(1, 2, 1, 0))):
        _, view = pc.random_source(T0, H, W, layout, order, **kw)
        want = pc.to_rgb(view, layout, order)[IDX]
        staged, stage = preprocess.gather_pixels(RgbFrames(view, layout, order), IDX, pin=False)
        assert preprocess.is_rgb_frames(staged) and staged.shape == (10, H, W, 3) and staged.layout == layout
        assert np.array_equal(pc.to_rgb(staged.data.numpy(), staged.layout, staged.order), want)
        assert stage.is_contiguous() and stage.numel() == 10 * H * W * per_pixel            # what bytes_uploaded states
        assert staged.data.untyped_storage().data_ptr() == stage.untyped_storage().data_ptr()
        assert np.array_equal(addressed(staged), want)
        assert np.array_equal(addressed(staged[3:7]), want[3:7])                            # a slab of the staged frames


# ------------------------------------------------------------------------------------------------ refused configs
@pytest.mark.parametrize("other,v", [("tdc_shard_frames", True), ("tdc_batch_frames", 512), ("tdc_batch_prompts", 4)])
def test_sharded_batched_and_multi_prompt_configs_refuse_an_rgb_frames_as_they_refuse_frames(other, v):
    lm = feature_lm(tdc_frame_inputs=True, **{other: v})
    lm.get_model()._tdc_encoder = Untouchable()
    frames = RgbFrames.chw(np.ascontiguousarray(make_frames(30).transpose(0, 3, 1, 2)))
    with pytest.raises(ValueError) as ei:
        call(lm, [[frames], None])
    assert "tdc_frame_inputs" in str(ei.value) and other in str(ei.value)


# ------------------------------------------------------------------------------------------------ the funnel
class _PixelFrames(_Frames):
    """the double's pixels_from_frames on the RGB frames an RgbFrames stands for; records what it was handed"""

    def pixels_from_frames(self, frames, idx=None):
        self.handed = getattr(self, "handed", []) + [frames]
        if preprocess.is_rgb_frames(frames):
            frames = pc.to_rgb(frames.data.numpy(), frames.layout, frames.order)
        return _Frames.pixels_from_frames(self, frames, idx)


class PixelEngine(_PixelFrames, FeatureEngine):
    pass


@pytest.mark.parametrize("layout,order", [("chw", "rgb"), ("hwc", "bgra"), ("hwc", "l")])
def test_frame_source_hands_the_wrapper_and_the_a1_indices_only(layout, order):
    eng = PixelEngine(N=5)
    rgb = make_frames(40)                                             # [40, 4, 6, 3]
    C = len(order)
    stored = np.zeros((40, 4, 6, C), np.uint8)
    for c, i in enumerate(pc.channel_index(order)):
        stored[..., i] = rgb[..., c if "l" not in order else 1]
    if layout == "chw":
        stored = np.ascontiguousarray(stored.transpose(0, 3, 1, 2))
    r = RgbFrames(stored, layout, order)
    plain = pc.to_rgb(stored, layout, order)
    wi, gi = {}, {}
    want = encode.encode_frames_with(eng, plain, 4, 4, [1, 2, 3], frame_cap=30, info=wi)
    eng.asked, eng.handed = [], []
    got = encode.encode_frames_with(eng, r, 4, 4, [1, 2, 3], frame_cap=30, info=gi)
    assert torch.equal(got, want) and gi == wi and gi["frames_in"] == 40 and gi["frames_resized"] == 30
    assert eng.asked == [encode.frame_indices(eng.cfg, 40, 4, 30)] and len(eng.handed) == 1 and eng.handed[0] is r
    i1, i2 = {}, {}                                                   # the image form, through the slice the mixin takes
    assert torch.equal(encode.encode_frames_with(eng, r[3:4], None, 4, None, info=i1, image=True),
                       encode.encode_frames_with(eng, plain[3:4], None, 4, None, info=i2, image=True)) and i1 == i2
    a, b = encode.export_features_from_frames_with(eng, r, slab=16), encode.export_features_from_frames_with(eng, plain, slab=16)
    assert torch.equal(a.siglip, b.siglip) and torch.equal(a.dino, b.dino) and a.frames == 40 and a.image_size == b.image_size == (4, 6)
