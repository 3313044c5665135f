"""CPU: encode from rotated video.  The numpy restatement of the orientation (tests/orient_cases.py,
written from the index formulas) against np.rot90 and reversed slices, the EXIF table against Pillow, the host logic of
preprocess.Oriented, and the frames funnel (encode.FrameSource) taking an Oriented where it takes frames - on the engine
double of test_frame_inputs, whose pixels are the preprocess double's of the upright frames."""
import importlib

import numpy as np
import pytest
import torch

import tdc_video_amd  # noqa: F401
import orient_cases as oc
import yuv_cases as yc
from tdc_video_amd import encode, preprocess
from test_features import FeatureEngine, Untouchable, feature_lm
from test_frame_inputs import _Frames, call, make_frames

Oriented = preprocess.Oriented


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("rotate,hflip", oc.ALL)
def test_restatement_equals_rot90_and_reversed_slices(rotate, hflip):
    S = np.random.RandomState(rotate + hflip).randint(0, 256, (3, 5, 7, 3)).astype(np.uint8)
    want = np.rot90(S, -(rotate // 90), axes=(1, 2))              # k < 0: clockwise
    if hflip:
        want = want[:, :, ::-1]
    got = oc.orient(S, rotate, hflip)
    assert got.shape == (3,) + oc.out_hw(5, 7, rotate) + (3,) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, want)
    if (rotate, hflip) == (180, True):                            # the vertical flip
        assert np.array_equal(got, S[:, ::-1])


def test_the_eight_orientations_are_distinct_and_close_under_composition():
    S = np.arange(2 * 3 * 3).reshape(2, 3, 3).astype(np.uint8)[None]
    outs = [oc.orient(S, r, f) for r, f in oc.ALL]
    flat = [o.tobytes() + bytes(o.shape) for o in outs]
    assert len(set(flat)) == 8
    for o in outs:                                                 # a second orientation lands on one of the eight again
        for r, f in oc.ALL:
            two = oc.orient(o, r, f)
            assert two.tobytes() + bytes(two.shape) in flat


def test_exif_table_equals_pillow():
    from PIL import Image, ImageOps
    assert preprocess.EXIF_ORIENTATIONS == oc.EXIF
    S = np.random.RandomState(1).randint(0, 256, (5, 7, 3)).astype(np.uint8)
    for orientation in range(1, 9):
        im = Image.fromarray(S)
        ex = im.getexif()
        ex[0x0112] = orientation
        im.info["exif"] = ex.tobytes()
        upright = ImageOps.exif_transpose(im)
        want = np.asarray(S if upright is None else upright)
        rotate, hflip = oc.EXIF[orientation]
        assert np.array_equal(oc.orient(S, rotate, hflip), want), orientation
        o = Oriented.exif(S[None], orientation)
        assert (o.rotate, o.hflip) == (rotate, hflip) and o.shape == (1,) + want.shape


# ------------------------------------------------------------------------------------------------ the container
def test_oriented_describes_frames_without_copying():
    a = oc.random_frames(6, 4, 6)
    t = torch.from_numpy(a)
    for rotate, hflip in oc.ALL:
        o = Oriented(t, rotate, hflip)
        assert o.shape == (6,) + oc.out_hw(4, 6, rotate) + (3,) and o.frames.data_ptr() == t.data_ptr()
        assert (o.rotate, o.hflip, o.quarters) == (rotate, hflip, rotate // 90) and not o.is_cuda
        assert o.is_identity == ((rotate, hflip) == (0, False))
        s = o[2:5]
        assert s.shape == (3,) + o.shape[1:] and (s.rotate, s.hflip) == (rotate, hflip)
        assert s.frames.data_ptr() == t[2:5].data_ptr()            # the same memory
        assert o[1:2].shape[0] == 1
        assert encode.frames_size(o) == (6, oc.out_hw(4, 6, rotate)) and encode.FrameSource(o).image_size == oc.out_hw(4, 6, rotate)
    assert Oriented(a, 90).frames.data_ptr() == a.__array_interface__["data"][0]       # a numpy array, not copied either
    assert encode.frames_size(Oriented(a, 90), (9, 9)) == (6, (9, 9))
    assert Oriented(a).is_identity and Oriented(a).shape == (6, 4, 6, 3)
    with pytest.raises(TypeError, match="slice"):
        Oriented(a, 90)[0]
    with pytest.raises(TypeError, match="slice"):
        Oriented(a, 90)[::2]
    # over a YuvFrames: the shape is that of the upright RGB frames the planes convert to
    y, u, v = yc.random_planes(5, 4, 6)
    f = preprocess.YuvFrames.i420(y, u, v)
    o = Oriented(f, 270, True)
    assert o.shape == (5, 6, 4, 3) and o.frames is f and o[1:3].shape == (2, 6, 4, 3) and o[1:3].frames.shape == (2, 4, 6, 3)
    assert preprocess.is_oriented(o) and not preprocess.is_yuv_frames(o) and not preprocess.is_oriented(f)
    assert not preprocess.is_oriented(t) and not preprocess.is_oriented(a)


def test_is_oriented_on_a_class_imported_under_the_second_package_name():
    other = importlib.import_module("tdc_video_amd.preprocess")     # `from tdc_video_amd import preprocess` is "tdc-video_amd.preprocess"
    a = oc.random_frames(2, 4, 6)
    for made_by, asked in ((other, preprocess), (preprocess, other)):
        o = made_by.Oriented(a, 90, True)
        assert asked.is_oriented(o) and not asked.is_yuv_frames(o)
        with pytest.raises(ValueError, match="Oriented"):
            asked.Oriented(o, 90)                                  # an Oriented inside an Oriented, whichever name made it


def test_oriented_refusals():
    a = oc.random_frames(2, 4, 6)
    for rotate in (1, -90, 45, 360, True, False, "90", None, 90.5):
        with pytest.raises(ValueError, match="rotate"):
            Oriented(a, rotate)
    for hflip in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="hflip"):
            Oriented(a, 90, hflip)
    for orientation in (0, 9, -1, True, None, "6"):
        with pytest.raises(ValueError, match="EXIF"):
            Oriented.exif(a, orientation)
    with pytest.raises(ValueError, match="Oriented"):
        Oriented(Oriented(a, 90), 90)
    # what check_frames refuses
    for bad in (a.astype(np.int16), a[..., :2], a[0], np.zeros((0, 4, 6, 3), np.uint8), torch.zeros(2, 4, 6, 3)):
        with pytest.raises(ValueError, match="frames"):
            Oriented(bad, 90)
    # what YuvFrames refuses is refused where the YuvFrames is made, before there is anything to wrap
    y, u, v = yc.random_planes(2, 4, 6)
    with pytest.raises(ValueError):
        Oriented(preprocess.YuvFrames.i420(y, u[:, :1], v), 90)


def test_preprocess_selected_checks_an_oriented_on_the_host_before_any_launch():
    towers = (dict(R=2, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)),) * 2
    y, u, v = yc.random_planes(6, 4, 6)
    for o in (Oriented(oc.random_frames(6, 4, 6), 90), Oriented(preprocess.YuvFrames.i420(y, u, v), 180, True)):
        for idx in ([0, 6], [-1, 2], [2, 1], []):
            with pytest.raises(ValueError, match="idx"):
                preprocess.preprocess_selected(o, idx, towers)      # no GPU here: raised before one would be needed
        with pytest.raises(ValueError, match="slab"):
            preprocess.preprocess_selected(o, None, towers, slab=0)
        with pytest.raises(ValueError, match="float16"):
            preprocess.preprocess_selected(o, None, towers, dtype=torch.float32)


def test_c_abi_entry_is_declared():
    from tdc_video_amd import lib, ops
    assert "tdc_orient_frames" in lib.SIGNATURES and len(lib.SIGNATURES["tdc_orient_frames"][1]) == 8
    assert callable(ops.orient_frames)


@pytest.mark.parametrize("other,v", [("tdc_feature_inputs", True), ("tdc_shard_frames", True), ("tdc_batch_frames", 512),
                                     ("tdc_shard_cache_bytes", 1 << 30), ("tdc_batch_prompts", 4)])
def test_sharded_batched_and_multi_prompt_configs_refuse_an_oriented_as_they_refuse_frames(other, v):
    lm = feature_lm(tdc_frame_inputs=True, **{other: v})
    lm.get_model()._tdc_encoder = Untouchable()
    with pytest.raises(ValueError) as ei:
        call(lm, [[Oriented(make_frames(30), 90)], None])
    assert "tdc_frame_inputs" in str(ei.value) and other in str(ei.value)


# ------------------------------------------------------------------------------------------------ the funnel
class _OrientedFrames(_Frames):
    """the double's pixels_from_frames on the upright frames of an Oriented; records what it was handed"""

    def pixels_from_frames(self, frames, idx=None):
        self.handed = getattr(self, "handed", []) + [frames]
        if preprocess.is_oriented(frames):
            inner = frames.frames
            frames = oc.orient(inner.numpy() if torch.is_tensor(inner) else inner, frames.rotate, frames.hflip)
        return _Frames.pixels_from_frames(self, frames, idx)


class OrientEngine(_OrientedFrames, FeatureEngine):
    pass


@pytest.mark.parametrize("rotate,hflip", [(90, False), (270, True), (180, False), (0, True)])
def test_frame_source_hands_the_wrapper_and_the_a1_indices_only(rotate, hflip):
    eng = OrientEngine(N=5)
    stored = make_frames(40)                                          # [40, 4, 6, 3]
    upright = oc.orient(stored, rotate, hflip)
    wi, gi = {}, {}
    want = encode.encode_frames_with(eng, upright, 4, 4, [1, 2, 3], frame_cap=30, info=wi)
    eng.asked, eng.handed = [], []
    o = Oriented(stored, rotate, hflip)
    got = encode.encode_frames_with(eng, o, 4, 4, [1, 2, 3], frame_cap=30, info=gi)
    assert torch.equal(got, want) and gi == wi and gi["frames_in"] == 40 and gi["frames_resized"] == 30
    assert eng.asked == [encode.frame_indices(eng.cfg, 40, 4, 30)] and len(eng.handed) == 1 and eng.handed[0] is o
    # the image form, through the slice the mixin takes
    i1, i2 = {}, {}
    assert torch.equal(encode.encode_frames_with(eng, o[3:4], None, 4, None, info=i1, image=True),
                       encode.encode_frames_with(eng, upright[3:4], None, 4, None, info=i2, image=True)) and i1 == i2
    a, b = encode.export_features_from_frames_with(eng, o, slab=16), encode.export_features_from_frames_with(eng, upright, slab=16)
    assert torch.equal(a.siglip, b.siglip) and torch.equal(a.dino, b.dino) and a.frames == 40
    assert a.image_size == b.image_size == oc.out_hw(4, 6, rotate)
