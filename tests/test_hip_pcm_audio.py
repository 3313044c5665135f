"""GPU (-m gpu): encode from decoded PCM audio.  tdc_pcm_resample against the float64 restatement of
the definition (pcm_cases) - every rate, sample format and layout, its range independence, its memory contract and its
refusals - and the audio funnel on the tiny fixture engine: everything behind the resampler is the audio_wav path, so every
end-to-end comparison is bit for bit against the same call on audio.resample's waveform.

Kernel tolerance (derived, not measured): every fp32 output within (2K + 8) * 2^-24 * S * max|x| of the restatement, S = max_p
sum_j |table[p][j]| computed from the table - the worst case of a 2K-term fp32 FMA chain plus one rounding of the table;
fp16 outputs add 2^-11 |y| for the one rounding to fp16."""
import ctypes as C

import numpy as np
import pytest
import torch

import memcheck
import pcm_cases as pc
import synth
import test_hip_memory_contract as contract
from test_hip_boundary import loaded_lm
from test_hip_frame_inputs import frames_of, towers
from test_hip_pipeline import make_encoder
from util import load_fixture, pipeline_cfg

pytestmark = pytest.mark.gpu

KERNEL_RATES = (48000, 44100, 32000, 22050, 11025, 8000, 96000)
FMTS = ("s16", "f32")


def _audio():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import audio
    return audio


def bound(sr, xmax):
    """(the fp32 tolerance, the float64 table) of one rate"""
    _, _, K, t = pc.table64(sr)
    return (2 * K + 8) * 2.0 ** -24 * pc.gain_bound(t.astype(np.float32)) * xmax, t


def check(got, want, tol, what):
    got = got.double().cpu().numpy().reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    lim = tol if np.isscalar(tol) else np.asarray(tol)
    assert np.all(np.isfinite(got)) and np.all(err <= lim), (what, float(err.max()), float(np.max(lim)))
    return float(err.max())


# ---------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("sr", KERNEL_RATES)
def test_kernel_against_fp64(sr):
    """every sample format x layout x track length of one rate, fp32 and fp16 outputs, device-resident PCM read in place"""
    audio = _audio()
    tol, t64 = bound(sr, 1.0)
    worst = 0.0
    for n in (37, 12345, sr + 1):
        for fmt in FMTS:
            refs = {}
            for layout in pc.LAYOUTS:
                view, kw, x, _, _ = pc.layout_case(layout, n, fmt, 11 * n + len(fmt), torch, "cuda")
                pcm = audio.PcmAudio(view, sr, **kw)
                key = x.tobytes()
                if key not in refs:
                    refs[key] = pc.resample64(x, sr, t64)
                want = refs[key]
                assert pcm.n_out == len(want) == pc.n_out_of(n, sr)
                y32 = audio.resample(pcm)
                assert tuple(y32.shape) == (1, pcm.n_out) and y32.dtype == torch.float32
                worst = max(worst, check(y32, want, tol, (sr, n, fmt, layout)))
                y16 = audio.resample(pcm, dtype=torch.float16)
                assert y16.dtype == torch.float16
                check(y16, want, tol + 2.0 ** -11 * np.abs(want), (sr, n, fmt, layout, "fp16"))
    print("tdc_pcm_resample sr %d: largest fp32 error %.3g, bound %.3g" % (sr, worst, tol))


def test_int16_extremes():
    audio = _audio()
    for sr in (48000, 44100):
        tol, t64 = bound(sr, 1.0)
        for code in (-32768, 32767):
            x = torch.full((12345, 2), code, dtype=torch.int16, device="cuda")
            want = pc.resample64(np.full(12345, code / 32768.0), sr, t64)
            got = audio.resample(audio.PcmAudio(x, sr))
            check(got, want, tol, (sr, code))
            mid = got[0, 2000:3000].double().cpu().numpy()            # far from both ends: the DC gain of a row is 1
            assert np.abs(mid - code / 32768.0).max() <= tol


@pytest.mark.parametrize("sr", (48000, 44100, 8000))
def test_channel_mean(sr):
    audio = _audio()
    tol, t64 = bound(sr, 1.0)
    for fmt in FMTS:
        for C_, planar in ((2, False), (2, True), (6, False), (4, True)):
            n = 12345
            a = pc.uniform_pcm(n, C_, fmt, 5 + C_)
            want = pc.resample64(pc.mean32(a), sr, t64)
            if planar:                                               # planes 16-byte multiples apart: the vector form
                plane = (n + 7) // 8 * 8
                buf = torch.zeros(C_, plane, dtype=torch.from_numpy(a).dtype, device="cuda")
                buf[:, :n] = torch.from_numpy(a).t().cuda()
                pcm = audio.PcmAudio(buf[:, :n], sr, channel="mean", layout="planar")
            else:
                pcm = audio.PcmAudio(torch.from_numpy(a).cuda(), sr, channel="mean")
            check(audio.resample(pcm), want, tol, (sr, fmt, C_, planar))
            host = audio.PcmAudio(a.T.copy() if planar else a, sr, channel="mean", layout="planar" if planar else None)
            assert memcheck.same_bits(audio.resample(host), audio.resample(pcm))


@pytest.mark.parametrize("sr", (44100, 48000))
def test_range_independence_and_load_forms(sr):
    """outputs [lo, hi) asked on their own are the same bits as in the whole-track call - from device PCM (read in place) and
    from host PCM (only the window's span is staged, from a multiple of M) - and the 16-byte and one-sample load forms agree"""
    audio = _audio()
    n = 3 * sr + 17
    for fmt in FMTS:
        vec, kw, x, _, _ = pc.layout_case("mono", n, fmt, 3, torch, "cuda")
        sca, _, x2, _, _ = pc.layout_case("offset1", n, fmt, 3, torch, "cuda")
        assert np.array_equal(x, x2) and vec.data_ptr() % 16 == 0 and sca.data_ptr() % 16 != 0
        whole = audio.resample(audio.PcmAudio(vec, sr))
        assert memcheck.same_bits(whole, audio.resample(audio.PcmAudio(sca, sr)))
        inter = torch.from_numpy(pc.uniform_pcm(n, 2, fmt, 4))
        mono = {"vec": vec, "sca": sca, "host": vec.cpu(), "pinned": vec.cpu().pin_memory()}
        stereo = {"dev": inter.cuda(), "host": inter}
        for dtype in (torch.float32, torch.float16):
            full = {"vec": audio.resample(audio.PcmAudio(vec, sr), dtype=dtype),
                    "stereo": audio.resample(audio.PcmAudio(stereo["dev"], sr, channel=1), dtype=dtype)}
            for lo in (1, 255, 257, 1000):
                for length in (1, 255, 777, 20001):
                    hi = lo + length
                    for name, src in mono.items():
                        got = audio.resample(audio.PcmAudio(src, sr), lo, hi, dtype=dtype)
                        assert memcheck.same_bits(got, full["vec"][:, lo:hi]), (fmt, name, lo, hi)
                    for name, src in stereo.items():
                        st = {}
                        got = audio.resample(audio.PcmAudio(src, sr, channel=1), lo, hi, dtype=dtype, stats=st)
                        assert memcheck.same_bits(got, full["stereo"][:, lo:hi]), (fmt, name, lo, hi)
                        if name == "host":                           # the window's span of ONE channel, not the track
                            K = audio.resample_tables(sr)[2]
                            L, M = pc.factors(sr)
                            assert 0 < st["uploaded_bytes"] <= (length * M // L + 2 * K + M + 1) * inter.element_size()
        tail = audio.resample(audio.PcmAudio(vec, sr), whole.shape[1] - 333, whole.shape[1])      # the window at the track's end
        assert memcheck.same_bits(tail, whole[:, -333:])


def test_16k_is_a_plain_select():
    audio = _audio()
    for fmt in FMTS:
        for layout in pc.LAYOUTS:
            view, kw, x, _, _ = pc.layout_case(layout, 20001, fmt, 9, torch, "cuda")
            pcm = audio.PcmAudio(view, 16000, **kw)
            got = audio.resample(pcm)
            assert np.array_equal(got.cpu().numpy()[0].view(np.uint32), x.view(np.uint32)), (fmt, layout)
            assert memcheck.same_bits(audio.resample(pcm, 5, 18000), got[:, 5:18000])
            assert torch.equal(audio.resample(pcm, dtype=torch.float16), got.half())
            host = audio.PcmAudio(view.cpu(), 16000, **kw)
            assert memcheck.same_bits(audio.resample(host, 5, 18000), got[:, 5:18000])
        short = audio.PcmAudio(torch.from_numpy(pc.uniform_pcm(37, 1, fmt, 2)).cuda(), 16000)     # padded to one second
        got = audio.resample(short)
        assert tuple(got.shape) == (1, 16000) and torch.count_nonzero(got[:, 37:]) == 0
        assert np.array_equal(got.cpu().numpy()[0, :37], pc.as_float(pc.uniform_pcm(37, 1, fmt, 2)[:, 0]))
    s = torch.tensor([-32768, -1, 0, 1, 32767], dtype=torch.int16, device="cuda")
    assert audio.resample(audio.PcmAudio(s, 16000))[0, :5].tolist() == [-1.0, -1 / 32768, 0.0, 1 / 32768, 32767 / 32768]


# ---------------------------------------------------------------------------------------------------- the memory contract
# tests/test_memcheck.py holds every launching entry point of the C ABI to a named test that runs it inside guarded and
# poisoned memory, through the registry of test_hip_memory_contract.  tdc_pcm_resample's is the function below: it is entered
# there under its own name (not a test_ name: that module collects nothing new).
@contract.covers("tdc_pcm_resample")
def pcm_resample_memory_contract(sr, fmt):
    """tdc_pcm_resample: out in a guarded arena - nothing outside out[0 .. n_out) changes; the track inside a backing buffer
    whose other channels, padding between the samples of a strided view, gap between planes and 64 elements before and after
    the track hold zeros, then a poison (0xAAAA as int16, NaN as float32) - identical, finite output."""
    from tdc_video_amd import ops
    audio = _audio()
    L, M, K, table = audio.resample_tables(sr, "cuda")
    poison = -21846 if fmt == "s16" else float("nan")
    for layout in pc.LAYOUTS:
        for n, lo, n_out in ((12345, 0, None), (12345, 257, 1001), (37, 0, None)):
            results = []
            for p in (None, poison):
                view, kw, _, _, _ = pc.layout_case(layout, n, fmt, 21, torch, "cuda", poison=p)
                pcm = audio.PcmAudio(view, sr, **kw)
                cnt = pcm.n_out if n_out is None else n_out
                for dtype in (torch.float32, torch.float16):
                    out, arena = memcheck.guarded((cnt,), dtype, "cuda", 512, 512)
                    ops.pcm_resample(pcm.x, pcm.channel_index, L, M, table, K, lo, cnt, out)
                    torch.cuda.synchronize()
                    memcheck.assert_untouched(arena)
                    assert memcheck.all_finite(out)
                    results.append(out.clone())
            assert memcheck.same_bits(results[0], results[2]) and memcheck.same_bits(results[1], results[3]), (layout, n, lo)
    # the mean reads every channel and still nothing between the frames of a strided view or around the track
    results = []
    data = torch.from_numpy(pc.uniform_pcm(12345, 2, fmt, 22)).cuda()
    for p in (0, poison):
        buf = torch.full((64 + 12345 * 5 + 64,), p, dtype=data.dtype, device="cuda")
        view = buf[64:64 + 12345 * 5].view(12345, 5)[:, :2]
        view.copy_(data)
        out, arena = memcheck.guarded((4000,), torch.float32, "cuda", 512, 512)
        ops.pcm_resample(view, -1, L, M, table, K, 0, 4000, out)
        torch.cuda.synchronize()
        memcheck.assert_untouched(arena)
        results.append(out.clone())
    assert memcheck.same_bits(*results) and memcheck.all_finite(results[0])


contract.pcm_resample_memory_contract = pcm_resample_memory_contract


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("sr", (44100, 48000, 16000, 8000))
def test_memory_contract(sr, fmt):
    pcm_resample_memory_contract(sr, fmt)


# ---------------------------------------------------------------------------------------------------- refusals
def test_badarg_before_any_launch():
    audio = _audio()
    from tdc_video_amd import lib as L
    lib = L.load()
    Lp, M, K, table = audio.resample_tables(48000, "cuda")
    x = torch.zeros(64 + 1000 * 2, dtype=torch.int16, device="cuda")
    out, arena = memcheck.guarded((400,), torch.float32, "cuda", 64, 64)
    good = dict(pcm=x.data_ptr(), fmt=0, n_in=1000, channels=2, ss=2, cs=1, channel=0, L=Lp, M=M, table=table.data_ptr(), K=K,
                lo=0, n=300, out=out.data_ptr(), f32=1)

    def rc(**kw):
        a = dict(good, **kw)
        return lib.tdc_pcm_resample(C.c_void_p(a["pcm"]), a["fmt"], a["n_in"], a["channels"], a["ss"], a["cs"], a["channel"], a["L"],
                                    a["M"], C.c_void_p(a["table"]), a["K"], a["lo"], a["n"], C.c_void_p(a["out"]), a["f32"],
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [rc(pcm=0), rc(table=0), rc(out=0),                                                    # null pointers
           rc(pcm=x.data_ptr() + 1), rc(fmt=1, pcm=x.data_ptr() + 2), rc(out=out.data_ptr() + 2), rc(f32=0, out=out.data_ptr() + 1),
           rc(table=table.data_ptr() + 4),                                                       # misaligned pointers
           rc(fmt=-1), rc(fmt=2), rc(channel=2), rc(channel=5), rc(channel=-2), rc(channels=0), rc(n_in=0), rc(n_in=-5),
           rc(K=0), rc(K=-3), rc(lo=-1), rc(n=-1), rc(ss=0), rc(ss=-2), rc(cs=-1), rc(L=0), rc(L=641), rc(M=0), rc(M=(1 << 20) + 1),
           rc(lo=1 << 40, n=1), rc(K=9000), rc(L=1, M=300)]                                       # a span beyond the LDS
    torch.cuda.synchronize()
    assert all(r != 0 for r in bad) and set(bad) == {bad[0]}, bad        # TDC_E_BADARG, every one
    memcheck.assert_untouched(arena, torch.zeros(400, dtype=torch.bool))
    with pytest.raises(L.TdcHipError):
        L.check(bad[0], "tdc_pcm_resample")
    assert rc(n=0) == 0 and rc() == 0                                    # nothing to write; and the good call goes through
    torch.cuda.synchronize()
    rows = torch.zeros(400, dtype=torch.bool)
    rows[:300] = True
    memcheck.assert_untouched(arena, rows)


# ---------------------------------------------------------------------------------------------------- end to end
def _beats_state():
    """the random 768-wide BEATs of test_raw_waveform_audio_through_beats_vs_oracle (tests/golden/beats_small.npz is 64 wide
    and cannot feed the 768-wide audio_proj of the pipeline fixture)"""
    import beats_oracle as BO
    bcfg = dict(BO.BEATS_ITER3_CFG, embed_dim=64, encoder_layers=2, encoder_ffn_embed_dim=256, conv_pos=16,
                num_buckets=64, max_distance=200)
    g = torch.Generator().manual_seed(31)
    rn = lambda *s, std=0.05: torch.randn(*s, generator=g) * std
    Cw, E = 768, 64
    BW = {"patch_embedding.weight": rn(E, 1, 16, 16, std=0.06), "layer_norm.weight": 1 + rn(E), "layer_norm.bias": rn(E),
          "post_extract_proj.weight": rn(Cw, E, std=0.1), "post_extract_proj.bias": rn(Cw),
          "encoder.pos_conv.0.weight_g": 1 + rn(1, 1, 16).abs(), "encoder.pos_conv.0.weight_v": rn(Cw, Cw // 16, 16),
          "encoder.pos_conv.0.bias": rn(Cw), "encoder.layer_norm.weight": 1 + rn(Cw), "encoder.layer_norm.bias": rn(Cw)}
    emb = rn(64, 12, std=1.0)
    for i in range(2):
        p = "encoder.layers.%d." % i
        for nme in ("q_proj", "k_proj", "v_proj", "out_proj"):
            BW[p + "self_attn." + nme + ".weight"], BW[p + "self_attn." + nme + ".bias"] = rn(Cw, Cw, std=0.04), rn(Cw)
        BW[p + "self_attn.grep_linear.weight"], BW[p + "self_attn.grep_linear.bias"] = rn(8, 64, std=0.2), rn(8, std=0.2)
        BW[p + "self_attn.grep_a"] = 1 + rn(1, 12, 1, 1, std=0.2)
        BW[p + "self_attn.relative_attention_bias.weight"] = emb
        BW[p + "fc1.weight"], BW[p + "fc1.bias"] = rn(256, Cw, std=0.04), rn(256)
        BW[p + "fc2.weight"], BW[p + "fc2.bias"] = rn(Cw, 256, std=0.06), rn(Cw)
        for nme in ("self_attn_layer_norm", "final_layer_norm"):
            BW[p + nme + ".weight"], BW[p + nme + ".bias"] = 1 + rn(Cw), rn(Cw)
    return BW, bcfg


def _tracks(seconds):
    """a 48 kHz interleaved stereo int16 track and a 44.1 kHz planar stereo float32 track of `seconds`: tones under noise"""
    rng = np.random.RandomState(8)
    out = {}
    for name, sr in (("s16_48k", 48000), ("f32_44k", 44100)):
        n = seconds * sr
        t = np.arange(n) / sr
        a = np.stack([0.3 * np.sin(2 * np.pi * (180.0 + 40.0 * c) * t * (1 + 0.05 * t)) + 0.05 * rng.randn(n) for c in range(2)], 1)
        out[name] = (np.round(a * 32767).clip(-32768, 32767).astype(np.int16), sr, {}) if name == "s16_48k" else \
            (np.ascontiguousarray(a.T.astype(np.float32)), sr, {"layout": "planar"})
    return out


@pytest.fixture(scope="module")
def fx():
    """the T = 40 audio fixture's engine with a BEATs encoder and 126-px frame towers - made once, never changed"""
    from tdc_video_amd.beats import BeatsEncoder
    W, o = load_fixture("pipeline_T40_audio.npz")
    enc = make_encoder(W, pipeline_cfg(o), torch.float16)
    BW, bcfg = _beats_state()
    enc.beats = BeatsEncoder(BW, bcfg, dtype=torch.float16, device="cuda:0")
    enc.frame_towers = towers()
    vid = torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    ids = torch.from_numpy(o["input_ids"])
    seconds = o["audio_wav"].shape[1] // 16000
    return dict(W=W, o=o, enc=enc, vs=vid.cuda(), vd=(vid + 0.01).cuda(), ids=ids, size=tuple(int(v) for v in o["image_size"]),
                pid=[int(i) for i in o["prompt_ids"]], tracks=_tracks(seconds), beats=(BW, bcfg), vid=vid)


def _run(f, audio_in, **kw):
    n = f["ids"].shape[1]
    return f["enc"].encode_video(f["vs"], f["vd"], f["size"], budget_text_len=n, n_text_tokens=n - 1, prompt_ids=f["pid"],
                                 audio=audio_in, **kw)


@pytest.mark.parametrize("track", ("s16_48k", "f32_44k"))
def test_encode_video_from_pcm_equals_the_waveform_path(fx, track):
    audio = _audio()
    data, sr, kw = fx["tracks"][track]
    host = audio.PcmAudio(data, sr, **kw)
    dev = audio.PcmAudio(torch.from_numpy(data).cuda(), sr, **kw)
    wav = audio.resample(host)
    assert wav.is_cuda and wav.dtype == torch.float32 and wav.shape[1] == fx["o"]["audio_wav"].shape[1]
    assert memcheck.same_bits(audio.resample(dev), wav) and memcheck.same_bits(fx["enc"].resample_pcm(dev), wav)
    want = _run(fx, {"audio_wav": wav})
    base = _run(fx, None)
    assert base.shape != want.shape or not torch.equal(base, want)      # the audio counts
    for pcm in (host, dev):
        assert torch.equal(_run(fx, {"audio_pcm": pcm}), want)
    # encode_frames: the same audio funnel behind another source
    frames = frames_of(90, 160)
    n = fx["ids"].shape[1]
    ef = lambda a: fx["enc"].encode_frames(frames, n, n - 1, fx["pid"], audio=a)
    assert torch.equal(ef({"audio_pcm": host}), ef({"audio_wav": wav}))
    # the frame cache: the BEATs windows are keyed by the content of the resampled waveform - a second question hits them
    c = fx["enc"].new_cache(1 << 30)
    i1, i2 = {}, {}
    assert torch.equal(_run(fx, {"audio_pcm": host}, cache=c, info=i1), want)
    assert i1["cache"]["windows_encoded"] > 0
    assert torch.equal(_run(fx, {"audio_pcm": dev}, cache=c, info=i2), want)
    assert i2["cache"]["windows_encoded"] == 0 and i2["cache"]["frames_encoded"] == 0
    for k in ("audio_wav", "beats_windows", "audio_tokens"):
        with pytest.raises(ValueError, match="audio_pcm"):
            _run(fx, {"audio_pcm": host, k: wav})


def _same(a, b):
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y)
        else:
            assert x == y


def test_mixin_passes_pcm_through(fx):
    audio = _audio()
    lm = loaded_lm(fx["W"], fx["o"], audio_input=True)
    BW, bcfg = fx["beats"]
    lm.get_model().initialize_audio(beats_ckpt={"cfg": bcfg, "model": BW})
    data, sr, kw = fx["tracks"]["s16_48k"]
    pcm = audio.PcmAudio(data, sr, **kw)
    ids = fx["ids"]

    def call(au):
        return lm.prepare_inputs_labels_for_multimodal(ids, None, torch.ones_like(ids), None, ids.clone(),
                                                       [fx["vid"].unsqueeze(0), (fx["vid"] + 0.01).unsqueeze(0)],
                                                       image_sizes=[fx["size"]], video_indices=[None], prompts=[fx["pid"]],
                                                       audios=[au])
    want = call({"audio_wav": audio.resample(pcm)})
    _same(call({"audio_pcm": pcm}), want)
    with pytest.raises(ValueError, match="audio_pcm"):
        call({"audio_pcm": pcm, "audio_wav": audio.resample(pcm)})


class _Traced:
    """the loaded library with every C-ABI call logged by name"""

    def __init__(self, real, log):
        self.__dict__.update(_real=real, _log=log)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("tdc_"):
            return fn

        def call(*a):
            self._log.append(name)
            return fn(*a)
        return call


def test_other_audio_issues_no_resample_launch(fx, monkeypatch):
    """a dict without audio_pcm, and no audio at all, issue the launches they issued before: none of them is the resampler"""
    audio = _audio()
    from tdc_video_amd import lib as L
    data, sr, kw = fx["tracks"]["s16_48k"]
    wav = audio.resample(audio.PcmAudio(data, sr, **kw))
    log = []
    monkeypatch.setattr(L, "_lib", _Traced(L.load(), log))
    _run(fx, {"audio_wav": wav})
    with_wav = list(log)
    del log[:]
    _run(fx, None)
    without = list(log)
    del log[:]
    _run(fx, {"audio_pcm": audio.PcmAudio(torch.from_numpy(data).cuda(), sr, **kw)})
    assert "tdc_fbank" in with_wav and len(without) > 10
    assert "tdc_pcm_resample" not in with_wav and "tdc_pcm_resample" not in without
    assert log == ["tdc_pcm_resample"] + with_wav                       # one launch in front, the waveform path behind it
