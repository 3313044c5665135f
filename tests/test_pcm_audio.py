"""CPU: the PCM resampler's definition and host logic.

Quality is measured on the float64 restatement of the definition (tests/pcm_cases.py) with one-second unit tones; the first
and last 400 outputs (5 % of the 16000) are left out, nothing else.  Figures measured with this definition (dB re the tone):
1 kHz error -96.3 .. -98.5, 6 kHz error -87.2 .. -88.3, tones from 8.8 kHz to sr/2 come out at -89.7 .. -97.5, 1 kHz from
8 kHz within -87.4; the bounds below leave 2 - 6 dB for tone phase and table rounding."""
import numpy as np
import pytest
import torch

import pcm_cases as pc

EDGE = 400
DOWN_RATES = (48000, 44100, 32000, 22050, 96000)


def _audio():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import audio
    return audio


def _tone_error_db(sr, freq, table):
    y = pc.resample64(pc.tone(freq, sr, sr), sr, table)
    assert len(y) == 16000
    ideal = pc.tone(freq, 16000, 16000)
    return pc.db(np.abs(y - ideal)[EDGE:-EDGE].max())


@pytest.mark.parametrize("sr", DOWN_RATES)
def test_definition_passband_and_stopband(sr):
    table = pc.table64(sr)[3]
    e1, e6 = _tone_error_db(sr, 1000.0, table), _tone_error_db(sr, 6000.0, table)
    print("sr %d: 1 kHz error %.1f dB, 6 kHz error %.1f dB" % (sr, e1, e6))
    assert e1 <= -90.0 and e6 <= -84.0
    worst = -1e9
    for f in np.linspace(8800.0, 0.999 * sr / 2, 40):
        y = pc.resample64(pc.tone(f, sr, sr, 0.3), sr, table)
        worst = max(worst, pc.db(np.abs(y)[EDGE:-EDGE].max()))
    print("sr %d: loudest stopband tone %.1f dB" % (sr, worst))
    assert worst <= -85.0


def test_definition_upsampling_from_8k():
    e1 = _tone_error_db(8000, 1000.0, pc.table64(8000)[3])
    print("sr 8000: 1 kHz error %.1f dB" % e1)
    assert e1 <= -85.0


@pytest.mark.parametrize("sr", pc.RATES)
def test_product_table_is_the_restatement_rounded_once(sr):
    audio = _audio()
    L, M, K, t = audio.resample_tables(sr)
    rL, rM, rK, r = pc.table64(sr)
    assert (L, M, K) == (rL, rM, rK) and L * sr == M * 16000 and np.gcd(L, M) == 1
    assert K == int(np.ceil(32 / (0.9 * min(1.0, 16000 / sr))))
    assert t.dtype == torch.float32 and tuple(t.shape) == (L, 2 * K) and not t.is_cuda
    assert np.array_equal(t.numpy().view(np.uint32), r.astype(np.float32).view(np.uint32))
    assert np.abs(t.numpy().astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
    assert audio.resample_tables(sr)[3] is t                      # made once per rate and device


def test_widest_tables():
    audio = _audio()
    for sr, rows, taps in ((44100, 160, 196), (22050, 320, 98)):
        L, _, K, t = audio.resample_tables(sr)
        assert (L, 2 * K) == (rows, taps) and t.numel() * 4 == 125440          # 122.5 KB


@pytest.mark.parametrize("sr", pc.RATES)
def test_n_out(sr):
    audio = _audio()
    L, M = pc.factors(sr)
    for n in (1, 37, sr - 1, sr, sr + 1, 2 * 44100 + 123):
        pcm = audio.PcmAudio(torch.zeros(n, dtype=torch.int16), sr)
        want = 16000 if n < sr else -(-n * L // M)
        assert pcm.n_out == want == pc.n_out_of(n, sr) and pcm.n_in == n
    if sr == 44100:
        assert audio.PcmAudio(np.zeros(2 * 44100 + 123, np.float32), sr).n_out == 32045


def test_shapes_layouts_and_slices():
    audio = _audio()
    a = np.arange(2 * 1000, dtype=np.int16).reshape(1000, 2)
    inter = audio.PcmAudio(a, 48000, channel=1)
    planar = audio.PcmAudio(np.ascontiguousarray(a.T), 48000, channel=1, layout="planar")
    for p in (inter, planar):
        assert (p.n_in, p.channels, p.channel_index, p.n_out) == (1000, 2, 1, 16000)
        assert torch.equal(p.x, torch.from_numpy(a))
    assert inter.x.data_ptr() == torch.from_numpy(a).data_ptr()                 # described, not copied
    assert tuple(inter.x.stride()) == (2, 1) and tuple(planar.x.stride()) == (1, 1000)
    mono = audio.PcmAudio(torch.arange(50000, dtype=torch.float32), 44100)
    assert (mono.channels, mono.n_out) == (1, -(-50000 * 160 // 441))
    cut = mono[4410:48510]                                                      # one second from 0.1 s
    assert cut.n_in == 44100 and cut.n_out == 16000 and cut.x.data_ptr() == mono.x[4410:].data_ptr()
    assert cut.sample_rate == 44100 and audio.PcmAudio(a, 48000, channel="mean")[10:20].channel_index == -1
    flipped = audio.PcmAudio(a[::-1], 48000)                                    # a negative numpy stride: made contiguous
    assert torch.equal(flipped.x, torch.from_numpy(np.ascontiguousarray(a[::-1])))
    padded = audio.PcmAudio(torch.zeros(100, 5, dtype=torch.int16)[:, :2], 32000)
    assert tuple(padded.x.stride()) == (5, 1)
    assert audio.is_pcm_audio(mono) and not audio.is_pcm_audio(mono.x)
    with pytest.raises(TypeError):
        mono[::2]
    with pytest.raises(ValueError):
        mono[10:10]


def test_input_span_is_the_window_plus_2k():
    audio = _audio()
    pcm = audio.PcmAudio(torch.zeros(10 * 48000, dtype=torch.int16), 48000)
    K = audio.resample_tables(48000)[2]
    assert audio.input_span(pcm, 0, pcm.n_out, K) == (0, pcm.n_in)
    a, b = audio.input_span(pcm, 16000, 32000, K)
    assert (a, b) == (48000 - K + 1, 3 * 31999 + K + 1) and b - a == 3 * 15999 + 2 * K
    at16 = audio.PcmAudio(torch.zeros(100, dtype=torch.int16), 16000)
    assert audio.input_span(at16, 50, 16000, 36) == (50, 100)


def test_value_errors():
    audio = _audio()
    ok = torch.zeros(100, 2, dtype=torch.int16)
    for data in (torch.zeros(100, dtype=torch.int32), torch.zeros(100, dtype=torch.float64), np.zeros(100, np.uint8),
                 torch.zeros(100, dtype=torch.float16), [0.0] * 100):
        with pytest.raises(ValueError):
            audio.PcmAudio(data, 48000)
    for data in (torch.zeros((), dtype=torch.int16), torch.zeros(2, 3, 4, dtype=torch.int16)):       # rank
        with pytest.raises(ValueError):
            audio.PcmAudio(data, 48000)
    for data in (torch.zeros(0, dtype=torch.int16), torch.zeros(0, 2, dtype=torch.int16), torch.zeros(5, 0, dtype=torch.float32)):
        with pytest.raises(ValueError):                                                                # empty
            audio.PcmAudio(data, 48000)
    for sr in (7999, 192001, 0, -48000, 44101, 16001, 48000.0, "48000", True, None):
        with pytest.raises(ValueError):
            audio.PcmAudio(ok, sr)
        with pytest.raises(ValueError):
            audio.resample_tables(sr)
    for ch in (2, -1, 1.0, "left", None, True):
        with pytest.raises(ValueError):
            audio.PcmAudio(ok, 48000, channel=ch)
    with pytest.raises(ValueError):
        audio.PcmAudio(ok, 48000, layout="packed")
    for sr in pc.RATES:
        audio.PcmAudio(ok, sr, channel=1)
    pcm = audio.PcmAudio(ok, 48000)
    for kw in (dict(lo=-1), dict(hi=16001), dict(lo=5, hi=4), dict(dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            audio.resample(pcm, **kw)
    with pytest.raises(ValueError):
        audio.resample(ok)


class _Engine:
    """the members normalize_audio / audio_key read, on the host: the fingerprint in numpy, the resampler = the float64
    restatement rounded to float32"""
    dev = torch.device("cpu")

    def __init__(self):
        self.resampled = 0

    def fingerprint(self, px, rows, row_bytes=None, row_stride=None):
        from tdc_video_amd.cache import fingerprint_rows_host
        b = px.contiguous().view(-1).view(torch.uint8).numpy()
        return [tuple(int(v) for v in fingerprint_rows_host(b[row_stride * r:row_stride * r + row_bytes])[0]) for r in rows]

    def resample_pcm(self, pcm):
        self.resampled += 1
        x = pc.mean32(pcm.x.numpy()) if pcm.channel == "mean" else pc.as_float(pcm.x[:, pcm.channel].numpy())
        return torch.from_numpy(pc.resample64(x, pcm.sample_rate).astype(np.float32))[None]


def test_normalize_audio_and_keys():
    audio = _audio()
    from tdc_video_amd import encode
    e = _Engine()
    a = pc.uniform_pcm(3000, 2, "s16", 1)
    b = a.copy()
    b[1500, 0] += 1
    pa, pa2, pb = (audio.PcmAudio(v, 48000) for v in (a, a.copy(), b))
    other = audio.PcmAudio(a, 48000, channel=1)
    norm = encode.normalize_audio(e, {"audio_pcm": pa})
    assert sorted(norm) == ["audio_wav"] and tuple(norm["audio_wav"].shape) == (1, 16000)
    assert norm["audio_wav"].dtype == torch.float32
    for same in (None, {"audio_wav": norm["audio_wav"]}, {"audio_pcm": None, "beats_windows": [1]}, norm["audio_wav"]):
        n0 = e.resampled
        assert encode.normalize_audio(e, same) is same and e.resampled == n0       # anything else: the object it is
    for k in ("audio_wav", "beats_windows", "audio_tokens", "audio_wav_mask"):
        with pytest.raises(ValueError):
            encode.normalize_audio(e, {"audio_pcm": pa, k: torch.zeros(1, 4)})
    with pytest.raises(ValueError):
        encode.normalize_audio(e, {"audio_pcm": torch.zeros(100)})
    idx = [0, 1, 2]
    key = lambda p: encode.audio_key(e, {"audio_pcm": p}, 3, idx)
    assert key(pa) == key(pa2) == encode.audio_key(e, norm, 3, idx)            # equal tracks, and the waveform itself
    assert key(pa) != key(pb) and key(pa) != key(other)
    assert encode.audio_key(e, None, 3, idx) is None

    class Src:
        T0 = 3

        def same_key(self, eng, idx, audio=None, video_index=None):
            assert audio is None or "audio_pcm" not in audio                   # normalised before the source sees it
            return ("video", tuple(idx), encode.audio_key(eng, audio, self.T0, idx, video_index))
    e.cfg = {"tokenizer_model_max_length": 8192}
    sk = lambda p: encode.same_source_key(e, Src(), 64, 224, {"audio_pcm": p})
    assert sk(pa) == sk(pa2) and sk(pa) != sk(pb)


def test_symbol_is_registered():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import lib
    assert "tdc_pcm_resample" in lib.SIGNATURES and len(lib.SIGNATURES["tdc_pcm_resample"][1]) == 16
