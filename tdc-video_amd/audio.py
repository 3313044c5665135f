"""Decoded PCM audio as an encode's audio input: a decoder's track - interleaved int16, planar
float32, any channel count, 8 .. 192 kHz - is described by a PcmAudio, not copied, and resample() turns the output window
asked for into the mono 16 kHz waveform of amplitude +-1 that `audio={"audio_wav": ...}` takes (tdc_pcm_resample).  The
conversion is the stated polyphase formula of include/tdc_hip.h - a Kaiser-windowed sinc table built here in float64 - and
no library's.  Everything behind the waveform (kaldi fbank, BEATs, a20, the window cache) is the audio_wav path."""
import math

import numpy as np
import torch

from . import ops

TARGET_RATE = 16000
ROLLOFF, ZERO_CROSSINGS, KAISER_BETA = 0.9, 32, 8.0
MIN_RATE, MAX_RATE, MAX_PHASES = 8000, 192000, 640


def rate_factors(sample_rate):
    """(L, M) of an input rate: 16000 / g and sample_rate / g, g their gcd.  ValueError for anything but an integer rate in
    [8000, 192000] with L <= 640 (8, 11.025, 12, 16, 22.05, 24, 32, 44.1, 48, 88.2, 96, 176.4, 192 kHz all pass)."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)):
        raise ValueError("sample_rate must be an integer number of Hz, got %r" % (sample_rate,))
    sr = int(sample_rate)
    if not MIN_RATE <= sr <= MAX_RATE:
        raise ValueError("sample_rate must be in [%d, %d] Hz, got %d" % (MIN_RATE, MAX_RATE, sr))
    g = math.gcd(sr, TARGET_RATE)
    L, M = TARGET_RATE // g, sr // g
    if L > MAX_PHASES:
        raise ValueError("sample_rate %d Hz needs %d filter phases towards %d Hz, at most %d are taken"
                         % (sr, L, TARGET_RATE, MAX_PHASES))
    return L, M


def resample_table(sample_rate):
    """the filter of one input rate on the host -> (L, M, K, float32 [L, 2K]): built in float64 by the formula of
    include/tdc_hip.h, every row divided by its own sum, rounded once to float32"""
    L, M = rate_factors(sample_rate)
    c = ROLLOFF * min(1.0, TARGET_RATE / float(sample_rate))
    W = ZERO_CROSSINGS / c
    K = int(math.ceil(W))
    j = np.arange(-K + 1, K + 1, dtype=np.float64)
    p = np.arange(L, dtype=np.float64)
    tau = p[:, None] / L - j[None, :]
    inside = np.abs(tau) < W
    r = np.where(inside, 1.0 - (tau / W) ** 2, 0.0)
    h = c * np.sinc(c * tau) * np.i0(KAISER_BETA * np.sqrt(r)) / np.i0(KAISER_BETA)
    h = np.where(inside, h, 0.0)
    h = h / h.sum(axis=1, keepdims=True)
    return L, M, K, h.astype(np.float32)


_TABLES = {}        # (sample_rate, device) -> (L, M, K, the table on that device): made once, kept


def resample_tables(sample_rate, device=None):
    """(L, M, K, table float32 [L, 2K]) of one input rate as a tensor on `device` (None: the host)"""
    rate_factors(sample_rate)                             # ValueError for a rate that is not taken
    key = (int(sample_rate), str(torch.device("cpu" if device is None else device)))
    if key not in _TABLES:
        L, M, K, t = resample_table(sample_rate)
        _TABLES[key] = (L, M, K, torch.from_numpy(t).to(key[1]).contiguous())
    return _TABLES[key]


class PcmAudio:
    """One decoded audio track, described and not copied.  data: int16 (x = s / 32768, soundfile's convention) or float32
    (used as it is), a torch tensor on the host or on a device, or a numpy array: [n] mono, [n, C] interleaved (a decoder's
    packed formats), or [C, n] with layout="planar".  Element strides are taken as they are (a view with padding between
    samples, a channel of a wider buffer); a numpy view with a negative stride is made contiguous.  sample_rate: integer Hz
    (rate_factors).  channel: the index the waveform is taken from (default 0, the reference's audio[:, 0]) or "mean" = the
    fp32 mean of all channels, taken before filtering.  pcm[a:b] is a PcmAudio over input samples a .. b of the same memory
    (the reference's start_time / end_time slice).  n_out: the 16 kHz samples the track resamples to, ceil(n * L / M), and
    16000 for a track shorter than one second (as if it were zero-padded to one second first).  A PcmAudio has no padding:
    there is no mask to go with it."""

    def __init__(self, data, sample_rate, channel=0, layout=None):
        if isinstance(data, np.ndarray):
            if data.dtype not in (np.int16, np.float32):
                raise ValueError("PCM samples must be int16 or float32, got %s" % (data.dtype,))
            if any(s < 0 for s in data.strides):      # a reversed view: torch takes no negative strides
                data = np.ascontiguousarray(data)
            data = torch.from_numpy(data)
        if not torch.is_tensor(data):
            raise ValueError("PCM samples must be a torch tensor or a numpy array, got %s" % type(data).__name__)
        if data.dtype not in (torch.int16, torch.float32):
            raise ValueError("PCM samples must be int16 or float32, got %s" % (data.dtype,))
        if layout not in (None, "interleaved", "planar"):
            raise ValueError("layout is None / \"interleaved\" ([n, C]) or \"planar\" ([C, n]), got %r" % (layout,))
        if data.dim() == 1:
            x = data.unsqueeze(1)
        elif data.dim() == 2:
            x = data.t() if layout == "planar" else data
        else:
            raise ValueError("PCM samples must be [n], [n, C] or (layout=\"planar\") [C, n], got %s" % (tuple(data.shape),))
        n, C = x.shape
        if n < 1 or C < 1:
            raise ValueError("an empty track: %d samples of %d channels" % (n, C))
        if C > 65535:
            raise ValueError("at most 65535 channels, got %d (is the layout \"planar\"?)" % C)
        self.L, self.M = rate_factors(sample_rate)
        if channel != "mean" and (isinstance(channel, bool) or not isinstance(channel, (int, np.integer))
                                  or not 0 <= int(channel) < C):
            raise ValueError("channel is an index in [0, %d) or \"mean\", got %r" % (C, channel))
        if (n > 1 and x.stride(0) == 0) or (C > 1 and x.stride(1) == 0):      # an expanded view: the kernel takes strides >= 1
            x = x.contiguous()
        self.x = x                                          # [n, C] over the caller's memory
        self.sample_rate, self.channel = int(sample_rate), channel if channel == "mean" else int(channel)
        self.n_in, self.channels = int(n), int(C)
        self.n_out = max(-(-self.n_in * self.L // self.M), TARGET_RATE)

    @property
    def is_cuda(self):
        return self.x.is_cuda

    @property
    def channel_index(self):
        """the `channel` argument of tdc_pcm_resample: the index, or -1 for the mean"""
        return -1 if self.channel == "mean" else self.channel

    def __getitem__(self, s):
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError("PcmAudio takes a slice of input samples a:b, got %r" % (s,))
        a, b, _ = s.indices(self.n_in)
        if b <= a:
            raise ValueError("an empty track: samples %d:%d of %d" % (a, b, self.n_in))
        return PcmAudio(self.x[a:b], self.sample_rate, self.channel)


def is_pcm_audio(x):
    """a PcmAudio, recognised by its members (the package can be imported under two names: not by isinstance)"""
    return all(hasattr(x, k) for k in ("x", "sample_rate", "channel_index", "n_in", "n_out", "L", "M")) and not torch.is_tensor(x)


def input_span(pcm, lo, hi, K):
    """the input samples [a, b) that outputs [lo, hi) of a track read: floor(lo M / L) - K + 1 .. floor((hi - 1) M / L) + K,
    cut to the track (b <= a: the window lies in the zero padding).  At 16 kHz an output reads its own sample."""
    L, M = pcm.L, pcm.M
    if L == 1 and M == 1:
        return min(lo, pcm.n_in), min(hi, pcm.n_in)
    return max(lo * M // L - K + 1, 0), min((hi - 1) * M // L + K + 1, pcm.n_in)


def resample(pcm, lo=0, hi=None, dtype=torch.float32, device=None, stats=None):
    """outputs [lo, hi) of the track's 16 kHz waveform (hi None: pcm.n_out) -> wav [1, hi - lo] `dtype` (float32, or float16 =
    round to nearest of the fp32 sum) on `device` (default: the track's own device, the current one for a host track).  The
    bits of an output do not depend on the window it is asked in.  Device PCM is read in place through its strides.  Host PCM:
    only the span the window reads (input_span: its samples plus 2K of margin), of the addressed channel(s), goes through one
    pinned staging copy and one upload - pinned dense memory is uploaded from where it lies; the span starts at a multiple of
    M, so the staged samples keep their filter phase.  stats (a dict) receives uploaded_bytes."""
    if not is_pcm_audio(pcm):
        raise ValueError("resample takes a PcmAudio, got %s" % type(pcm).__name__)
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("the waveform is float32 or float16, got %s" % (dtype,))
    hi = pcm.n_out if hi is None else int(hi)
    lo = int(lo)
    if not 0 <= lo <= hi <= pcm.n_out:
        raise ValueError("outputs [%d, %d) are not a window of the track's %d" % (lo, hi, pcm.n_out))
    if device is None:
        device = pcm.x.device if pcm.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    L, M, K, table = resample_tables(pcm.sample_rate, device)
    a, b = input_span(pcm, lo, hi, K)
    if stats is not None:
        stats["uploaded_bytes"] = 0
    if hi == lo or b <= a:
        return torch.zeros(1, hi - lo, dtype=dtype, device=device)
    x, channel, shift = pcm.x, pcm.channel_index, 0
    if not x.is_cuda:
        k = a // M                                          # the span from a multiple of M: output n of the track is output
        a, shift = k * M, k * L                             # n - k L of the span, phase and taps unchanged
        src = x[a:b] if channel < 0 else x[a:b, channel:channel + 1]
        if not (src.is_pinned() and src.is_contiguous()):
            stage = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
            stage.copy_(src)
            src = stage
        x, channel = src.to(device, non_blocking=True), min(channel, 0)
        if stats is not None:
            stats["uploaded_bytes"] = src.numel() * src.element_size()
    elif x.device != device:
        x = x.to(device)
    out = torch.empty(1, hi - lo, dtype=dtype, device=device)
    ops.pcm_resample(x, channel, L, M, table, K, lo - shift, hi - lo, out[0])
    return out
