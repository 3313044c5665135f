"""Test-side restatement of the PCM resampler's definition (include/tdc_hip.h) in float64 numpy,
written from the stated formula and not from tdc-video_amd/audio.py, plus the makers of the test inputs.

    g = gcd(sr, 16000), L = 16000 / g, M = sr / g;  rolloff 0.9, 32 zero crossings, Kaiser beta 8
    c = rolloff * min(1, 16000 / sr);  W = 32 / c;  K = ceil(W)
    h(tau) = c sinc(c tau) I0(beta sqrt(1 - (tau / W)^2)) / I0(beta) for |tau| < W, else 0
    table[p][j] = h(p / L - j), j = -K+1 .. K, every row divided by its sum
    y[n] = sum_j table[(n M) mod L][j] x[floor(n M / L) + j],  x = 0 outside the track
"""
import math

import numpy as np

OUT_RATE = 16000
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


def factors(sr):
    g = math.gcd(sr, OUT_RATE)
    return OUT_RATE // g, sr // g


def kernel(tau, c, W, beta=8.0):
    """h(tau) in float64"""
    u = tau / W
    inside = np.abs(tau) < W
    win = np.i0(beta * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(beta)
    return np.where(inside, c * np.sinc(c * tau) * win, 0.0)


def table64(sr, rolloff=0.9, zeros=32, beta=8.0):
    """-> (L, M, K, float64 [L, 2K]), rows normalised to sum 1"""
    L, M = factors(sr)
    c = rolloff * min(1.0, OUT_RATE / float(sr))
    W = zeros / c
    K = int(math.ceil(W))
    j = np.arange(-K + 1, K + 1, dtype=np.float64)
    rows = np.stack([kernel(p / L - j, c, W, beta) for p in range(L)])
    rows = rows / rows.sum(axis=1, keepdims=True)
    return L, M, K, rows


def n_out_of(n_in, sr):
    """ceil(n L / M); a track shorter than one second is zero-padded to one second first"""
    L, M = factors(sr)
    return -(-max(n_in, sr) * L // M)


def resample64(x, sr, table=None, lo=0, hi=None):
    """outputs [lo, hi) of the definition for the mono float track x, in float64.  table: the [L, 2K] table the sum runs over
    (default table64; the kernel tests pass the float32 table the kernel reads, as float64)."""
    if table is None:
        table = table64(sr)[3]
    L, M = factors(sr)
    t = np.asarray(table, dtype=np.float64)
    K = t.shape[1] // 2
    assert t.shape == (L, 2 * K)
    x = np.asarray(x, dtype=np.float64)
    hi = n_out_of(len(x), sr) if hi is None else hi
    n = np.arange(lo, hi, dtype=np.int64)
    if L == 1 and M == 1:
        xp = np.concatenate([x, np.zeros(max(hi - len(x), 0))])
        return xp[n]
    base, phase = (n * M) // L, (n * M) % L
    last = int(base.max()) + K if len(n) else 0
    xp = np.concatenate([np.zeros(K), x, np.zeros(max(last + 1 - len(x), 0) + 1)])        # xp[i + K] = x[i]
    idx = base[:, None] + np.arange(-K + 1, K + 1)[None, :] + K
    return (xp[idx] * t[phase]).sum(axis=1)


def gain_bound(table):
    """S = max over the phases of sum_j |table[p][j]|"""
    return float(np.abs(np.asarray(table, dtype=np.float64)).sum(axis=1).max())


def tone(freq, sr, n, phase=0.0):
    return np.sin(2.0 * np.pi * freq * np.arange(n) / sr + phase)


def db(v):
    return 20.0 * math.log10(max(float(v), 1e-300))


# ---- inputs of the kernel tests ------------------------------------------------------------------------------------------
def uniform_pcm(n, channels, fmt, seed):
    """[n, channels] uniform in +-1: float32, or int16 over the whole code range"""
    rng = np.random.RandomState(seed)
    if fmt == "s16":
        return rng.randint(-32768, 32768, size=(n, channels)).astype(np.int16)
    return rng.uniform(-1.0, 1.0, size=(n, channels)).astype(np.float32)


def as_float(a):
    """the input sample of the definition: s / 32768 for int16 (exact in float32), float32 as it is"""
    a = np.asarray(a)
    return a.astype(np.float32) / np.float32(32768.0) if a.dtype == np.int16 else a.astype(np.float32)


def mean32(a):
    """the fp32 mean of all channels of [n, C]: summed in ascending channel order in float32, one float32 division"""
    f = as_float(a)
    s = f[:, 0].copy()
    for c in range(1, f.shape[1]):
        s = (s + f[:, c]).astype(np.float32)
    return (s / np.float32(f.shape[1])).astype(np.float32)


LAYOUTS = ("mono", "interleaved2", "planar2", "interleaved6_ch3", "strided", "offset1")


def layout_case(layout, n, fmt, seed, torch, device="cpu", poison=None):
    """one layout of the kernel tests -> (tensor to hand to PcmAudio, PcmAudio keywords, the selected channel as float32 [n],
    the backing buffer, a boolean mask over the backing buffer of the elements the call may read).
    poison: a value written to every element of the backing buffer outside that read set (int16 code or float)."""
    dt = torch.int16 if fmt == "s16" else torch.float32
    C, ch, kw = {"mono": (1, 0, {}), "interleaved2": (2, 0, {}), "planar2": (2, 1, {"layout": "planar"}),
                 "interleaved6_ch3": (6, 3, {}), "strided": (2, 1, {}), "offset1": (1, 0, {})}[layout]
    data = uniform_pcm(n, C, fmt, seed + 1)
    data[:, ch] = uniform_pcm(n, 1, fmt, seed)[:, 0]          # the selected channel: the same samples in every layout
    want = as_float(data[:, ch])
    pad = 64                                    # elements before and after the track in the backing buffer
    if layout == "strided":                     # frames of 2 channels, 5 elements apart: 3 elements of padding per frame
        buf = torch.zeros(pad + n * 5 + pad, dtype=dt)
        view = buf[pad:pad + n * 5].view(n, 5)[:, :2]
    elif layout == "planar2":                   # two planes with a gap between them
        plane = (n + 7) // 8 * 8 + 24          # a multiple of 16 bytes: the second plane keeps the first one's alignment
        buf = torch.zeros(pad + 2 * plane + pad, dtype=dt)
        view = buf[pad:pad + 2 * plane].view(2, plane)[:, :n]
    elif layout == "offset1":                   # one element past a 16-byte boundary: the 16-byte form is refused
        buf = torch.zeros(pad + 1 + n + pad, dtype=dt)
        view = buf[pad + 1:pad + 1 + n]
    elif layout == "mono":
        buf = torch.zeros(pad + n + pad, dtype=dt)
        view = buf[pad:pad + n]
    else:
        buf = torch.zeros(pad + n * C + pad, dtype=dt)
        view = buf[pad:pad + n * C].view(n, C)
    src = torch.from_numpy(data)
    if layout == "planar2":
        view.copy_(src.t())
    elif view.dim() == 1:
        view.copy_(src[:, 0])
    else:
        view.copy_(src)
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    mview = mask.as_strided(view.shape, view.stride(), view.storage_offset())
    if layout == "planar2":
        mview[ch, :] = True
    elif view.dim() == 1:
        mview[:] = True
    else:
        mview[:, ch] = True
    if poison is not None:
        buf[~mask] = poison
    buf = buf.to(device)
    view = buf.as_strided(view.shape, view.stride(), view.storage_offset())
    return view, dict(kw, channel=ch), want, buf, mask
