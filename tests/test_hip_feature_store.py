"""GPU (-m gpu): the compact feature store (features.FeatureSet with store = "e4m3").

  1. the decode form of tdc_gather_rows (tdc_gather_tables.scale) against torch's own float8_e4m3fn, bit for bit;
  2. its memory contract (tests/memcheck.py): writes out[i, 0 .. cols), reads the `cols` bytes and the scales of the rows
     `src` names and nothing else;
  3. the round trip lossless -> compact -> decoded rows against the bound the formats give;
  4. encode_features from a compact set on the reduced-dimension engine of test_hip_features (towers 48 / 64 wide: the
     SigLIP rows carry padding columns) against the lossless encode_features of the same engine - the selection equal, the
     tokens within the measured contract below.

The contract of item 4 cannot be derived; it was measured on an MI355X over the videos VIDEO_SEEDS of this module
(measure_parity, also what profiles/feature_store.json records): worst compressed-token error MEASURED_COMP (absolute, unit-norm
rows), worst static-row error MEASURED_STATIC (relative to max|ref|); the bounds are twice those."""
import numpy as np
import pytest
import torch

import memcheck as mc
import synth
from test_hip_boundary import loaded_lm
from test_hip_pipeline import make_encoder
from util import load_fixture, pipeline_cfg

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
VIDEO_SEEDS = (0, 1, 2, 3, 4, 5)
MEASURED_COMP, MEASURED_STATIC = 3.052e-4, 4.104e-4       # MI355X, worst of the six videos (fp16 engine)
TOL_COMP, TOL_STATIC = 2 * MEASURED_COMP, 2 * MEASURED_STATIC


@pytest.fixture(scope="module")
def ops():
    import tdc_video_amd  # noqa: F401
    from tdc_video_amd import ops as o
    assert torch.cuda.is_available()
    return o


def decode_ref(tab, scale, rows, cols, dtype):
    """(bytes.view(float8_e4m3fn).float() * scale[:, None]).to(dtype) of the named rows, on the host"""
    t = tab[rows, :cols].contiguous().view(torch.float8_e4m3fn).float()
    return (t * scale[rows][:, None]).to(dtype)


def same_or_both_nan(got, want):
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want.float())
    return bool(torch.equal(torch.isnan(got.float()), nan)) and torch.equal(got[~nan], want[~nan]) and \
        torch.equal(torch.signbit(got[~nan].float()), torch.signbit(want[~nan].float()))


def byte_table(g, R, cols, ld, offset):
    """uint8 [R, cols] rows with row stride ld at `offset` bytes behind an allocation's start; all 256 byte values occur"""
    tab = torch.randint(0, 256, (R, cols), generator=g, dtype=torch.uint8)
    tab.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    buf = torch.zeros(offset + R * ld + 64, dtype=torch.uint8, device="cuda")
    dev = buf[offset:offset + R * ld].view(R, ld)
    dev[:, :cols] = tab.cuda()
    return tab, dev[:, :cols]


def scales(g, R):
    s = torch.rand(R, generator=g) * 4.0 + 2.0 ** -6
    s[0], s[1], s[2], s[3], s[4] = 0.0, 1e-40, -0.75, 3.0e3, 2.0 ** -20     # zero, fp32 denormal, negative, fp16 overflow, tiny
    assert s[1] > 0 and s[1] < torch.finfo(torch.float32).tiny
    return s


# ------------------------------------------------------------------------------------------------ 1. decode exactness
@pytest.mark.parametrize("dtype", DT)
def test_decode_is_torchs_e4m3_times_scale_bit_for_bit(ops, dtype):
    g = torch.Generator().manual_seed(11)
    R = 40
    sc = scales(g, R)
    scd = sc.cuda()
    for cols in (8, 52, 64, 1152):
        # (row stride - cols, base offset): 16-byte loads, 8-byte loads (stride), 8-byte loads (base), element-wise (stride), (base)
        for extra, offset in ((32, 0), (24, 0), (32, 8), (13, 0), (32, 3)):
            tab, dev = byte_table(g, R, cols, cols + extra, offset)
            assert dev.data_ptr() % 16 == offset % 16 and dev.stride(0) == cols + extra
            for n in (1, 577):
                rows = torch.tensor([3] if n == 1 else [(R - 1 - i) % R for i in range(n)])      # reversed, every row 14 times
                src = torch.stack([torch.zeros_like(rows), rows], 1).int().cuda().contiguous()
                ldo = (cols + 7) // 8 * 8 + 8
                out = torch.full((n, ldo), 7.0, dtype=dtype, device="cuda")
                ops.gather_rows([dev], src, n, cols, out=out, scales=[scd], dtype=dtype)
                torch.cuda.synchronize()
                assert same_or_both_nan(out[:, :cols], decode_ref(tab, sc, rows, cols, dtype)), (cols, extra, offset, n)
                assert bool((out[:, cols:] == 7.0).all()), "pad columns written"
    # an output that allows no 16-byte store (odd row stride): element-wise too
    tab, dev = byte_table(g, R, 64, 96, 0)
    rows = torch.arange(R - 1, -1, -1)
    src = torch.stack([torch.zeros_like(rows), rows], 1).int().cuda().contiguous()
    out = torch.zeros(R, 67, dtype=dtype, device="cuda")
    ops.gather_rows([dev], src, R, 64, out=out, scales=[scd], dtype=dtype)
    assert same_or_both_nan(out[:, :64], decode_ref(tab, sc, rows, 64, dtype))


@pytest.mark.parametrize("dtype", DT)
def test_one_call_mixes_16_bit_and_e4m3_tables(ops, dtype):
    g = torch.Generator().manual_seed(12)
    R, cols = 40, 72
    sc = scales(g, R)
    tab, dev = byte_table(g, R, cols, 96, 0)
    t16 = torch.randn(9, cols, generator=g).to(dtype)
    vec = torch.randn(cols, generator=g).to(dtype)                # the newline row beside decoded rows
    pairs = [(1, 5), (0, 2), (2, 0), (1, 39), (0, 8), (1, 0), (1, 5), (2, 0), (0, 0)]
    src = torch.tensor(pairs, dtype=torch.int32).cuda()
    got = ops.gather_rows([t16.cuda(), dev, vec.cuda()], src, len(pairs), cols, scales=[None, sc.cuda(), None])
    assert got.dtype == dtype
    for i, (k, r) in enumerate(pairs):
        want = t16[r] if k == 0 else vec if k == 2 else decode_ref(tab, sc, torch.tensor([r]), cols, dtype)[0]
        assert same_or_both_nan(got[i], want), (i, k, r)
    # all scales None is the 16-bit form, unchanged
    src0 = torch.tensor([(0, 8), (1, 0), (0, 0)], dtype=torch.int32).cuda()
    assert torch.equal(ops.gather_rows([t16.cuda(), vec.cuda()], src0, 3, cols, scales=[None, None]).cpu(),
                       torch.stack([t16[8], vec, t16[0]]))


def test_gather_rows_checks_scales_on_the_host(ops):
    tab = torch.zeros(6, 16, dtype=torch.uint8, device="cuda")
    src = torch.tensor([[0, 5]], dtype=torch.int32).cuda()
    ok = torch.ones(6, device="cuda")
    assert ops.gather_rows([tab], src, 1, 16, scales=[ok], dtype=torch.float16).shape == (1, 16)
    for bad in (torch.ones(5, device="cuda"), torch.ones(6, device="cuda", dtype=torch.float16), torch.ones(6), ok.view(6, 1)):
        with pytest.raises(AssertionError):
            ops.gather_rows([tab], src, 1, 16, scales=[bad], dtype=torch.float16)
    with pytest.raises(AssertionError):                           # a row past the table, caught by the range check
        ops.gather_rows([tab], torch.tensor([[0, 6]], dtype=torch.int32).cuda(), 1, 16, scales=[ok], dtype=torch.float16)
    with pytest.raises(AssertionError):                           # every table e4m3: the output type must be given
        ops.gather_rows([tab], src, 1, 16, scales=[ok])
    with pytest.raises(AssertionError):                           # 16-bit bytes where e4m3 ones are announced
        ops.gather_rows([tab.half()], src, 1, 16, scales=[ok], dtype=torch.float16)


# ------------------------------------------------------------------------------------------------ 2. memory contract
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cols,ld,ldo", [(64, 96, 136), (72, 96, 136), (76, 93, 132)])      # 16-byte loads, 8-byte loads, element-wise
def test_decode_memory_contract(ops, dtype, cols, ld, ldo):
    """the e4m3 table rows no `src` entry names, the bytes cols .. ld behind the named rows, the scales of the other rows and
    everything around the table, the scales and `src` are poison (0x00, then 0xFF = NaN as e4m3 and as fp32); the output sits in
    a guarded arena"""
    g = torch.Generator().manual_seed(13)
    BAND = 64
    tab = torch.randint(0, 0x7F, (60, cols), generator=g, dtype=torch.uint8) | (torch.randint(0, 2, (60, cols), generator=g,
                                                                                              dtype=torch.uint8) << 7)
    sc = torch.rand(60, generator=g) + 0.25
    t16 = torch.randn(1, cols, generator=g).to(dtype)
    src = torch.tensor([[0, 5], [1, 0], [0, 59], [1, 0], [0, 5]], dtype=torch.int32)
    named = [5, 59]
    outs = []
    for fill in mc.PATTERNS:
        T0 = mc.poisoned(tab[named].cuda(), BAND, BAND, ld=ld, fill=fill, rows=named, total_rows=60, pad="poison")[0]
        S0 = mc.poisoned(sc[named].cuda(), BAND, BAND, fill=fill, rows=named, total_rows=60)[0]
        T1 = mc.poisoned(t16.cuda(), BAND, BAND, ld=ld, fill=fill)[0]
        out, oa = mc.guarded((5, cols), dtype, "cuda", BAND, BAND, ld=ldo, fill=fill)
        ops.gather_rows([T0, T1], mc.poisoned(src.cuda(), BAND, BAND, fill=fill)[0], 5, cols, out=out, validated=True,
                        scales=[S0, None])
        torch.cuda.synchronize()
        mc.assert_untouched(oa)
        outs.append(out.clone())
    assert mc.all_finite(outs[0]) and mc.all_finite(outs[1]), "the output is not finite: a poisoned byte or scale was read"
    assert mc.same_bits(outs[0], outs[1]), "the output depends on memory outside the declared read set"
    want = torch.stack([decode_ref(tab, sc, torch.tensor([5]), cols, dtype)[0], t16[0],
                        decode_ref(tab, sc, torch.tensor([59]), cols, dtype)[0], t16[0],
                        decode_ref(tab, sc, torch.tensor([5]), cols, dtype)[0]])
    assert torch.equal(outs[1].cpu(), want)


# ------------------------------------------------------------------------------------------------ the reduced engine
def _load(name="pipeline_T40.npz"):
    W, o = load_fixture(name)
    return dict(W=W, o=o, pid=[int(i) for i in o["prompt_ids"]], size=tuple(int(v) for v in o["image_size"]))


def video(o, seed):
    """[40, 3, px, px] on the fixture's basis: seed 0 is the fixture's own video, others the same construction re-drawn"""
    if seed == 0:
        return torch.from_numpy(synth.video_from_basis(o["video_basis"], o["video_coef"]))
    _, coef = synth.make_basis_and_coef(40, o["video_basis"].shape[-1], nb=o["video_basis"].shape[0], seed=seed)
    return torch.from_numpy(synth.video_from_basis(o["video_basis"], coef))


SMALL_PAIRS = (3, 9, 14, 20, 26)                 # of the 29 pairs of the 30 kept frames: the ones that stay inside a scene


def planted_video(o, enc, seed=9):
    """40 frames of which a1 keeps 30 (frame cap 30): a scene cut inside every kept pair but the five SMALL_PAIRS, so the 24
    lowest similarities of the 29 (max_num_segments = 24) lie far below the other five - the selection has one well-separated answer"""
    from tdc_video_amd import encode
    idx = encode.frame_indices(enc.cfg, 40, 9, 30)
    assert len(idx) == 30
    quiet = {t for j in SMALL_PAIRS for t in range(idx[j] + 1, idx[j + 1] + 1)}        # frames that continue their scene
    rng = np.random.RandomState(seed)
    nb = o["video_basis"].shape[0]
    coef = np.zeros((40, nb), dtype=np.float32)
    scenes = [0]
    for t in range(1, 40):
        if t in quiet:
            scenes.append(scenes[-1])
        else:                                   # a scene neither of the two frames before it shows (a kept pair may span two cuts)
            free = [s for s in range(nb) if s not in scenes[-2:]]
            scenes.append(free[rng.randint(0, len(free))])
    for t, s in enumerate(scenes):
        coef[t, s] = 1.0
        coef[t] += 0.02 * rng.randn(nb).astype(np.float32)
    return torch.from_numpy(synth.video_from_basis(o["video_basis"], coef)), idx


def row_kinds(enc, info, n_text):
    """per emitted row 0 = static (verbatim connector rows), 1 = compressed (unit-norm), 2 = separator - the plan of the call"""
    from tdc_video_amd import encode
    T = len(info["frame_indices"])
    h, w = info["final_size"][0]
    plan, _ = encode.emission_plan(enc, T, h * (w + 1), info["seg_indices"], encode.visual_budget(enc.cfg, n_text))
    return torch.from_numpy(np.asarray(plan.kind))


def parity(enc, want, got, info, n_text=8):
    """(worst absolute error on the compressed rows, worst error on the static rows relative to max|ref|)"""
    kinds = row_kinds(enc, info, n_text).to(want.device)
    assert kinds.numel() == want.shape[0] == got.shape[0] and bool((kinds == 1).any()) and bool((kinds == 0).any())
    d = (got.float() - want.float()).abs()
    comp, stat = kinds == 1, kinds == 0
    assert bool(((want[comp].float().norm(dim=1) - 1).abs() < 2e-3).all()), "the compressed rows are unit-norm"
    assert torch.equal(got[kinds == 2], want[kinds == 2]), "separators are verbatim"
    return float(d[comp].max()), float(d[stat].max() / want[stat].float().abs().max())


def measure_parity(enc, f, seeds=VIDEO_SEEDS):
    """per video seed: (compressed abs, static rel) of encode_features(compact) against encode_features(lossless), all frames
    kept - asserting on the way what must hold exactly: the selection, the shapes, the reported source of the similarities"""
    out = []
    for seed in seeds:
        vid = video(f["o"], seed).cuda()
        fs = enc.export_features(vid, vid + 0.01, f["size"])
        cs = enc.compact_features(fs)
        wi, gi = {}, {}
        want = enc.encode_features(fs, 9, 8, f["pid"], info=wi)
        got = enc.encode_features(cs, 9, 8, f["pid"], info=gi)
        assert gi.pop("selection_sims") == "stored" and gi == wi and len(gi["seg_indices"]) == 24
        assert got.shape == want.shape and got.dtype == want.dtype
        out.append(parity(enc, want, got, gi))
    return out


@pytest.fixture(scope="module")
def fx():
    """the T = 40 fixture, its fp16 engine (refinement off), the fixture video's lossless and compact sets - made once"""
    f = _load()
    f["enc"] = enc = make_encoder(f["W"], pipeline_cfg(f["o"]), torch.float16)
    assert enc.selection_eps is None
    f["vid"] = vid = video(f["o"], 0)
    f["fs"] = enc.export_features(vid.cuda(), (vid + 0.01).cuda(), f["size"])
    f["cs"] = enc.compact_features(f["fs"])
    return f


# ------------------------------------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("dtype", DT)
def test_round_trip_is_within_the_bound_of_the_formats(dtype):
    """x -> e4m3(x / s) * s, s = max|row| / 448: |x' - x| <= (2^-4 + u + 2^-12) |x| + 1.001 * 2^-10 * s + 2^-24 - half an ulp of
    three mantissa bits on a normal e4m3 value, u of the 16-bit result, 2^-12 for the fp32 products; half the e4m3 denormal
    spacing 2^-9 below 2^-6; 2^-24 of a denormal 16-bit result"""
    from tdc_video_amd.features import FeatureSet
    f = _load()
    enc = make_encoder(f["W"], pipeline_cfg(f["o"]), dtype)
    g = torch.Generator().manual_seed(21)
    T0, P = 5, 64
    u = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    xs = []
    for D in (48, 64):
        x = torch.randn(T0 * P, D, generator=g) * torch.exp(torch.randn(T0 * P, 1, generator=g) * 2.0)
        x = x.clamp(-150.0, 150.0)                                # the outlier below stays inside fp16
        x[7] = 0.0                                                # a zero row
        x[8, 5] *= 200.0                                          # a 200x outlier: the rest of its row in the e4m3 denormals
        x[9] = x[9].abs() * 2.0 ** -18                            # a tiny row
        x[10, :] = 448.0
        xs.append(x.to(dtype).reshape(T0, P, D).cuda())
    fs = FeatureSet(xs[0], xs[1], (384, 384), enc.feature_signature())
    cs = enc.compact_features(fs)
    assert cs.store == "e4m3" and cs.rows_dtype == dtype and cs.siglip.dtype == torch.uint8 and cs.siglip.is_cuda
    assert cs.nbytes == T0 * P * (48 + 64) + 8 * T0 * P + 4 * (T0 - 1)
    assert torch.equal(cs.sims, enc.sims_tensor(enc.feature_rows(fs.dino), T0))       # the lossless path's a5 launch, bit for bit
    for name, x, b, sc in (("siglip", xs[0], cs.siglip, cs.siglip_scale), ("dino", xs[1], cs.dino, cs.dino_scale)):
        D = x.shape[2]
        x = x.reshape(T0 * P, D).float()
        amax = x.abs().amax(1)
        s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        assert torch.allclose(sc.reshape(-1), s, rtol=2e-7, atol=0.0) and float(sc.reshape(-1)[7]) == 1.0
        for idx in (None, [4, 0, 2]):
            rows = enc.decode_feature_rows(b, sc, idx, dtype)
            sel = torch.arange(T0) if idx is None else torch.tensor(idx)
            want = x.reshape(T0, P, D)[sel.cuda()].reshape(-1, D)
            ss = s.reshape(T0, P)[sel.cuda()].reshape(-1, 1)
            assert rows.shape == (len(sel) * P, (D + 63) // 64 * 64) and rows.dtype == dtype
            assert torch.count_nonzero(rows[:, D:]) == 0, "padding columns"
            err = (rows[:, :D].float() - want).abs()
            bound = (2.0 ** -4 + u + 2.0 ** -12) * want.abs() + 1.001 * 2.0 ** -10 * ss + 2.0 ** -24
            worst = float((err / bound).max())
            print("round trip %s %s frames %s: worst error / bound = %.3f" % (dtype, name, idx, worst))
            assert worst <= 1.0
            if idx is None:
                assert torch.count_nonzero(rows[7]) == 0, "a zero row decodes to zeros"
                assert torch.equal(rows[10, :D], want[10].to(dtype)), "the row maximum is exact"


def test_export_and_compact_give_the_same_bytes(fx):
    enc, fs, cs = fx["enc"], fx["fs"], fx["cs"]
    ex = enc.export_features(fx["vid"].cuda(), (fx["vid"] + 0.01).cuda(), fx["size"], store="e4m3")
    assert sorted(ex.tensors()) == sorted(cs.tensors()) == ["dino", "dino_scale", "siglip", "siglip_scale", "sims"]
    for k, t in cs.tensors().items():
        assert torch.equal(getattr(ex, k), t) and t.is_cuda, k
    assert tuple(cs.siglip.shape) == (40, 64, 48) and tuple(cs.dino.shape) == (40, 64, 64) and cs.signature == fs.signature
    assert torch.equal(cs.sims, enc.sims_tensor(enc.feature_rows(fs.dino), 40)) and cs.sims.dtype == torch.float32
    assert cs.nbytes == 40 * 64 * (48 + 64) + 8 * 40 * 64 + 4 * 39 and enc.compact_features(cs) is cs
    with pytest.raises(ValueError, match="store"):
        enc.export_features(fx["vid"][:2].cuda(), fx["vid"][:2].cuda(), fx["size"], store="int8")


# ------------------------------------------------------------------------------------------------ 4. end to end
def test_all_frames_kept_the_selection_is_the_lossless_one_and_the_tokens_within_the_contract(fx):
    enc = fx["enc"]
    launches = []
    sims_tensor = enc.sims_tensor
    enc.sims_tensor = lambda d, T: launches.append(T) or sims_tensor(d, T)
    try:
        wi, gi = {}, {}
        enc.encode_features(fx["fs"], 9, 8, fx["pid"], info=wi)
        assert launches == [40]
        enc.encode_features(fx["cs"], 9, 8, fx["pid"], info=gi)
        assert launches == [40], "the compact set ran an a5 launch with every frame kept"
        assert gi["seg_indices"] == wi["seg_indices"] and gi["selection_sims"] == "stored" and "selection_sims" not in wi
    finally:
        enc.sims_tensor = sims_tensor
    res = measure_parity(enc, fx)
    for seed, (c, s) in zip(VIDEO_SEEDS, res):
        print("compact vs lossless, video seed %d: compressed rows max abs %.3e, static rows max rel %.3e" % (seed, c, s))
    print("worst: compressed %.3e (bound %s), static %.3e (bound %s)" % (max(c for c, _ in res), TOL_COMP,
                                                                         max(s for _, s in res), TOL_STATIC))
    assert max(c for c, _ in res) <= TOL_COMP and max(s for _, s in res) <= TOL_STATIC


def test_subsampled_frames_select_on_the_decoded_rows(fx):
    from tdc_video_amd import segment as seg
    enc = fx["enc"]
    vid, idx = planted_video(fx["o"], enc)
    vs, vd = vid.cuda(), (vid + 0.01).cuda()
    fs = enc.export_features(vs, vd, fx["size"])
    cs = enc.compact_features(fs)
    # the planted property, asserted on the lossless rows: the 24th and the 25th lowest similarity lie far apart, and the
    # decoded rows move no similarity by a tenth of that gap
    from tdc_video_amd import encode
    lossless = enc.sims_tensor(encode.feature_rows(enc, fs, idx)[1], 30).cpu()
    decoded = enc.sims_tensor(encode.feature_rows(enc, cs, idx)[1], 30).cpu()
    order = lossless.sort().values
    gap, moved = float(order[24] - order[23]), float((decoded - lossless).abs().max())
    print("planted video: selection gap %.4f, similarities moved by at most %.2e" % (gap, moved))
    assert gap > 0.05 and moved < 0.1 * gap
    assert sorted(lossless.argsort()[24:].tolist()) == list(SMALL_PAIRS)
    wi, gi = {}, {}
    want = enc.encode_features(fs, 9, 8, fx["pid"], frame_cap=30, info=wi)
    got = enc.encode_features(cs, 9, 8, fx["pid"], frame_cap=30, info=gi)
    assert gi.pop("selection_sims") == "decoded" and gi == wi and gi["frame_indices"] == idx
    assert gi["seg_indices"] == seg.select_segments(lossless.tolist(), 24) == [j for j in range(29) if j not in SMALL_PAIRS]
    assert got.shape == want.shape
    c, s = parity(enc, want, got, gi)
    print("compact vs lossless, 30 of 40 frames: compressed rows max abs %.3e, static rows max rel %.3e" % (c, s))
    assert c <= TOL_COMP and s <= TOL_STATIC


def test_one_image(fx):
    enc = fx["enc"]
    im = fx["vid"][7:8].cuda()
    size = (360, 640)
    fs = enc.export_features(im, im + 0.01, size)
    cs = enc.compact_features(fs)
    assert cs.sims is None and cs.frames == 1
    wi, gi = {}, {}
    want = enc.encode_features(fs, None, 8, None, image=True, info=wi)
    got = enc.encode_features(cs, None, 8, None, image=True, info=gi)
    assert gi == wi and got.shape == want.shape and got.dtype == want.dtype
    assert float((got.float() - want.float()).abs().max() / want.float().abs().max()) <= TOL_STATIC
    sig, dino = enc.decode_feature_rows(cs.siglip, cs.siglip_scale, None, enc.dtype), \
        enc.decode_feature_rows(cs.dino, cs.dino_scale, None, enc.dtype)
    assert torch.equal(got, enc.connector(sig, dino, 1, [size])[0][:, :enc.H])      # the connector on the decoded rows, nothing else


def test_saved_loaded_pinned_and_back(fx, tmp_path):
    enc, cs = fx["enc"], fx["cs"]
    want = enc.encode_features(cs, 9, 8, fx["pid"], frame_cap=30)
    want_all = enc.encode_features(cs, 9, 8, fx["pid"])
    path = str(tmp_path / "v.tdcfeat")
    cs.save(path)
    loaded = type(cs).load(path)
    assert loaded.store == "e4m3" and not loaded.siglip.is_cuda and loaded.nbytes == cs.nbytes
    host = loaded.cpu()
    assert all(t.is_pinned() for t in host.tensors().values()) and host.rows_dtype == cs.rows_dtype
    assert torch.equal(enc.encode_features(host, 9, 8, fx["pid"], frame_cap=30), want)          # uploaded by the call
    assert torch.equal(enc.encode_features(host, 9, 8, fx["pid"]), want_all)
    back = host.to(enc.dev)
    assert all(t.is_cuda for t in back.tensors().values())
    for k, t in cs.tensors().items():
        assert torch.equal(getattr(back, k), t), k
    assert torch.equal(enc.encode_features(back, 9, 8, fx["pid"], frame_cap=30), want)
    # a compact set of the other 16-bit type is refused by this engine
    other = type(cs)(cs.siglip, cs.dino, cs.image_size, cs.signature, cs.siglip_scale, cs.dino_scale, cs.sims, torch.bfloat16)
    with pytest.raises(ValueError, match="decode to"):
        enc.encode_features(other, 9, 8, fx["pid"])


def test_prompts_equal_the_single_prompt_calls(fx):
    enc, cs, pid = fx["enc"], fx["cs"], fx["pid"]
    qs = [dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid),
          dict(budget_text_len=9, n_text_tokens=11, prompt_ids=pid[:5] + pid[-1:]),
          dict(budget_text_len=9, n_text_tokens=8, prompt_ids=pid[1:4] + pid[-1:])]
    infos = [{} for _ in qs]
    got = enc.encode_features_prompts(cs, qs, infos=infos, pad_fraction=1.0)
    assert [i["prompts"]["group_size"] for i in infos] == [3, 3, 3]
    for p, q in enumerate(qs):
        wi = {}
        want = enc.encode_features(cs, q["budget_text_len"], q["n_text_tokens"], q["prompt_ids"], info=wi)
        assert torch.equal(got[p], want), p
        assert {k: v for k, v in infos[p].items() if k != "prompts"} == wi and wi["selection_sims"] == "stored"


def _call(lm, ids, images, size, prompts, n=1):
    ids = ids.repeat(n, 1)
    pos = torch.arange(ids.shape[1])[None].repeat(n, 1)
    return lm.prepare_inputs_labels_for_multimodal(ids, pos, torch.ones_like(ids), None, ids.clone(), images,
                                                   image_sizes=[size] * n, video_indices=[None] * n, prompts=prompts,
                                                   audios=[None] * n)


def test_through_the_mixin(fx):
    lm = loaded_lm(fx["W"], fx["o"], tdc_feature_inputs=True)
    ids = torch.from_numpy(fx["o"]["input_ids"])
    eng = lm.get_model().tdc_engine()
    vid = fx["vid"]
    fs = eng.export_features(vid, vid + 0.01, fx["size"])
    cs = eng.export_features(vid, vid + 0.01, fx["size"], store="e4m3")
    towers = []
    tower = eng.tower
    eng.tower = lambda name, px: towers.append(name) or tower(name, px)
    want = _call(lm, ids, [[fs], [None]], fx["size"], [fx["pid"]])
    got = _call(lm, ids, [[cs], [None]], fx["size"], [fx["pid"]])
    host = _call(lm, ids, [[cs.cpu()], [None]], fx["size"], [fx["pid"]])
    assert towers == [] and len(got) == len(want) == 10
    for a, b, c in zip(got, want, host):
        if torch.is_tensor(a):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, c)
        else:
            assert a == b == c
    # the spliced embeddings: text rows verbatim, visual rows within the contract of the static rows (the looser one)
    d = (got[4].detach().float() - want[4].detach().float()).abs().max() / want[4].detach().float().abs().max()
    assert float(d) <= max(TOL_STATIC, TOL_COMP)
    # config.tdc_batch_prompts: the same compact video twice is one group
    pid = fx["pid"]
    prompts = [pid, pid[:5] + pid[-1:]]
    clone = type(cs)(cs.siglip.clone(), cs.dino.clone(), cs.image_size, cs.signature, cs.siglip_scale.clone(),
                     cs.dino_scale.clone(), cs.sims.clone(), cs.rows_dtype)
    off = _call(lm, ids, [[cs, clone], [None, None]], fx["size"], prompts, 2)
    lm.get_model().config.tdc_batch_prompts = 4
    lm.get_model().config.tdc_prompt_pad_fraction = 1.0
    seen = []
    multi = eng.encode_features_prompts
    eng.encode_features_prompts = lambda fs_, qs, **kw: seen.append(len(qs)) or multi(fs_, qs, **kw)
    on = _call(lm, ids, [[cs, clone], [None, None]], fx["size"], prompts, 2)
    assert seen == [2]
    for a, b in zip(on, off):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
