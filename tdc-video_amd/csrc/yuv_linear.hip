// YUV 4:2:0 / 4:2:2 -> RGB with interpolated chroma: every planar surface yuv_planes.hip and yuv_hdr.hip
// take at those sub-samplings, 8-bit 4:2:0 included.  The chroma samples are interpolated linearly per axis at the samples'
// depth - two taps per sub-sampled axis, weights in quarters by where the samples sit (tdc_chroma_site), indices clamped on the
// picture's own Wc and Hc, one rounding of the 2-D sum - and the result takes the place of the replicated sample in the
// per-pixel code of yuv_samples.h / yuv_pixels.h, which runs unchanged: SDR (h == NULL) or the HDR tone mapping.
// The threads, the forms (WORD / VEC, chosen on the host from the same alignment facts) and the stores are yuv_frames'.  A
// thread reads its own run of chroma samples in each row it needs - its own row, and for 4:2:0 the row above (centred) and
// the row below - with the loads of the replicate kernel, and one halo sample left (centred) and right of the run as
// single-sample loads; neighbouring threads re-read those from the vector cache / L2.  No LDS but the HDR table.
#include "yuv_linear.h"
#include "yuv_pixels.h"

namespace {

// one chroma row of a thread's unit: the NC samples of its run (NC = 1: WORD; NC = 4: the vector forms, loaded as yuv_frames
// loads them) with the clamped halo samples -> the horizontal sums of its 2 NC pixels, for u and v
template <int BS, int FORM>
__device__ __forceinline__ void chroma_row(const tdc_yuv_planes& p, const unsigned char* uf, const unsigned char* vf, long long crow,
                                           int xu, int Wc, const depth& d, int u_is_high, const axis_taps& wx,
                                           int (&hu)[FORM == WORD ? 2 : 8], int (&hv)[FORM == WORD ? 2 : 8]) {
    constexpr int NC = FORM == WORD ? 1 : 4;
    int su[NC + 2], sv[NC + 2];
    chroma_run<BS, NC, FORM>(p, uf, vf, crow, xu, d, u_is_high, su + 1, sv + 1);
    // the halo: by index on the picture's own Wc, never past the row's read set
    const int k0 = xu * NC;
    su[0] = sv[0] = 0;
    if (wx.eb) {        // uniform: only the centred siting looks left
        const long long off = crow + (long long)(k0 > 0 ? k0 - 1 : 0) * p.c_step;
        su[0] = sample_at<BS>(uf + off, d);
        sv[0] = sample_at<BS>(vf + off, d);
    }
    const long long off = crow + (long long)(k0 + NC < Wc ? k0 + NC : Wc - 1) * p.c_step;
    su[NC + 1] = sample_at<BS>(uf + off, d);
    sv[NC + 1] = sample_at<BS>(vf + off, d);
    horizontal_sums<NC>(su, wx, hu);
    horizontal_sums<NC>(sv, wx, hv);
}

// the walk, the units and the stores are yuv_frames' (yuv_samples.h) at sub_x = 1, with a chroma term per pixel.  A
// neighbour's index is clamped to [0, Wc - 1] / [0, Hc - 1] of the frame t itself.
template <int BS, int FORM, class PX>
__device__ __forceinline__ void yuv_linear_frames(const tdc_yuv_planes& p, const tdc_yuv_coef& c, const depth& d, const PX& px,
                                                  const tdc_chroma_site& s, int T, int H, int W, int units_x, int u_is_high,
                                                  unsigned char* rgb) {
    constexpr int NP = FORM == WORD ? 2 : 8;        // pixels of a unit's row
    const int Hc = (H + p.sub_y) >> p.sub_y, Wc = (W + 1) >> 1;
    const axis_taps wx = axis_taps_of(s.sit_x, 1), wy = axis_taps_of(s.sit_y, p.sub_y);
    const long long units = yuv_units(p, H, units_x);
    for (int t = blockIdx.y; t < T; t += gridDim.y)
        for (long long i = first_unit(); i < units; i += unit_stride()) {
            const yuv_unit n = yuv_unit_of(p, t, i, units_x, H, W, rgb);
            int hu[NP], hv[NP];                         // the unit's own chroma row
            chroma_row<BS, FORM>(p, n.uf, n.vf, (long long)n.yc * p.c_pitch, n.xu, Wc, d, u_is_high, wx, hu, hv);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                if (dy == 1 && !n.two_rows) break;
                const int wa = dy ? wy.oa : wy.ea, wb = dy ? wy.ob : wy.eb;
                int gu[NP], gv[NP];                     // the other chroma row of this pixel row: above (dy = 0) or below
#pragma unroll
                for (int k = 0; k < NP; ++k) gu[k] = gv[k] = 0;
                if (wb) {       // uniform
                    const int ro = dy ? (n.yc + 1 < Hc ? n.yc + 1 : Hc - 1) : (n.yc > 0 ? n.yc - 1 : 0);
                    chroma_row<BS, FORM>(p, n.uf, n.vf, (long long)ro * p.c_pitch, n.xu, Wc, d, u_is_high, wx, gu, gv);
                }
                chroma_terms ct[NP];
#pragma unroll
                for (int k = 0; k < NP; ++k)
                    ct[k] = chroma(c, d, interpolated(wa, hu[k], wb, gu[k]), interpolated(wa, hv[k], wb, gv[k]));
                emit_row<BS, 0, FORM, 2>(c, d, px, n.yr + (long long)dy * p.y_pitch, n.orow + (long long)dy * W * 3, n.xu, W, ct);
            }
        }
}

template <int BS, int FORM>
__global__ __launch_bounds__(256) void yuv_linear_to_rgb_kernel(tdc_yuv_planes p, tdc_yuv_coef c, tdc_chroma_site s, int T, int H, int W,
                                                                int units_x, int u_is_high, unsigned char* rgb) {
    yuv_linear_frames<BS, FORM>(p, c, depth_of(p, 8), sdr_pixel(), s, T, H, W, units_x, u_is_high, rgb);
}

template <int FORM>
__global__ __launch_bounds__(256) void yuv_linear_hdr_to_rgb_kernel(tdc_yuv_planes p, tdc_yuv_coef c, tdc_hdr_desc h, tdc_chroma_site s,
                                                                    int T, int H, int W, int units_x, int u_is_high, unsigned char* rgb) {
    extern __shared__ float lut[];      // 2^bits entries
    stage_hdr_lut(lut, h, p.bits);
    yuv_linear_frames<2, FORM>(p, c, depth_of(p, p.bits), hdr_pixel{h, lut}, s, T, H, W, units_x, u_is_high, rgb);
}

template <int BS, int FORM>
void launch_form(const yuv_launch& l, hipStream_t st, const tdc_yuv_planes& p, const tdc_yuv_coef& c, const tdc_hdr_desc* h,
                 const tdc_chroma_site& s, int T, int H, int W, unsigned char* rgb) {
    const dim3 block(256);
    if constexpr (BS == 2) {
        if (h) {
            hipLaunchKernelGGL((yuv_linear_hdr_to_rgb_kernel<FORM>), l.grid, block, sizeof(float) << p.bits, st, p, c, *h, s, T, H, W,
                               l.units_x, l.u_is_high, rgb);
            return;
        }
    }
    hipLaunchKernelGGL((yuv_linear_to_rgb_kernel<BS, FORM>), l.grid, block, 0, st, p, c, s, T, H, W, l.units_x, l.u_is_high, rgb);
}

template <int BS>
void launch(const yuv_launch& l, hipStream_t st, const tdc_yuv_planes& p, const tdc_yuv_coef& c, const tdc_hdr_desc* h,
            const tdc_chroma_site& s, int T, int H, int W, unsigned char* rgb) {
    with_form(l.form, [&](auto form) { launch_form<BS, decltype(form)::value>(l, st, p, c, h, s, T, H, W, rgb); });
}

}  // namespace

extern "C" int tdc_yuv_linear_to_rgb(const tdc_yuv_planes* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h, const tdc_chroma_site* s,
                                     int T, int H, int W, unsigned char* rgb, void* stream) {
    if (!chroma_site_ok(s) || !yuv_args_ok(p, c, T, H, W, rgb) || p->sub_x != 1) return TDC_E_BADARG;
    if (h && (p->bits == 8 || !hdr_desc_ok(h))) return TDC_E_BADARG;
    const yuv_launch l = yuv_launch_of(p, T, H, W, rgb);
    if (p->bits == 8) launch<1>(l, (hipStream_t)stream, *p, *c, h, *s, T, H, W, rgb);
    else launch<2>(l, (hipStream_t)stream, *p, *c, h, *s, T, H, W, rgb);
    return (int)hipGetLastError();
}
