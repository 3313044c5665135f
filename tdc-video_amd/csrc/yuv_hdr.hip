// HDR YUV -> SDR RGB: 10- or 12-bit PQ or HLG surfaces, every layout yuv_planes.hip takes, tone-mapped
// to sRGB bytes by the stated formula of include/tdc_hip.h - no library's tone mapper.  The threads, the loads, the two forms
// (WORD / VEC, chosen on the host from the same alignment facts) and the stores are yuv_planes.hip's, shared through
// yuv_samples.h; what differs is what a pixel's three accumulators become, ONE device function for both forms:
//   stage A   the accumulators clamped and shifted to codes E_R, E_G, E_B in [0, N] at the samples' depth (integers, exact)
//   stage B   float32: l_c = LUT[E_c] (linear light in units of SDR white, or HLG scene light), the HLG OOTF, extended
//             Reinhard on the largest channel, the gamut matrix, the sRGB OETF, the byte
// The table (2^bits floats, 4 or 16 KB, random access) is staged into LDS once per block.  The powers are exp2(k * log2(x))
// on v_log_f32 / v_exp_f32, about eight transcendentals per pixel (two for the OOTF, six for the three sRGB curves).
#include "yuv_pixels.h"

namespace {

template <int SUBX, int FORM>
__global__ __launch_bounds__(256) void yuv_hdr_to_rgb_kernel(tdc_yuv_planes p, tdc_yuv_coef c, tdc_hdr_desc h, int T, int H, int W,
                                                             int units_x, int u_is_high, unsigned char* rgb) {
    extern __shared__ float lut[];      // 2^bits entries
    stage_hdr_lut(lut, h, p.bits);
    yuv_frames<2, SUBX, FORM>(p, c, depth_of(p, p.bits), hdr_pixel{h, lut}, T, H, W, units_x, u_is_high, rgb);
}

template <int SUBX>
void launch(const yuv_launch& l, hipStream_t st, const tdc_yuv_planes& p, const tdc_yuv_coef& c, const tdc_hdr_desc& h, int T, int H,
            int W, unsigned char* rgb) {
    with_form(l.form, [&](auto form) {
        hipLaunchKernelGGL((yuv_hdr_to_rgb_kernel<SUBX, decltype(form)::value>), l.grid, dim3(256), sizeof(float) << p.bits, st, p, c, h, T,
                           H, W, l.units_x, l.u_is_high, rgb);
    });
}

}  // namespace

extern "C" int tdc_yuv_hdr_to_rgb(const tdc_yuv_planes* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h, int T, int H, int W,
                                  unsigned char* rgb, void* stream) {
    if (!hdr_desc_ok(h) || !yuv_args_ok(p, c, T, H, W, rgb) || p->bits == 8) return TDC_E_BADARG;
    const yuv_launch l = yuv_launch_of(p, T, H, W, rgb);
    if (p->sub_x == 1) launch<1>(l, (hipStream_t)stream, *p, *c, *h, T, H, W, rgb);
    else launch<0>(l, (hipStream_t)stream, *p, *c, *h, T, H, W, rgb);
    return (int)hipGetLastError();
}
