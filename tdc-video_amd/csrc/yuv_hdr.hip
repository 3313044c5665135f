// HDR YUV -> SDR RGB: 10- or 12-bit PQ or HLG surfaces, every layout yuv_planes.hip takes, tone-mapped
// to sRGB bytes by the stated formula of include/tdc_hip.h - no library's tone mapper.  The threads, the loads, the two forms
// (WORD / VEC, chosen on the host from the same alignment facts) and the stores are yuv_planes.hip's, shared through
// yuv_samples.h; what differs is what a pixel's three accumulators become, ONE device function for both forms:
//   stage A   the accumulators clamped and shifted to codes E_R, E_G, E_B in [0, N] at the samples' depth (integers, exact)
//   stage B   float32: l_c = LUT[E_c] (linear light in units of SDR white, or HLG scene light), the HLG OOTF, extended
//             Reinhard on the largest channel, the gamut matrix, the sRGB OETF, the byte
// The table (2^bits floats, 4 or 16 KB, random access) is staged into LDS once per block.  The powers are exp2(k * log2(x))
// on v_log_f32 / v_exp_f32, about eight transcendentals per pixel (two for the OOTF, six for the three sRGB curves).
#include <math.h>

#include "yuv_samples.h"

namespace {

struct hdr_pixel {
    tdc_hdr_desc h;
    const float* lut;     // the table in LDS

    // x^(1/2.4) scaled: the sRGB OETF of a clipped channel -> its byte
    __device__ __forceinline__ unsigned srgb_byte(float x) const {
        x = fminf(fmaxf(x, 0.0f), 1.0f);
        const float v = x <= 0.0031308f ? 12.92f * x : __builtin_fmaf(1.055f, fast_exp2((1.0f / 2.4f) * __builtin_amdgcn_logf(x)), -0.055f);
        return (unsigned)__builtin_fmaf(255.0f, v, 0.5f);
    }

    __device__ __forceinline__ void operator()(const depth& d, int ar, int ag, int ab, unsigned& r, unsigned& g, unsigned& b) const {
        float lr = lut[clip_down(d, ar)], lg = lut[clip_down(d, ag)], lb = lut[clip_down(d, ab)];
        if (h.ootf_exp != 0.0f) {       // HLG: scene light -> display light in units of SDR white (uniform branch)
            const float ys = h.luma[0] * lr + h.luma[1] * lg + h.luma[2] * lb;
            const float gain = ys > 0.0f ? h.ootf_scale * fast_exp2(h.ootf_exp * __builtin_amdgcn_logf(ys)) : 0.0f;
            lr *= gain; lg *= gain; lb *= gain;
        }
        const float m = fmaxf(lr, fmaxf(lg, lb));
        const float f = __builtin_fmaf(m, h.inv_p2, 1.0f) * fast_rcp(1.0f + m);
        lr *= f; lg *= f; lb *= f;
        r = srgb_byte(h.gamut[0] * lr + h.gamut[1] * lg + h.gamut[2] * lb);
        g = srgb_byte(h.gamut[3] * lr + h.gamut[4] * lg + h.gamut[5] * lb);
        b = srgb_byte(h.gamut[6] * lr + h.gamut[7] * lg + h.gamut[8] * lb);
    }
};

template <int SUBX, int FORM>
__global__ __launch_bounds__(256) void yuv_hdr_to_rgb_kernel(tdc_yuv_planes p, tdc_yuv_coef c, tdc_hdr_desc h, int T, int H, int W,
                                                             int units_x, int u_is_high, unsigned char* rgb) {
    extern __shared__ float lut[];      // 2^bits entries
    for (int i = threadIdx.x; i < 1 << p.bits; i += 256) lut[i] = h.lut[i];
    __syncthreads();
    yuv_frames<2, SUBX, FORM>(p, c, depth_of(p, p.bits), hdr_pixel{h, lut}, T, H, W, units_x, u_is_high, rgb);
}

template <int SUBX>
void launch(const yuv_launch& l, hipStream_t st, const tdc_yuv_planes& p, const tdc_yuv_coef& c, const tdc_hdr_desc& h, int T, int H,
            int W, unsigned char* rgb) {
    const dim3 block(256);
    const size_t lds = sizeof(float) << p.bits;
    if (l.form == WORD) hipLaunchKernelGGL((yuv_hdr_to_rgb_kernel<SUBX, WORD>), l.grid, block, lds, st, p, c, h, T, H, W, l.units_x, 0, rgb);
    else if (l.form == VEC_PLANAR) hipLaunchKernelGGL((yuv_hdr_to_rgb_kernel<SUBX, VEC_PLANAR>), l.grid, block, lds, st, p, c, h, T, H, W, l.units_x, 0, rgb);
    else hipLaunchKernelGGL((yuv_hdr_to_rgb_kernel<SUBX, VEC_PAIRED>), l.grid, block, lds, st, p, c, h, T, H, W, l.units_x, l.u_is_high, rgb);
}

}  // namespace

extern "C" int tdc_yuv_hdr_to_rgb(const tdc_yuv_planes* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h, int T, int H, int W,
                                  unsigned char* rgb, void* stream) {
    if (!h || !yuv_args_ok(p, c, T, H, W, rgb) || p->bits == 8) return TDC_E_BADARG;
    if (!h->lut || !aligned(h->lut, 4)) return TDC_E_BADARG;
    bool finite = isfinite(h->ootf_scale) && isfinite(h->ootf_exp) && isfinite(h->inv_p2);
    for (float v : h->luma) finite = finite && isfinite(v);
    for (float v : h->gamut) finite = finite && isfinite(v);
    if (!finite) return TDC_E_BADARG;
    if (!(h->inv_p2 > 0.0f && h->inv_p2 <= 1.0f) || !(h->ootf_exp >= 0.0f && h->ootf_exp < 1.0f)) return TDC_E_BADARG;
    if (h->ootf_exp != 0.0f && !(h->ootf_scale > 0.0f)) return TDC_E_BADARG;
    const yuv_launch l = yuv_launch_of(p, T, H, W, rgb);
    if (p->sub_x == 1) launch<1>(l, (hipStream_t)stream, *p, *c, *h, T, H, W, rgb);
    else launch<0>(l, (hipStream_t)stream, *p, *c, *h, T, H, W, rgb);
    return (int)hipGetLastError();
}
