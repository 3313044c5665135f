// What a pixel's three accumulators become, shared by every YUV -> RGB kernel (yuv_planes.hip, yuv_hdr.hip, yuv_packed.hip): the
// SDR functor, the HDR functor with the staging of its table into LDS and the host's refusals of a
// tdc_hdr_desc (section 21).  One definition each, so that a packed surface gives the bytes of the same samples held in planes
// by construction.
#pragma once
#include <math.h>

#include "yuv_samples.h"

namespace {

struct sdr_pixel {      // clip8 of each accumulator
    __device__ __forceinline__ void operator()(const depth& d, int ar, int ag, int ab, unsigned& r, unsigned& g, unsigned& b) const {
        r = clip_down(d, ar); g = clip_down(d, ag); b = clip_down(d, ab);
    }
};

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

// the table (2^bits floats) into LDS, once per block of 256 threads
__device__ __forceinline__ void stage_hdr_lut(float* lut, const tdc_hdr_desc& h, int bits) {
    for (int i = threadIdx.x; i < 1 << bits; i += 256) lut[i] = h.lut[i];
    __syncthreads();
}

// everything tdc_yuv_hdr_to_rgb refuses about the descriptor, before any launch
inline bool hdr_desc_ok(const tdc_hdr_desc* h) {
    if (!h || !h->lut || !aligned(h->lut, 4)) return false;
    bool finite = isfinite(h->ootf_scale) && isfinite(h->ootf_exp) && isfinite(h->inv_p2);
    for (float v : h->luma) finite = finite && isfinite(v);
    for (float v : h->gamut) finite = finite && isfinite(v);
    if (!finite) return false;
    if (!(h->inv_p2 > 0.0f && h->inv_p2 <= 1.0f) || !(h->ootf_exp >= 0.0f && h->ootf_exp < 1.0f)) return false;
    if (h->ootf_exp != 0.0f && !(h->ootf_scale > 0.0f)) return false;
    return true;
}

}  // namespace
