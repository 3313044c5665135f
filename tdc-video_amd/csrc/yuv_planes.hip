// YUV -> RGB for planar and semi-planar surfaces (DESIGN.md sections 19 and 20): 8, 10 or 12 significant bits (bytes, or
// little-endian 16-bit words aligned to either end), 4:2:0, 4:2:2 or 4:4:4, planar or interleaved chroma in either order.
// tdc_yuv420_to_rgb (NV12 / NV21 / I420, yuv.hip) is tdc_yuv_to_rgb at bits = 8, 4:2:0 on the host - the same refusals, choice
// of form and grid, through yuv_samples.h - in front of a kernel of its own.  The conversion is the stated fixed-point
// formula of include/tdc_hip.h, section 19's with s = bits - 8 more bits in the samples, the rounding term and the shift;
// replicated chroma; no library's converter and no transfer function.
// HBM-bound sample work: a thread owns a block (1 + sub_y) rows high, so a chroma sample is loaded once.  Two forms of ONE
// kernel, chosen on the host from alignment facts alone:
//   WORD    (1 + sub_y) x (1 + sub_x) pixels per thread, one sample per load, byte stores: any width, any pitch, any view
//   VEC     (1 + sub_y) x 8 pixels per thread: one 8- (bytes) or 16-byte (words) luma load per row, the 8 >> sub_x chroma
//           samples in one load per plane - interleaved: the pairs from the lower of the two pointers, 32 bytes as two
//           16-byte loads - and three 8-byte stores per row.
// Bits of a word outside the sample are masked off before anything else sees them.  Both forms give the same bytes.
#include "yuv_pixels.h"

namespace {

template <int BS, int SUBX, int FORM>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(tdc_yuv_planes p, tdc_yuv_coef c, int T, int H, int W, int units_x,
                                                         int u_is_high, unsigned char* rgb) {
    yuv_frames<BS, SUBX, FORM>(p, c, depth_of(p, 8), sdr_pixel(), T, H, W, units_x, u_is_high, rgb);
}

template <int BS, int SUBX>
void launch(const yuv_launch& l, hipStream_t st, const tdc_yuv_planes& p, const tdc_yuv_coef& c, int T, int H, int W, unsigned char* rgb) {
    with_form(l.form, [&](auto form) {
        hipLaunchKernelGGL((yuv_to_rgb_kernel<BS, SUBX, decltype(form)::value>), l.grid, dim3(256), 0, st, p, c, T, H, W, l.units_x,
                           l.u_is_high, rgb);
    });
}

}  // namespace

extern "C" int tdc_yuv_to_rgb(const tdc_yuv_planes* p, const tdc_yuv_coef* c, int T, int H, int W, unsigned char* rgb,
                              void* stream) {
    if (!yuv_args_ok(p, c, T, H, W, rgb)) return TDC_E_BADARG;
    const yuv_launch l = yuv_launch_of(p, T, H, W, rgb);
    hipStream_t st = (hipStream_t)stream;
    if (p->bits == 8 && p->sub_x == 1) launch<1, 1>(l, st, *p, *c, T, H, W, rgb);
    else if (p->bits == 8) launch<1, 0>(l, st, *p, *c, T, H, W, rgb);
    else if (p->sub_x == 1) launch<2, 1>(l, st, *p, *c, T, H, W, rgb);
    else launch<2, 0>(l, st, *p, *c, T, H, W, rgb);
    return (int)hipGetLastError();
}
