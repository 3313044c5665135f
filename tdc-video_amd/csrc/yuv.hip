// YUV 4:2:0 -> RGB on the device: NV12 / NV21 from a hardware decoder, planar I420 from a software
// one -> the uint8 [T, H, W, 3] frames tdc_preprocess_frames takes.  tdc_yuv420_to_rgb is tdc_yuv_to_rgb (yuv_planes.hip) at
// bits = 8, 4:2:0: the refusals (yuv_args_ok), the choice of form and the grid (yuv_launch_of) are that entry's, through
// yuv_samples.h, and so are the chroma terms and the clamp (at the constant depth of bytes).  What stays here is the kernel:
// the body of yuv_frames<1, 1, FORM> written out for bytes - 32-bit unit indices, both luma rows loaded before the first
// store - instruction for instruction the kernel this entry has always had.  The NV12 launch through the shared body
// measured slower than this one by more than two runs of this one differed (profiles/yuv_kernel_family.json).
//   WORD    2 x 2 pixels per thread, byte loads and stores: any width, any pitch, any pointer
//   VEC     2 x 8 pixels per thread: 8-byte luma loads, 4-byte (planar) or 8-byte (interleaved) chroma loads, three 8-byte
//           stores per row.  The interleaved form reads the u / v pairs in one load from the lower of the two pointers.
// The layouts differ only in the two chroma pointers and the byte step between samples; both forms give the same bytes,
// which are tdc_yuv_to_rgb's (tests/test_hip_yuv_hibit_inputs.py).
#include "yuv_samples.h"

namespace {

// eight pixels of one row: luma bytes in (lo, hi), chroma terms of the four samples -> 24 bytes as three 8-byte words
__device__ __forceinline__ void row8(const tdc_yuv_coef& c, const depth& d, unsigned lo, unsigned hi, const chroma_terms (&ct)[4],
                                     uint2 (&o)[3]) {
    unsigned r[8], g[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int yy = c.cy * ((int)(((i < 4 ? lo : hi) >> (8 * (i & 3))) & 255u) - c.y_off);
        const chroma_terms& k = ct[i >> 1];
        r[i] = clip_down(d, yy + k.r); g[i] = clip_down(d, yy + k.g); b[i] = clip_down(d, yy + k.b);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // pack_row8 of yuv_samples.h, written out: the instructions of this kernel stay what they were
        const int i = 4 * h;
        const unsigned w0 = r[i] | g[i] << 8 | b[i] << 16 | r[i + 1] << 24;
        const unsigned w1 = g[i + 1] | b[i + 1] << 8 | r[i + 2] << 16 | g[i + 2] << 24;
        const unsigned w2 = b[i + 2] | r[i + 3] << 8 | g[i + 3] << 16 | b[i + 3] << 24;
        if (h == 0) { o[0].x = w0; o[0].y = w1; o[1].x = w2; }
        else { o[1].y = w0; o[2].x = w1; o[2].y = w2; }
    }
}

// grid: x strides over the frame's units (a unit = one thread's block; units_x per block row, Hc block rows), y strides
// over the frames.  Every index is derived from T, H, W and the strides the host has checked against them.
template <int FORM>
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(tdc_yuv420_planes p, tdc_yuv_coef c, int T, int H, int W,
                                                            int units_x, int u_is_high, unsigned char* rgb) {
    const depth d8 = depth_of(8, 0, 8);      // constants: the chroma terms and the clamp are yuv_samples.h's at 8 bits
    const int Hc = (H + 1) >> 1;
    const int units = units_x * Hc;     // <= 32768 * 32768: fits an int
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const unsigned char* yf = p.y + (long long)t * p.y_frame;
        const unsigned char* uf = p.u + (long long)t * p.c_frame;
        const unsigned char* vf = p.v + (long long)t * p.c_frame;
        unsigned char* of = rgb + (long long)t * H * W * 3;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < units; i += gridDim.x * 256) {   // < 2^30 + 2^19
            const int yc = i / units_x, xu = i - yc * units_x;
            const int y0 = 2 * yc;
            const bool two_rows = y0 + 1 < H;   // odd H: the last block has one row
            const unsigned char* yr = yf + (long long)y0 * p.y_pitch;
            const long long crow = (long long)yc * p.c_pitch;
            unsigned char* orow = of + (long long)y0 * W * 3;
            if (FORM == WORD) {
                const int x0 = 2 * xu;
                const bool two_cols = x0 + 1 < W;   // odd W: the last column has one pixel
                const chroma_terms k = chroma(c, d8, uf[crow + (long long)xu * p.c_step], vf[crow + (long long)xu * p.c_step]);
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    if (dy == 1 && !two_rows) break;
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        if (dx == 1 && !two_cols) break;
                        const int yy = c.cy * ((int)yr[(long long)dy * p.y_pitch + x0 + dx] - c.y_off);
                        unsigned char* o = orow + ((long long)dy * W + x0 + dx) * 3;
                        o[0] = (unsigned char)clip_down(d8, yy + k.r);
                        o[1] = (unsigned char)clip_down(d8, yy + k.g);
                        o[2] = (unsigned char)clip_down(d8, yy + k.b);
                    }
                }
            } else {
                unsigned ub, vb;    // four u and four v bytes
                if (FORM == VEC_PLANAR) {
                    ub = *reinterpret_cast<const unsigned*>(uf + crow + 4 * xu);
                    vb = *reinterpret_cast<const unsigned*>(vf + crow + 4 * xu);
                } else {            // four pairs in eight bytes at the lower pointer; u_is_high: the pairs are (v, u)
                    const uint2 w = *reinterpret_cast<const uint2*>((u_is_high ? vf : uf) + crow + 8 * xu);
                    const unsigned even = (w.x & 255u) | (w.x >> 8 & 0xff00u) | (w.y << 16 & 0xff0000u) | (w.y << 8 & 0xff000000u);
                    const unsigned odd = (w.x >> 8 & 255u) | (w.x >> 16 & 0xff00u) | (w.y << 8 & 0xff0000u) | (w.y & 0xff000000u);
                    ub = u_is_high ? odd : even;
                    vb = u_is_high ? even : odd;
                }
                chroma_terms ct[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) ct[s] = chroma(c, d8, (int)(ub >> (8 * s) & 255u), (int)(vb >> (8 * s) & 255u));
                const uint2 l0 = *reinterpret_cast<const uint2*>(yr + 8 * xu);
                uint2 l1 = l0;
                if (two_rows) l1 = *reinterpret_cast<const uint2*>(yr + p.y_pitch + 8 * xu);
                uint2 o[3];
                row8(c, d8, l0.x, l0.y, ct, o);
                uint2* d = reinterpret_cast<uint2*>(orow + 24 * xu);
                d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
                if (two_rows) {
                    row8(c, d8, l1.x, l1.y, ct, o);
                    d = reinterpret_cast<uint2*>(orow + (long long)W * 3 + 24 * xu);
                    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
                }
            }
        }
    }
}

}  // namespace

extern "C" int tdc_yuv420_to_rgb(const tdc_yuv420_planes* p, const tdc_yuv_coef* c, int T, int H, int W,
                                 unsigned char* rgb, void* stream) {
    if (!p) return TDC_E_BADARG;
    const tdc_yuv_planes q = {p->y, p->u, p->v, p->y_frame, p->c_frame, p->y_pitch, p->c_pitch, p->c_step, 8, 0, 1, 1};
    if (!yuv_args_ok(&q, c, T, H, W, rgb)) return TDC_E_BADARG;
    const yuv_launch l = yuv_launch_of(&q, T, H, W, rgb);
    with_form(l.form, [&](auto form) {
        hipLaunchKernelGGL(yuv420_to_rgb_kernel<decltype(form)::value>, l.grid, dim3(256), 0, (hipStream_t)stream, *p, *c, T, H, W,
                           l.units_x, l.u_is_high, rgb);
    });
    return (int)hipGetLastError();
}
