// YUV 4:2:0 -> RGB on the device: what stands between a decoder's surfaces (NV12 / NV21 from a
// hardware decoder, planar I420 from a software one) and the uint8 [T, H, W, 3] frames tdc_preprocess_frames takes.  The
// conversion is the stated 16.16 fixed-point formula of include/tdc_hip.h with replicated chroma, not any library's.
// HBM-bound byte work: 1.5 bytes read and 3 written per pixel.  A thread owns a block two rows high, so a chroma sample is
// loaded once for its 2 x 2 pixels.  Two forms of ONE kernel, chosen on the host from alignment facts alone:
//   SCALAR  2 x 2 pixels per thread, byte loads and stores: any width, any pitch, any pointer
//   VEC     2 x 8 pixels per thread: 8-byte luma loads, 4-byte (planar) or 8-byte (interleaved) chroma loads, three 8-byte
//           stores per row.  The interleaved form reads the u / v pairs in one load from the lower of the two pointers.
// The layouts differ only in the two chroma pointers and the byte step between samples; both forms give the same bytes.
#include "common.h"
#include "../../include/tdc_hip.h"

namespace {

enum { SCALAR = 0, VEC_PLANAR = 1, VEC_PAIRED = 2 };

struct chroma_terms { int r, g, b; };   // the chroma part of each channel's accumulator, rounding term included

__device__ __forceinline__ chroma_terms chroma(const tdc_yuv_coef& c, int u, int v) {
    const int cb = u - 128, cr = v - 128;
    return {c.crv * cr + 32768, -c.cgu * cb - c.cgv * cr + 32768, c.cbu * cb + 32768};
}

// clip8(acc >> 16), with the clamp taken on the accumulator: [0, 2^24) holds exactly the values whose floor shift is in
// [0, 255], and the result is then byte 2 of the clamped word.  (Shift first, clamp after gave wrong bytes in the 8-pixel
// form: NOTES.md section 3, item 13.)
__device__ __forceinline__ unsigned clip8(int acc) {
    const int v = acc < 0 ? 0 : (acc > 0xffffff ? 0xffffff : acc);
    return (unsigned)v >> 16;
}

// eight pixels of one row: luma bytes in (lo, hi), chroma terms of the four samples -> 24 bytes as three 8-byte words
__device__ __forceinline__ void row8(const tdc_yuv_coef& c, unsigned lo, unsigned hi, const chroma_terms (&ct)[4], uint2 (&o)[3]) {
    unsigned r[8], g[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int yy = c.cy * ((int)(((i < 4 ? lo : hi) >> (8 * (i & 3))) & 255u) - c.y_off);
        const chroma_terms& k = ct[i >> 1];
        r[i] = clip8(yy + k.r); g[i] = clip8(yy + k.g); b[i] = clip8(yy + k.b);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // four pixels = 12 bytes = three words
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
            if (FORM == SCALAR) {
                const int x0 = 2 * xu;
                const bool two_cols = x0 + 1 < W;   // odd W: the last column has one pixel
                const chroma_terms k = chroma(c, uf[crow + (long long)xu * p.c_step], vf[crow + (long long)xu * p.c_step]);
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    if (dy == 1 && !two_rows) break;
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        if (dx == 1 && !two_cols) break;
                        const int yy = c.cy * ((int)yr[(long long)dy * p.y_pitch + x0 + dx] - c.y_off);
                        unsigned char* o = orow + ((long long)dy * W + x0 + dx) * 3;
                        o[0] = (unsigned char)clip8(yy + k.r);
                        o[1] = (unsigned char)clip8(yy + k.g);
                        o[2] = (unsigned char)clip8(yy + k.b);
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
                for (int s = 0; s < 4; ++s) ct[s] = chroma(c, (int)(ub >> (8 * s) & 255u), (int)(vb >> (8 * s) & 255u));
                const uint2 l0 = *reinterpret_cast<const uint2*>(yr + 8 * xu);
                uint2 l1 = l0;
                if (two_rows) l1 = *reinterpret_cast<const uint2*>(yr + p.y_pitch + 8 * xu);
                uint2 o[3];
                row8(c, l0.x, l0.y, ct, o);
                uint2* d = reinterpret_cast<uint2*>(orow + 24 * xu);
                d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
                if (two_rows) {
                    row8(c, l1.x, l1.y, ct, o);
                    d = reinterpret_cast<uint2*>(orow + (long long)W * 3 + 24 * xu);
                    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
                }
            }
        }
    }
}

inline bool aligned(const void* p, unsigned a) { return ((unsigned long long)p & (a - 1)) == 0; }
inline bool multiple(long long v, int a) { return v % a == 0; }

}  // namespace

extern "C" int tdc_yuv420_to_rgb(const tdc_yuv420_planes* p, const tdc_yuv_coef* c, int T, int H, int W,
                                 unsigned char* rgb, void* stream) {
    if (!p || !c || !rgb || !p->y || !p->u || !p->v) return TDC_E_BADARG;
    if (T < 1 || H < 1 || W < 1 || T > 65535 || H > 65535 || W > 65535) return TDC_E_BADARG;
    if (p->c_step != 1 && p->c_step != 2) return TDC_E_BADARG;
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    if (p->y_pitch < W || p->c_pitch < p->c_step * Wc) return TDC_E_BADARG;
    // a frame stride must clear the plane's last row (it is used only between frames)
    if (T > 1 && (p->y_frame < (long long)(H - 1) * p->y_pitch + W ||
                  p->c_frame < (long long)(Hc - 1) * p->c_pitch + p->c_step * (Wc - 1) + 1)) return TDC_E_BADARG;
    if (c->y_off != 0 && c->y_off != 16) return TDC_E_BADARG;
    const int coef[5] = {c->cy, c->crv, c->cgu, c->cgv, c->cbu};
    for (int v : coef)
        if (v < 0 || v > (1 << 18)) return TDC_E_BADARG;   // |accumulator| < 2^28 for every input byte

    // the vector form: every 8-byte luma load, chroma load and RGB store lands on its own alignment in every row of every frame
    int form = SCALAR, u_is_high = 0;
    if (W % 8 == 0 && aligned(p->y, 8) && multiple(p->y_pitch, 8) && (T == 1 || multiple(p->y_frame, 8)) && aligned(rgb, 8)) {
        if (p->c_step == 1) {
            if (aligned(p->u, 4) && aligned(p->v, 4) && multiple(p->c_pitch, 4) && (T == 1 || multiple(p->c_frame, 4)))
                form = VEC_PLANAR;
        } else if (p->v == p->u + 1 || p->u == p->v + 1) {
            u_is_high = p->u > p->v;
            if (aligned(u_is_high ? p->v : p->u, 8) && multiple(p->c_pitch, 8) && (T == 1 || multiple(p->c_frame, 8)))
                form = VEC_PAIRED;
        }
    }
    const int units_x = form == SCALAR ? Wc : W / 8;
    const long long units = (long long)units_x * Hc;
    // memory-bound: about eight blocks per CU in flight, the rest by striding
    const int gx = (int)((units + 255) / 256 < 2048 ? (units + 255) / 256 : 2048);
    const int gy = T < 2048 / gx ? T : (2048 / gx > 1 ? 2048 / gx : 1);
    const dim3 grid(gx, gy), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (form == SCALAR) hipLaunchKernelGGL(yuv420_to_rgb_kernel<SCALAR>, grid, block, 0, st, *p, *c, T, H, W, units_x, 0, rgb);
    else if (form == VEC_PLANAR) hipLaunchKernelGGL(yuv420_to_rgb_kernel<VEC_PLANAR>, grid, block, 0, st, *p, *c, T, H, W, units_x, 0, rgb);
    else hipLaunchKernelGGL(yuv420_to_rgb_kernel<VEC_PAIRED>, grid, block, 0, st, *p, *c, T, H, W, units_x, u_is_high, rgb);
    return (int)hipGetLastError();
}
