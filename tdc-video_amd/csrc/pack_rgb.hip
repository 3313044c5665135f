// Decoded pictures in the layouts decoders and capture write - channel-first planes, B G R order, 4-byte pixels with an
// alpha or padding byte, one gray plane, a row pitch, a crop - to the packed R G B frames tdc_preprocess_frames takes
// (DESIGN.md section 24).  A permutation (gray: a replication) of bytes, exact by construction:
//   O[t, y, x, c] = src[t*fs + y*rs + x*ps + chan[c]]          O uint8 [T, H, W, 3] contiguous, c = 0, 1, 2 (R, G, B)
// HBM-bound byte work modelled on orient.hip's row-keeping kernel: no LDS, blockIdx.y over the frames, 64-bit offsets.
//   PLANAR   (ps == 1)               a thread moves four consecutive pixels: one 4-byte load per distinct channel offset (one
//                                    for gray), 12 bytes stored as three words
//   INTER4   (ps == 4, chan < 4)     four pixels as four aligned words (V16: as one 16-byte load), 12 bytes stored
//   INTER3   (ps == 3, chan < 3)     12 bytes loaded as three words, the channels permuted in registers, 12 bytes stored
//   BYTE                             a thread moves one pixel as three bytes; takes any descriptor
// The host picks a word form from facts of the descriptor alone: W is a multiple of 4 (so every destination row starts on a
// word when dst does, and a row is whole groups), dst, the source pointer plus each channel offset (PLANAR) or the source
// pointer (INTER3 / INTER4), the row stride and the frame stride are multiples of 4 (of 16 for V16).  Everything else takes the
// BYTE form for the launch.  The forms move the same bytes to the same places.
// A planar form of sixteen pixels per thread (16-byte loads, three 16-byte stores 48 bytes apart between lanes) was measured
// and lost to PLANAR: NOTES.md section 20.
#include "common.h"
#include "../../include/tdc_hip.h"

namespace {

enum { THREADS = 256 };
enum Form { PLANAR, INTER4, INTER4_V16, INTER3, BYTE };

struct w3 { unsigned a, b, c; };    // twelve bytes: four packed pixels; 4-byte aligned
struct __align__(16) w4 { unsigned a, b, c, d; };     // sixteen bytes: four 4-byte pixels; loaded whole where 16-byte aligned

struct source {                      // tdc_rgb_source as the kernels take it
    const unsigned char* src;
    long long fs, rs, ps;
    long long c0, c1, c2;
};

// four pixels, each in the low bytes of a word, the R, G, B sample of a pixel s0, s1, s2 bits up -> the twelve packed bytes
__device__ __forceinline__ w3 pack4(unsigned p0, unsigned p1, unsigned p2, unsigned p3, int s0, int s1, int s2) {
    w3 o;
    o.a = ((p0 >> s0) & 255u) | ((p0 >> s1) & 255u) << 8 | ((p0 >> s2) & 255u) << 16 | ((p1 >> s0) & 255u) << 24;
    o.b = ((p1 >> s1) & 255u) | ((p1 >> s2) & 255u) << 8 | ((p2 >> s0) & 255u) << 16 | ((p2 >> s1) & 255u) << 24;
    o.c = ((p2 >> s2) & 255u) | ((p3 >> s0) & 255u) << 8 | ((p3 >> s1) & 255u) << 16 | ((p3 >> s2) & 255u) << 24;
    return o;
}

// the R, G and B samples of four consecutive pixels, one word per channel -> the twelve packed bytes
__device__ __forceinline__ w3 interleave4(unsigned r, unsigned g, unsigned b) {
    w3 o;
    o.a = (r & 255u) | (g & 255u) << 8 | (b & 255u) << 16 | (r >> 8 & 255u) << 24;
    o.b = (g >> 8 & 255u) | (b >> 8 & 255u) << 8 | (r >> 16 & 255u) << 16 | (g >> 16 & 255u) << 24;
    o.c = (b >> 16 & 255u) | (r >> 24) << 8 | (g >> 24) << 16 | (b >> 24) << 24;
    return o;
}

// pixels a thread moves
constexpr int unit_of(int form) { return form == BYTE ? 1 : 4; }

// grid: x over the frame's units (H rows of W / unit_of(FORM) groups of pixels), y over the frames
template <int FORM>
__global__ __launch_bounds__(THREADS) void pack_rgb_kernel(source s, int T, int H, int W, unsigned char* __restrict__ dst) {
    const int per_row = W / unit_of(FORM);
    const long long units = (long long)H * per_row;
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= units) return;
    const int y = (int)(i / per_row), g = (int)(i - (long long)y * per_row);
    const int x = unit_of(FORM) * g;
    const long long row = (long long)W * 3, frame = (long long)H * row;
    const long long at = y * s.rs + x * s.ps;           // of the unit's first pixel in its frame
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const unsigned char* p = s.src + t * s.fs + at;
        unsigned char* d = dst + t * frame + y * row + (long long)x * 3;
        if (FORM == BYTE) {
            const unsigned char r = p[s.c0], gg = p[s.c1], b = p[s.c2];
            d[0] = r; d[1] = gg; d[2] = b;
        } else if (FORM == PLANAR) {
            const unsigned r = *reinterpret_cast<const unsigned*>(p + s.c0);
            const unsigned gg = s.c1 == s.c0 ? r : *reinterpret_cast<const unsigned*>(p + s.c1);
            const unsigned b = s.c2 == s.c0 ? r : (s.c2 == s.c1 ? gg : *reinterpret_cast<const unsigned*>(p + s.c2));
            *reinterpret_cast<w3*>(d) = interleave4(r, gg, b);
        } else if (FORM == INTER3) {
            const w3 w = *reinterpret_cast<const w3*>(p);
            *reinterpret_cast<w3*>(d) = pack4(w.a, w.a >> 24 | w.b << 8, w.b >> 16 | w.c << 16, w.c >> 8,
                                              8 * (int)s.c0, 8 * (int)s.c1, 8 * (int)s.c2);
        } else {
            w4 w;
            if (FORM == INTER4_V16) {
                w = *reinterpret_cast<const w4*>(p);
            } else {
                const unsigned* q = reinterpret_cast<const unsigned*>(p);
                w.a = q[0]; w.b = q[1]; w.c = q[2]; w.d = q[3];
            }
            *reinterpret_cast<w3*>(d) = pack4(w.a, w.b, w.c, w.d, 8 * (int)s.c0, 8 * (int)s.c1, 8 * (int)s.c2);
        }
    }
}

inline bool multiple(unsigned long long v, unsigned long long m) { return (v & (m - 1)) == 0; }

const long long STRIDE_MAX = 1ll << 40;

}  // namespace

extern "C" int tdc_pack_rgb(const tdc_rgb_source* s, int T, int H, int W, unsigned char* dst, void* stream) {
    if (!s || !s->src || !dst) return TDC_E_BADARG;
    if (T < 1 || H < 1 || W < 1 || T > 65535 || H > 65535 || W > 65535) return TDC_E_BADARG;
    const long long fs = s->frame_stride, rs = s->row_stride, ps = s->pixel_stride;
    const long long c0 = s->chan[0], c1 = s->chan[1], c2 = s->chan[2];
    for (long long v : {fs, rs, ps, c0, c1, c2})
        if (v < 0 || v > STRIDE_MAX) return TDC_E_BADARG;
    const long long cmin = c0 < c1 ? (c0 < c2 ? c0 : c2) : (c1 < c2 ? c1 : c2);
    const long long cmax = c0 > c1 ? (c0 > c2 ? c0 : c2) : (c1 > c2 ? c1 : c2);
    const bool grouped = (ps == 3 || ps == 4) && cmax < ps;      // a pixel's samples lie inside its group of ps bytes
    // the source extent: from the first sample to the last byte of the last pixel's sample or group; every term < 2^56
    const unsigned long long last = (unsigned long long)((T - 1) * fs + (H - 1) * rs + (W - 1) * ps + (grouped ? ps - 1 : cmax));
    const unsigned long long n = 3ull * (unsigned long long)T * (unsigned long long)H * (unsigned long long)W;   // < 2^50
    const unsigned long long a = (unsigned long long)s->src + (unsigned long long)cmin, a_end = (unsigned long long)s->src + last + 1;
    const unsigned long long b = (unsigned long long)dst;
    if (a < b + n && b < a_end) return TDC_E_BADARG;       // the ranges overlap
    const unsigned long long p = (unsigned long long)s->src;
    // a stride that no address is formed with (one frame, one row) decides nothing
    const unsigned long long strides = (T > 1 ? (unsigned long long)fs : 0) | (H > 1 ? (unsigned long long)rs : 0);
    const bool words = W % 4 == 0 && multiple(b, 4) && multiple(strides, 4);
    int form = BYTE;
    if (words && ps == 1 && multiple((p + c0) | (p + c1) | (p + c2), 4)) form = PLANAR;
    else if (words && ps == 4 && grouped && multiple(p, 4)) form = multiple(p | strides, 16) ? INTER4_V16 : INTER4;
    else if (words && ps == 3 && grouped && multiple(p, 4)) form = INTER3;
    const source k = {s->src, fs, rs, ps, c0, c1, c2};
    hipStream_t st = (hipStream_t)stream;
    const long long units = (long long)H * (W / unit_of(form));      // < 2^32
    const dim3 grid((unsigned)((units + THREADS - 1) / THREADS), T), block(THREADS);     // <= 2^24 x 65535
    switch (form) {
        case PLANAR: hipLaunchKernelGGL(pack_rgb_kernel<PLANAR>, grid, block, 0, st, k, T, H, W, dst); break;
        case INTER4: hipLaunchKernelGGL(pack_rgb_kernel<INTER4>, grid, block, 0, st, k, T, H, W, dst); break;
        case INTER4_V16: hipLaunchKernelGGL(pack_rgb_kernel<INTER4_V16>, grid, block, 0, st, k, T, H, W, dst); break;
        case INTER3: hipLaunchKernelGGL(pack_rgb_kernel<INTER3>, grid, block, 0, st, k, T, H, W, dst); break;
        default: hipLaunchKernelGGL(pack_rgb_kernel<BYTE>, grid, block, 0, st, k, T, H, W, dst);
    }
    return (int)hipGetLastError();
}
