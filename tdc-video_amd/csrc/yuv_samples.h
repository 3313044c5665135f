// What the YUV -> RGB kernels share.  On the device: the sample extraction of DESIGN.md section 20 (bytes, or little-endian
// 16-bit words with the sample masked out of either end), the integer accumulators of the stated formula with the clamp taken
// before the shift, and the planar kernel body in pieces - which thread owns which pixels (yuv_unit_of), how it loads its run
// of chroma samples (chroma_run) and how a pixel row is loaded and stored (emit_row) - under yuv_frames (replicated chroma:
// yuv_planes.hip, yuv_hdr.hip) and yuv_linear_frames (yuv_linear.hip), with what a pixel's three accumulators become as a
// functor.  On the host, for every planar entry (tdc_yuv420_to_rgb of yuv.hip included): the refusals of a tdc_yuv_planes /
// tdc_yuv_coef pair, the choice between the one-sample form and the 8-pixel vector form from alignment facts alone, the grid
// every kernel of the family takes (stream_grid) and the run-time form as a template argument (with_form).
#pragma once
#include <type_traits>

#include "common.h"
#include "../../include/tdc_hip.h"

namespace {

enum { WORD = 0, VEC_PLANAR = 1, VEC_PAIRED = 2 };

// what the bit depth fixes, computed once per thread from the descriptor
struct depth {
    int shift;       // word -> sample: 16 - bits for MSB-aligned words, else 0
    unsigned mask;   // 2^bits - 1
    int mid;         // 2^(bits - 1)
    int round;       // 2^(down - 1)
    int top;         // 2^(16 + bits) - 1: the accumulators whose floor shift is in [0, 2^(16 + bits - down) - 1] are exactly [0, top]
    int down;        // 16 + s for 8-bit results (s = bits - 8), 16 for results at the samples' depth
};

// out_bits: 8 (RGB bytes) or p.bits (codes at full depth)
__device__ __forceinline__ depth depth_of(int bits, int msb_aligned, int out_bits) {
    const int down = 16 + bits - out_bits;
    return {msb_aligned ? 16 - bits : 0, (1u << bits) - 1u, 1 << (bits - 1), 1 << (down - 1), (1 << (16 + bits)) - 1, down};
}
__device__ __forceinline__ depth depth_of(const tdc_yuv_planes& p, int out_bits) { return depth_of(p.bits, p.msb_aligned, out_bits); }

struct chroma_terms { int r, g, b; };   // the chroma part of each channel's accumulator, rounding term included

__device__ __forceinline__ chroma_terms chroma(const tdc_yuv_coef& c, const depth& d, int u, int v) {
    const int cb = u - d.mid, cr = v - d.mid;
    return {c.crv * cr + d.round, -c.cgu * cb - c.cgv * cr + d.round, c.cbu * cb + d.round};
}

// clip(acc >> down), the clamp taken on the accumulator and the shift after it (NOTES.md section 3, item 13)
__device__ __forceinline__ unsigned clip_down(const depth& d, int acc) {
    const int v = acc < 0 ? 0 : (acc > d.top ? d.top : acc);
    return (unsigned)v >> d.down;
}

// N bytes (4, 8, 16 or 32) from an address aligned to min(N, 16), as 32-bit words
template <int N>
__device__ __forceinline__ void load_words(const unsigned char* p, unsigned (&w)[N / 4]) {
    if constexpr (N == 4) {
        w[0] = *reinterpret_cast<const unsigned*>(p);
    } else if constexpr (N == 8) {
        const uint2 a = *reinterpret_cast<const uint2*>(p);
        w[0] = a.x; w[1] = a.y;
    } else {
#pragma unroll
        for (int k = 0; k < N / 16; ++k) {
            const uint4 a = reinterpret_cast<const uint4*>(p)[k];
            w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w;
        }
    }
}

// sample i of a run of samples held in words: BS = 1 bytes, BS = 2 little-endian 16-bit words
template <int BS, int NW>
__device__ __forceinline__ int sample(const unsigned (&w)[NW], int i, const depth& d) {
    if constexpr (BS == 1) return (int)(w[i >> 2] >> (8 * (i & 3)) & 255u);
    else return (int)((w[i >> 1] >> (16 * (i & 1)) & 0xffffu) >> d.shift & d.mask);
}

template <int BS>
__device__ __forceinline__ int sample_at(const unsigned char* p, const depth& d) {
    if constexpr (BS == 1) return (int)*p;
    else return (int)((unsigned)*reinterpret_cast<const unsigned short*>(p) >> d.shift & d.mask);
}

// four pixels = 12 bytes = three words, twice: eight pixels of one row as three 8-byte words
__device__ __forceinline__ void pack_row8(const unsigned* r, const unsigned* g, const unsigned* b, uint2 (&o)[3]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = 4 * h;
        const unsigned w0 = r[i] | g[i] << 8 | b[i] << 16 | r[i + 1] << 24;
        const unsigned w1 = g[i + 1] | b[i + 1] << 8 | r[i + 2] << 16 | g[i + 2] << 24;
        const unsigned w2 = b[i + 2] | r[i + 3] << 8 | g[i + 3] << 16 | b[i + 3] << 24;
        if (h == 0) { o[0].x = w0; o[0].y = w1; o[1].x = w2; }
        else { o[1].y = w0; o[2].x = w1; o[2].y = w2; }
    }
}

// eight pixels of one row: their luma samples in words, the chroma terms of their 8 >> SUBX samples -> three 8-byte words
template <int BS, int SUBX, class PX>
__device__ __forceinline__ void row8(const tdc_yuv_coef& c, const depth& d, const PX& px, const unsigned (&lw)[2 * BS],
                                     const chroma_terms (&ct)[8 >> SUBX], uint2 (&o)[3]) {
    unsigned r[8], g[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int yy = c.cy * (sample<BS>(lw, i, d) - c.y_off);
        const chroma_terms& k = ct[i >> SUBX];
        px(d, yy + k.r, yy + k.g, yy + k.b, r[i], g[i], b[i]);
    }
    pack_row8(r, g, b, o);
}

// The walk every planar kernel takes.  grid: x strides over the frame's units (a unit = one thread's block; units_x per
// block row, Hc block rows), y strides over the frames:
//     for (int t = blockIdx.y; t < T; t += gridDim.y)
//         for (long long i = first_unit(); i < units; i += unit_stride()) { const yuv_unit n = yuv_unit_of(p, t, i, ...); ... }
// Every index is derived from T, H, W and the strides the host has checked against them.
struct yuv_unit {
    const unsigned char *uf, *vf;   // the frame's chroma planes
    const unsigned char* yr;        // the unit's first luma row
    unsigned char* orow;            // the unit's first output row
    int yc, xu;                     // its chroma row and its place in it
    bool two_rows;                  // 4:2:0 and not the last block of an odd H
};

__device__ __forceinline__ long long first_unit() { return (long long)blockIdx.x * 256 + threadIdx.x; }
__device__ __forceinline__ long long unit_stride() { return (long long)gridDim.x * 256; }

// units per frame: < 2^32, units_x and Hc are at most 65535
__device__ __forceinline__ long long yuv_units(const tdc_yuv_planes& p, int H, int units_x) {
    return (long long)units_x * ((H + p.sub_y) >> p.sub_y);
}

__device__ __forceinline__ yuv_unit yuv_unit_of(const tdc_yuv_planes& p, int t, long long i, int units_x, int H, int W, unsigned char* rgb) {
    const unsigned yc_ = (unsigned)i / (unsigned)units_x;     // i < 2^32: a 32-bit division
    const int yc = (int)yc_, xu = (int)((unsigned)i - yc_ * (unsigned)units_x);
    const int y0 = yc << p.sub_y;
    return {p.u + (long long)t * p.c_frame, p.v + (long long)t * p.c_frame, p.y + (long long)t * p.y_frame + (long long)y0 * p.y_pitch,
            rgb + (long long)t * H * W * 3 + (long long)y0 * W * 3, yc, xu, p.sub_y && y0 + 1 < H};
}

// the NC chroma samples of unit xu in the chroma row at byte offset crow: WORD one sample per load (NC = 1), VEC_PLANAR one
// load per plane, VEC_PAIRED the NC pairs at the lower pointer (u_is_high: the pairs are (v, u))
template <int BS, int NC, int FORM>
__device__ __forceinline__ void chroma_run(const tdc_yuv_planes& p, const unsigned char* uf, const unsigned char* vf, long long crow,
                                           int xu, const depth& d, int u_is_high, int* su, int* sv) {
    if constexpr (FORM == WORD) {
        const long long coff = crow + (long long)xu * p.c_step;
        su[0] = sample_at<BS>(uf + coff, d);
        sv[0] = sample_at<BS>(vf + coff, d);
    } else if constexpr (FORM == VEC_PLANAR) {
        unsigned uw[NC * BS / 4], vw[NC * BS / 4];
        load_words<NC * BS>(uf + crow + (long long)xu * (NC * BS), uw);
        load_words<NC * BS>(vf + crow + (long long)xu * (NC * BS), vw);
#pragma unroll
        for (int k = 0; k < NC; ++k) { su[k] = sample<BS>(uw, k, d); sv[k] = sample<BS>(vw, k, d); }
    } else {
        unsigned pw[2 * NC * BS / 4];
        load_words<2 * NC * BS>((u_is_high ? vf : uf) + crow + (long long)xu * (2 * NC * BS), pw);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int first = sample<BS>(pw, 2 * k, d), second = sample<BS>(pw, 2 * k + 1, d);
            su[k] = u_is_high ? second : first;
            sv[k] = u_is_high ? first : second;
        }
    }
}

// one pixel row of a unit, from its luma row and the chroma terms of its pixels (pixel k takes ct[k >> CSH]) to its bytes:
// WORD its NPX pixels, one sample per load and byte stores below W; the vector forms eight pixels, one luma load and three
// 8-byte stores.  px(d, accR, accG, accB, r, g, b) turns a pixel's three accumulators into its bytes.
template <int BS, int CSH, int FORM, int NPX, class PX>
__device__ __forceinline__ void emit_row(const tdc_yuv_coef& c, const depth& d, const PX& px, const unsigned char* yrow, unsigned char* orow,
                                         int xu, int W, const chroma_terms (&ct)[(FORM == WORD ? NPX : 8) >> CSH]) {
    if constexpr (FORM == WORD) {
        const int x0 = xu * NPX;
#pragma unroll
        for (int dx = 0; dx < NPX; ++dx) {
            if (dx == 1 && x0 + 1 >= W) break;      // odd W: the last column has one pixel
            const int yy = c.cy * (sample_at<BS>(yrow + (long long)(x0 + dx) * BS, d) - c.y_off);
            const chroma_terms& k = ct[dx >> CSH];
            unsigned char* o = orow + (long long)(x0 + dx) * 3;
            unsigned r, g, b;
            px(d, yy + k.r, yy + k.g, yy + k.b, r, g, b);
            o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)b;
        }
    } else {
        unsigned lw[2 * BS];
        uint2 o[3];
        load_words<8 * BS>(yrow + (long long)xu * (8 * BS), lw);
        row8<BS, CSH>(c, d, px, lw, ct, o);
        uint2* dst = reinterpret_cast<uint2*>(orow + 24ll * xu);
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    }
}

// replicated chroma: a thread owns (1 + sub_y) x (1 + SUBX) pixels (WORD) or (1 + sub_y) x 8 (the vector forms), so a chroma
// sample is loaded once
template <int BS, int SUBX, int FORM, class PX>
__device__ __forceinline__ void yuv_frames(const tdc_yuv_planes& p, const tdc_yuv_coef& c, const depth& d, const PX& px, int T, int H,
                                           int W, int units_x, int u_is_high, unsigned char* rgb) {
    constexpr int NC = FORM == WORD ? 1 : 8 >> SUBX;    // chroma samples of the unit's columns
    const long long units = yuv_units(p, H, units_x);
    for (int t = blockIdx.y; t < T; t += gridDim.y)
        for (long long i = first_unit(); i < units; i += unit_stride()) {
            const yuv_unit n = yuv_unit_of(p, t, i, units_x, H, W, rgb);
            int su[NC], sv[NC];
            chroma_run<BS, NC, FORM>(p, n.uf, n.vf, (long long)n.yc * p.c_pitch, n.xu, d, u_is_high, su, sv);
            chroma_terms ct[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) ct[k] = chroma(c, d, su[k], sv[k]);
            emit_row<BS, SUBX, FORM, 1 + SUBX>(c, d, px, n.yr, n.orow, n.xu, W, ct);
            if (n.two_rows) emit_row<BS, SUBX, FORM, 1 + SUBX>(c, d, px, n.yr + p.y_pitch, n.orow + (long long)W * 3, n.xu, W, ct);
        }
}

inline bool aligned(const void* p, unsigned a) { return ((unsigned long long)p & (a - 1)) == 0; }
inline bool multiple(long long v, int a) { return v % a == 0; }

// the coefficient and y_off checks of tdc_yuv_to_rgb at `bits`
inline bool yuv_coef_ok(const tdc_yuv_coef* c, int bits) {
    const int s = bits - 8;
    if (c->y_off != 0 && c->y_off != 16 << s) return false;
    const int coef[5] = {c->cy, c->crv, c->cgu, c->cgv, c->cbu};
    for (int v : coef)
        if (v < 0 || v > (1 << 18)) return false;
    long long cmax = c->crv > c->cbu ? c->crv : c->cbu;
    if ((long long)c->cgu + c->cgv > cmax) cmax = (long long)c->cgu + c->cgv;
    // every accumulator stays inside int32 for every sample value
    if (((long long)c->cy << bits) + (cmax << (bits - 1)) + (1ll << (15 + s)) >= (1ll << 31)) return false;
    return true;
}

// everything tdc_yuv_to_rgb refuses, before any launch
inline bool yuv_args_ok(const tdc_yuv_planes* p, const tdc_yuv_coef* c, int T, int H, int W, const unsigned char* rgb) {
    if (!p || !c || !rgb || !p->y || !p->u || !p->v) return false;
    if (T < 1 || H < 1 || W < 1 || T > 65535 || H > 65535 || W > 65535) return false;
    if (p->bits != 8 && p->bits != 10 && p->bits != 12) return false;
    if (!((p->sub_x == 1 && p->sub_y == 1) || (p->sub_x == 1 && p->sub_y == 0) || (p->sub_x == 0 && p->sub_y == 0))) return false;
    if ((p->msb_aligned != 0 && p->msb_aligned != 1) || (p->msb_aligned && p->bits == 8)) return false;
    const int bs = p->bits == 8 ? 1 : 2;       // bytes per sample
    if (p->c_step != bs && p->c_step != 2 * bs) return false;
    if (bs == 2 && (!aligned(p->y, 2) || !aligned(p->u, 2) || !aligned(p->v, 2) || p->y_pitch % 2 || p->c_pitch % 2 ||
                    p->y_frame % 2 || p->c_frame % 2)) return false;
    const int Hc = (H + p->sub_y) >> p->sub_y, Wc = (W + p->sub_x) >> p->sub_x;
    if (p->y_pitch < W * bs || p->c_pitch < p->c_step * Wc) return false;
    // a frame stride must clear the plane's last row (it is used only between frames)
    if (T > 1 && (p->y_frame < (long long)(H - 1) * p->y_pitch + W * bs ||
                  p->c_frame < (long long)(Hc - 1) * p->c_pitch + p->c_step * (Wc - 1) + bs)) return false;
    return yuv_coef_ok(c, p->bits);
}

// the grid of every kernel of the family, blocks of 256 threads over `units` units per frame and T frames.  Memory-bound:
// about eight blocks per CU in flight, the rest by striding
inline dim3 stream_grid(long long units, int T) {
    const int gx = (int)((units + 255) / 256 < 2048 ? (units + 255) / 256 : 2048);
    const int gy = T < 2048 / gx ? T : (2048 / gx > 1 ? 2048 / gx : 1);
    return dim3(gx, gy);
}

// the run-time form as a template argument: f(std::integral_constant<int, FORM>())
template <class F>
void with_form(int form, const F& f) {
    if (form == WORD) f(std::integral_constant<int, WORD>());
    else if (form == VEC_PLANAR) f(std::integral_constant<int, VEC_PLANAR>());
    else f(std::integral_constant<int, VEC_PAIRED>());
}

struct yuv_launch { int form, u_is_high, units_x; dim3 grid; };

// the vector form: every luma load, chroma load and RGB store lands on its own alignment in every row of every frame
inline yuv_launch yuv_launch_of(const tdc_yuv_planes* p, int T, int H, int W, const unsigned char* rgb) {
    const int bs = p->bits == 8 ? 1 : 2;
    const int Hc = (H + p->sub_y) >> p->sub_y, Wc = (W + p->sub_x) >> p->sub_x;
    int form = WORD, u_is_high = 0;
    const int lb = 8 * bs, nc = 8 >> p->sub_x;
    if (W % 8 == 0 && aligned(p->y, lb) && multiple(p->y_pitch, lb) && (T == 1 || multiple(p->y_frame, lb)) && aligned(rgb, 8)) {
        if (p->c_step == bs) {
            const int a = nc * bs;
            if (aligned(p->u, a) && aligned(p->v, a) && multiple(p->c_pitch, a) && (T == 1 || multiple(p->c_frame, a)))
                form = VEC_PLANAR;
        } else if (p->v == p->u + bs || p->u == p->v + bs) {
            u_is_high = p->u > p->v;
            const int a = 2 * nc * bs < 16 ? 2 * nc * bs : 16;
            if (aligned(u_is_high ? p->v : p->u, a) && multiple(p->c_pitch, a) && (T == 1 || multiple(p->c_frame, a)))
                form = VEC_PAIRED;
        }
    }
    const int units_x = form == WORD ? Wc : W / 8;
    return {form, u_is_high, units_x, stream_grid((long long)units_x * Hc, T)};
}

}  // namespace
