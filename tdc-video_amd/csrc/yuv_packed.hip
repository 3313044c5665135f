// Packed YUV -> RGB: surfaces in which luma and chroma share one row - YUY2 and its three orders, Y210 /
// Y212, AYUV in both orders, Y410, Y412 / Y416 and v210.  What is new is where a sample sits; what a sample becomes is not: the
// depth, the chroma terms and the clamp of yuv_samples.h and the two pixel functors of yuv_pixels.h, so the bytes are those of
// tdc_yuv_to_rgb (h == NULL) or tdc_yuv_hdr_to_rgb on the same samples held in planes.  HBM-bound sample work, no LDS but the
// HDR table.  A row is a run of groups (family: bytes per group, pixels per group); a thread owns one unit of one row:
//   GROUP     one group, loaded sample by sample (bytes, 16-bit words) or word by word (Y410, v210), byte stores: any width,
//             any pitch, any view
//   VEC       eight pixels (v210: 24, four groups) in 16-byte loads, three (nine) 8-byte stores; a v210 row whose width is
//             a multiple of 8 but not of 24 ends in one or two units of one group (one 16-byte load, byte stores)
// chosen on the host from alignment facts alone.  Bits outside a sample are masked off before anything else sees them; every
// form gives the same bytes.
// tdc_yuv_packed_linear_to_rgb is the 4:2:2 families with interpolated chroma.  ONE walk (packed_frames),
// ONE load of a unit's words (load_unit), ONE set of kernels and ONE pair of launchers serve both entries; what a unit is is a
// functor: `replicated` (packed_unit), or `interpolated_x` (packed_linear_unit: the chroma pair left (centred siting) and right
// of the unit's run as well).  The replicate kernels do not pass through the interpolation: their chroma loads are fewer.
#include "yuv_linear.h"
#include "yuv_pixels.h"

namespace {

enum { F422_8 = 0, F422_16 = 1, F444_8 = 2, F444_16 = 3, F410 = 4, FV210 = 5 };     // families
enum { GROUP = 0, VEC = 1 };

constexpr int fam_ss(int f) { return f == F422_8 || f == F444_8 ? 1 : (f == F422_16 || f == F444_16 ? 2 : 4); }   // bytes per load of GROUP
constexpr int fam_gw(int f) { return f == F422_16 || f == F444_16 ? 2 : (f == FV210 ? 4 : 1); }                    // 32-bit words per group
constexpr int fam_px(int f) { return f == F422_8 || f == F422_16 ? 2 : (f == FV210 ? 6 : 1); }                     // pixels per group
constexpr int fam_nc(int f) { return f == FV210 ? 3 : 1; }                                                           // chroma pairs per group

struct packed_lay { int y0, y1, u, v; };    // sample positions inside a group, in samples (bytes or 16-bit words)

// what the format fixes, on the host
struct packed_fmt { int family; packed_lay lay; };

inline bool packed_fmt_of(int format, packed_fmt& f) {
    switch (format) {
        case TDC_YUVP_YUYV: f = {F422_8, {0, 2, 1, 3}}; return true;
        case TDC_YUVP_YVYU: f = {F422_8, {0, 2, 3, 1}}; return true;
        case TDC_YUVP_UYVY: f = {F422_8, {1, 3, 0, 2}}; return true;
        case TDC_YUVP_VYUY: f = {F422_8, {1, 3, 2, 0}}; return true;
        case TDC_YUVP_Y210: f = {F422_16, {0, 2, 1, 3}}; return true;
        case TDC_YUVP_VUYA: f = {F444_8, {2, 2, 1, 0}}; return true;
        case TDC_YUVP_AYUV: f = {F444_8, {1, 1, 2, 3}}; return true;
        case TDC_YUVP_Y410: f = {F410, {0, 0, 0, 0}}; return true;
        case TDC_YUVP_Y416: f = {F444_16, {1, 1, 0, 2}}; return true;
        case TDC_YUVP_V210: f = {FV210, {0, 0, 0, 0}}; return true;
    }
    return false;
}

// one group of a row, from an address aligned to the family's sample or word size -> its 32-bit words
template <int FAM>
__device__ __forceinline__ void load_group(const unsigned char* g, unsigned (&w)[fam_gw(FAM)]) {
    if constexpr (fam_ss(FAM) == 1) {
        w[0] = (unsigned)g[0] | (unsigned)g[1] << 8 | (unsigned)g[2] << 16 | (unsigned)g[3] << 24;
    } else if constexpr (fam_ss(FAM) == 2) {
        const unsigned short* s = reinterpret_cast<const unsigned short*>(g);
#pragma unroll
        for (int k = 0; k < fam_gw(FAM); ++k) w[k] = (unsigned)s[2 * k] | (unsigned)s[2 * k + 1] << 16;
    } else {
        const unsigned* s = reinterpret_cast<const unsigned*>(g);
#pragma unroll
        for (int k = 0; k < fam_gw(FAM); ++k) w[k] = s[k];
    }
}

// 16-bit sample i (0 .. 3, uniform) of a group of two words: sample<2> of yuv_samples.h without indexing registers by a variable
__device__ __forceinline__ int sample16(const unsigned (&w)[2], int i, const depth& d) {
    const unsigned long long g = (unsigned long long)w[1] << 32 | w[0];
    return (int)(((unsigned)(g >> (16 * i)) & 0xffffu) >> d.shift & d.mask);
}

// the samples of one group: its luma samples and its chroma pairs
template <int FAM>
__device__ __forceinline__ void group_samples(const unsigned (&w)[fam_gw(FAM)], const packed_lay& l, const depth& d,
                                              int (&y)[fam_px(FAM)], int (&u)[fam_nc(FAM)], int (&v)[fam_nc(FAM)]) {
    if constexpr (FAM == F422_8) {
        y[0] = (int)(w[0] >> (8 * l.y0) & 255u); y[1] = (int)(w[0] >> (8 * l.y1) & 255u);
        u[0] = (int)(w[0] >> (8 * l.u) & 255u); v[0] = (int)(w[0] >> (8 * l.v) & 255u);
    } else if constexpr (FAM == F444_8) {
        y[0] = (int)(w[0] >> (8 * l.y0) & 255u);
        u[0] = (int)(w[0] >> (8 * l.u) & 255u); v[0] = (int)(w[0] >> (8 * l.v) & 255u);
    } else if constexpr (FAM == F422_16) {
        y[0] = sample16(w, l.y0, d); y[1] = sample16(w, l.y1, d);
        u[0] = sample16(w, l.u, d); v[0] = sample16(w, l.v, d);
    } else if constexpr (FAM == F444_16) {
        y[0] = sample16(w, l.y0, d);
        u[0] = sample16(w, l.u, d); v[0] = sample16(w, l.v, d);
    } else if constexpr (FAM == F410) {
        u[0] = (int)(w[0] & 1023u); y[0] = (int)(w[0] >> 10 & 1023u); v[0] = (int)(w[0] >> 20 & 1023u);
    } else {
        u[0] = (int)(w[0] & 1023u); y[0] = (int)(w[0] >> 10 & 1023u); v[0] = (int)(w[0] >> 20 & 1023u);
        y[1] = (int)(w[1] & 1023u); u[1] = (int)(w[1] >> 10 & 1023u); y[2] = (int)(w[1] >> 20 & 1023u);
        v[1] = (int)(w[2] & 1023u); y[3] = (int)(w[2] >> 10 & 1023u); u[2] = (int)(w[2] >> 20 & 1023u);
        y[4] = (int)(w[3] & 1023u); v[2] = (int)(w[3] >> 10 & 1023u); y[5] = (int)(w[3] >> 20 & 1023u);
    }
}

// interpolated chroma, the 4:2:2 families: chroma pair k of a row, as single-sample loads (v210: the words that hold it;
// R = k % 3, its place in the group)
template <int FAM, int R>
__device__ __forceinline__ void pair_at(const unsigned char* srow, int k, const packed_lay& l, const depth& d, int& u, int& v) {
    if constexpr (FAM == F422_8) {
        const unsigned char* g = srow + 4ll * k;
        u = (int)g[l.u]; v = (int)g[l.v];
    } else if constexpr (FAM == F422_16) {
        const unsigned char* g = srow + 8ll * k;
        u = sample_at<2>(g + 2 * l.u, d); v = sample_at<2>(g + 2 * l.v, d);
    } else {
        const unsigned* g = reinterpret_cast<const unsigned*>(srow) + 4ll * (k / 3);
        if constexpr (R == 0) { const unsigned w = g[0]; u = (int)(w & 1023u); v = (int)(w >> 20 & 1023u); }
        else { u = (int)(g[2] >> 20 & 1023u); v = (int)(g[3] >> 10 & 1023u); }
    }
}

// the words of a unit, NG whole groups at src: WIDE in 16-byte loads from a 16-byte-aligned address, else sample by sample
template <int FAM, int NG, bool WIDE>
__device__ __forceinline__ void load_unit(const unsigned char* src, unsigned (&all)[NG * fam_gw(FAM)]) {
    if constexpr (WIDE) {
        load_words<NG * fam_gw(FAM) * 4>(src, all);
    } else {
        static_assert(NG == 1, "sample-sized loads take one group");
        load_group<FAM>(src, all);
    }
}

// one unit of one row: NG whole groups from src -> the pixels x0 .. x0 + NG * P - 1 of the row at orow.  Units of a multiple of
// eight pixels are stored as 8-byte words (their first byte on an 8-byte boundary), the others byte by byte and only below W.
// The store is written out here and in packed_linear_unit: as a function of its own it changed the instructions of six of
// the replicate kernels, Y210's vector form among them (profiles/yuv_kernel_family.json).
template <int FAM, int NG, bool WIDE, class PX>
__device__ __forceinline__ void packed_unit(const unsigned char* src, unsigned char* orow, int x0, int W, const packed_lay& l,
                                            const tdc_yuv_coef& c, const depth& d, const PX& px) {
    constexpr int P = fam_px(FAM), GW = fam_gw(FAM), NC = fam_nc(FAM);
    constexpr int NPIX = NG * P;
    constexpr bool PACK = NPIX % 8 == 0;
    constexpr int CH = PACK ? 8 : NPIX;
    unsigned all[NG * GW];
    load_unit<FAM, NG, WIDE>(src, all);
    unsigned r[NPIX / CH][CH], g[NPIX / CH][CH], b[NPIX / CH][CH];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
        unsigned w[GW];
#pragma unroll
        for (int k = 0; k < GW; ++k) w[k] = all[gi * GW + k];
        int y[P], u[NC], v[NC];
        group_samples<FAM>(w, l, d, y, u, v);
        chroma_terms ct[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) ct[k] = chroma(c, d, u[k], v[k]);
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int yy = c.cy * (y[j] - c.y_off);
            const chroma_terms& k = ct[NC == 1 ? 0 : j >> 1];
            const int q = gi * P + j;
            px(d, yy + k.r, yy + k.g, yy + k.b, r[q / CH][q % CH], g[q / CH][q % CH], b[q / CH][q % CH]);
        }
    }
    if constexpr (PACK) {
        uint2* dst = reinterpret_cast<uint2*>(orow + (long long)x0 * 3);
#pragma unroll
        for (int k = 0; k < NPIX / 8; ++k) {
            uint2 o[3];
            pack_row8(r[k], g[k], b[k], o);
            dst[3 * k] = o[0]; dst[3 * k + 1] = o[1]; dst[3 * k + 2] = o[2];
        }
    } else {
#pragma unroll
        for (int j = 0; j < NPIX; ++j) {
            if (x0 + j < W) {       // the unused tail of a row's last group
                unsigned char* o = orow + (long long)(x0 + j) * 3;
                o[0] = (unsigned char)r[0][j]; o[1] = (unsigned char)g[0][j]; o[2] = (unsigned char)b[0][j];
            }
        }
    }
}


// What the walk calls for a unit: per_thread() once before the loops, unit() per unit.
// replicated chroma: a pixel takes the pair of its own group (v210: of its two pixels); nothing outside the unit is read
struct replicated {
    __device__ __forceinline__ int per_thread() const { return 0; }
    template <int FAM, int NG, bool WIDE, class PX>
    __device__ __forceinline__ void unit(int, const unsigned char* srow, const unsigned char* src, unsigned char* orow, int x0, int W,
                                         const packed_lay& l, const tdc_yuv_coef& c, const depth& d, const PX& px) const {
        packed_unit<FAM, NG, WIDE>(src, orow, x0, W, l, c, d, px);
    }
};
// packed_unit with interpolated chroma (the 4:2:2 families): the unit's NG groups hold the pairs k0 .. k0 + NG * NC - 1 of the
// row at srow, and the pair left (centred siting) and right of them are single-sample loads.  A pair at or past Wc (the unused
// tail of the row's last group) is never used: the clamp is by index on the picture's Wc.
template <int FAM, int NG, bool WIDE, class PX>
__device__ __forceinline__ void packed_linear_unit(const unsigned char* srow, const unsigned char* src, unsigned char* orow, int x0,
                                                   int W, const packed_lay& l, const tdc_yuv_coef& c, const depth& d, const PX& px,
                                                   const axis_taps& wx) {
    constexpr int P = fam_px(FAM), GW = fam_gw(FAM), NC = fam_nc(FAM);
    constexpr int NPIX = NG * P, NCU = NG * NC;
    static_assert(NPIX == 2 * NCU, "4:2:2: a chroma pair per two pixels");
    constexpr bool PACK = NPIX % 8 == 0;
    constexpr int CH = PACK ? 8 : NPIX;
    unsigned all[NG * GW];
    if constexpr (WIDE) {
        load_words<NG * GW * 4>(src, all);
    } else {
        static_assert(NG == 1, "sample-sized loads take one group");
        load_group<FAM>(src, all);
    }
    int ys[NPIX], su[NCU + 2], sv[NCU + 2];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
        unsigned w[GW];
#pragma unroll
        for (int k = 0; k < GW; ++k) w[k] = all[gi * GW + k];
        int y[P], u[NC], v[NC];
        group_samples<FAM>(w, l, d, y, u, v);
#pragma unroll
        for (int j = 0; j < P; ++j) ys[gi * P + j] = y[j];
#pragma unroll
        for (int k = 0; k < NC; ++k) { su[1 + gi * NC + k] = u[k]; sv[1 + gi * NC + k] = v[k]; }
    }
    const int k0 = x0 >> 1, Wc = (W + 1) >> 1;      // k0 < Wc: a unit starts below W
    su[0] = su[1]; sv[0] = sv[1];
    if (wx.eb && k0 > 0) pair_at<FAM, 2>(srow, k0 - 1, l, d, su[0], sv[0]);         // only the centred siting looks left
#pragma unroll
    for (int k = 1; k < NCU; ++k)                   // the tail of the row's last group takes the last live pair
        if (k0 + k >= Wc) { su[1 + k] = su[k]; sv[1 + k] = sv[k]; }
    su[NCU + 1] = su[NCU]; sv[NCU + 1] = sv[NCU];
    if (k0 + NCU < Wc) pair_at<FAM, 0>(srow, k0 + NCU, l, d, su[NCU + 1], sv[NCU + 1]);
    int hu[NPIX], hv[NPIX];
    horizontal_sums<NCU>(su, wx, hu);
    horizontal_sums<NCU>(sv, wx, hv);
    unsigned r[NPIX / CH][CH], g[NPIX / CH][CH], b[NPIX / CH][CH];
#pragma unroll
    for (int q = 0; q < NPIX; ++q) {
        const int yy = c.cy * (ys[q] - c.y_off);
        const chroma_terms k = chroma(c, d, interpolated(4, hu[q], 0, 0), interpolated(4, hv[q], 0, 0));
        px(d, yy + k.r, yy + k.g, yy + k.b, r[q / CH][q % CH], g[q / CH][q % CH], b[q / CH][q % CH]);
    }
    if constexpr (PACK) {
        uint2* dst = reinterpret_cast<uint2*>(orow + (long long)x0 * 3);
#pragma unroll
        for (int k = 0; k < NPIX / 8; ++k) {
            uint2 o[3];
            pack_row8(r[k], g[k], b[k], o);
            dst[3 * k] = o[0]; dst[3 * k + 1] = o[1]; dst[3 * k + 2] = o[2];
        }
    } else {
#pragma unroll
        for (int j = 0; j < NPIX; ++j) {
            if (x0 + j < W) {       // the unused tail of a row's last group
                unsigned char* o = orow + (long long)(x0 + j) * 3;
                o[0] = (unsigned char)r[0][j]; o[1] = (unsigned char)g[0][j]; o[2] = (unsigned char)b[0][j];
            }
        }
    }
}


// interpolated chroma: the taps of the horizontal axis once per thread
struct interpolated_x {
    tdc_chroma_site s;
    __device__ __forceinline__ axis_taps per_thread() const { return axis_taps_of(s.sit_x, 1); }
    template <int FAM, int NG, bool WIDE, class PX>
    __device__ __forceinline__ void unit(const axis_taps& wx, const unsigned char* srow, const unsigned char* src, unsigned char* orow,
                                         int x0, int W, const packed_lay& l, const tdc_yuv_coef& c, const depth& d, const PX& px) const {
        packed_linear_unit<FAM, NG, WIDE>(srow, src, orow, x0, W, l, c, d, px, wx);
    }
};

// grid: x strides over the frame's units (units_x per row, H rows), y strides over the frames, as in yuv_frames.  Every
// index is derived from T, H, W and the strides the host has checked against them.  VEC: the first units_vec units of a row
// are eight pixels (v210: 24); v210 rows whose width is no multiple of 24 end in units of one group.
template <int FAM, int FORM, class CH, class PX>
__device__ __forceinline__ void packed_frames(const tdc_yuv_packed& p, const packed_lay& l, const tdc_yuv_coef& c, const depth& d,
                                              const PX& px, const CH& ch, int T, int H, int W, int units_x, int units_vec,
                                              unsigned char* rgb) {
    constexpr int P = fam_px(FAM), GB = fam_gw(FAM) * 4;
    constexpr int NG = FAM == FV210 ? 4 : 8 / P;                // groups per vector unit
    const auto pt = ch.per_thread();
    const long long units = (long long)units_x * H;             // < 2^32: units_x and H are at most 65535
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const unsigned char* sf = p.base + (long long)t * p.frame;
        unsigned char* of = rgb + (long long)t * H * W * 3;
        for (long long i = first_unit(); i < units; i += unit_stride()) {
            // v210 VEC: the frame's vector units come first and its group units after them, so that the two kinds share one wave only once
            const bool tail = FAM == FV210 && FORM == VEC && i >= (long long)units_vec * H;
            const unsigned per_row = FAM == FV210 && FORM == VEC ? (unsigned)(tail ? units_x - units_vec : units_vec) : (unsigned)units_x;
            const unsigned j = (unsigned)(tail ? i - (long long)units_vec * H : i);     // i < 2^32: 32-bit divisions
            const unsigned row_ = j / per_row;
            const int row = (int)row_, xu = (int)(j - row_ * per_row);
            const unsigned char* srow = sf + (long long)row * p.pitch;
            unsigned char* orow = of + (long long)row * W * 3;
            if constexpr (FORM == GROUP) {
                ch.template unit<FAM, 1, false>(pt, srow, srow + (long long)xu * GB, orow, xu * P, W, l, c, d, px);
            } else if constexpr (FAM == FV210) {
                if (!tail) {
                    ch.template unit<FAM, NG, true>(pt, srow, srow + (long long)xu * (NG * GB), orow, xu * (NG * P), W, l, c, d, px);
                } else {
                    const int gi = units_vec * NG + xu;
                    ch.template unit<FAM, 1, true>(pt, srow, srow + (long long)gi * GB, orow, gi * P, W, l, c, d, px);
                }
            } else {
                ch.template unit<FAM, NG, true>(pt, srow, srow + (long long)xu * (NG * GB), orow, xu * (NG * P), W, l, c, d, px);
            }
        }
    }
}

// S: nothing for the replicate kernels, the chroma site for the interpolating ones, where the kernels have always taken it
template <int FAM, int FORM, class CH, class... S>
__global__ __launch_bounds__(256) void yuv_packed_to_rgb_kernel(tdc_yuv_packed p, packed_lay l, tdc_yuv_coef c, S... s, int T, int H,
                                                                int W, int units_x, int units_vec, unsigned char* rgb) {
    packed_frames<FAM, FORM>(p, l, c, depth_of(p.bits, p.msb_aligned, 8), sdr_pixel(), CH{s...}, T, H, W, units_x, units_vec, rgb);
}

template <int FAM, int FORM, class CH, class... S>
__global__ __launch_bounds__(256) void yuv_packed_hdr_to_rgb_kernel(tdc_yuv_packed p, packed_lay l, tdc_yuv_coef c, tdc_hdr_desc h, S... s,
                                                                    int T, int H, int W, int units_x, int units_vec, unsigned char* rgb) {
    extern __shared__ float lut[];      // 2^bits entries
    stage_hdr_lut(lut, h, p.bits);
    packed_frames<FAM, FORM>(p, l, c, depth_of(p.bits, p.msb_aligned, p.bits), hdr_pixel{h, lut}, CH{s...}, T, H, W, units_x, units_vec,
                             rgb);
}

struct packed_launch { int form, units_x, units_vec; dim3 grid; };

template <int FAM, int FORM, class CH, class... S>
void launch_form(const packed_launch& q, hipStream_t st, const tdc_yuv_packed& p, const packed_lay& l, const tdc_yuv_coef& c,
                 const tdc_hdr_desc* h, int T, int H, int W, unsigned char* rgb, const S&... s) {
    const dim3 block(256);
    if constexpr (fam_ss(FAM) != 1) {       // the families that hold more than 8 bits
        if (h) {
            hipLaunchKernelGGL((yuv_packed_hdr_to_rgb_kernel<FAM, FORM, CH, S...>), q.grid, block, sizeof(float) << p.bits, st, p, l, c, *h,
                               s..., T, H, W, q.units_x, q.units_vec, rgb);
            return;
        }
    }
    hipLaunchKernelGGL((yuv_packed_to_rgb_kernel<FAM, FORM, CH, S...>), q.grid, block, 0, st, p, l, c, s..., T, H, W, q.units_x, q.units_vec,
                       rgb);
}

template <int FAM, class CH, class... S>
void launch(const packed_launch& q, hipStream_t st, const tdc_yuv_packed& p, const packed_lay& l, const tdc_yuv_coef& c,
            const tdc_hdr_desc* h, int T, int H, int W, unsigned char* rgb, const S&... s) {
    if (q.form == VEC) return launch_form<FAM, VEC, CH>(q, st, p, l, c, h, T, H, W, rgb, s...);
    launch_form<FAM, GROUP, CH>(q, st, p, l, c, h, T, H, W, rgb, s...);
}

inline int group_bytes(int family) { return 4 * fam_gw(family); }

// everything tdc_yuv_packed_to_rgb refuses, before any launch
inline bool packed_args_ok(const tdc_yuv_packed* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h, int T, int H, int W,
                           const unsigned char* rgb, packed_fmt& f) {
    if (!p || !c || !rgb || !p->base) return false;
    if (T < 1 || H < 1 || W < 1 || T > 65535 || H > 65535 || W > 65535) return false;
    if (!packed_fmt_of(p->format, f)) return false;
    const int ws = fam_ss(f.family);
    if (ws == 1 ? p->bits != 8 : (ws == 2 ? p->bits != 10 && p->bits != 12 : p->bits != 10)) return false;
    if ((p->msb_aligned != 0 && p->msb_aligned != 1) || (p->msb_aligned && ws != 2)) return false;
    if (!aligned(p->base, ws) || p->pitch % ws || p->frame % ws) return false;
    const long long row = (long long)((W + fam_px(f.family) - 1) / fam_px(f.family)) * group_bytes(f.family);    // the row's read set
    if (p->pitch < row) return false;
    if (T > 1 && p->frame < (long long)(H - 1) * p->pitch + row) return false;
    if (!yuv_coef_ok(c, p->bits)) return false;
    if (h && (p->bits == 8 || !hdr_desc_ok(h))) return false;
    return true;
}

// the vector form: every 16-byte load and every 8-byte RGB store lands on its own alignment in every row of every frame.
// v210: W % 8 == 0 puts every row and every 24-pixel unit of the output on an 8-byte boundary; what is left of a row after
// its W / 24 vector units goes group by group.
inline packed_launch packed_launch_of(const tdc_yuv_packed* p, int family, int T, int H, int W, const unsigned char* rgb) {
    const int P = fam_px(family);
    const bool vec = W % 8 == 0 && (family != FV210 || W >= 24) && aligned(p->base, 16) && multiple(p->pitch, 16) &&
                     (T == 1 || multiple(p->frame, 16)) && aligned(rgb, 8);
    int units_vec = 0, units_x = (W + P - 1) / P;
    if (vec) {
        units_vec = family == FV210 ? W / 24 : W / 8;
        units_x = units_vec + (family == FV210 ? (W - 24 * units_vec + 5) / 6 : 0);
    }
    return {vec ? VEC : GROUP, units_x, units_vec, stream_grid((long long)units_x * H, T)};
}

}  // namespace

extern "C" int tdc_yuv_packed_to_rgb(const tdc_yuv_packed* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h, int T, int H, int W,
                                     unsigned char* rgb, void* stream) {
    packed_fmt f;
    if (!packed_args_ok(p, c, h, T, H, W, rgb, f)) return TDC_E_BADARG;
    const packed_launch q = packed_launch_of(p, f.family, T, H, W, rgb);
    hipStream_t st = (hipStream_t)stream;
    switch (f.family) {
        case F422_8: launch<F422_8, replicated>(q, st, *p, f.lay, *c, h, T, H, W, rgb); break;
        case F422_16: launch<F422_16, replicated>(q, st, *p, f.lay, *c, h, T, H, W, rgb); break;
        case F444_8: launch<F444_8, replicated>(q, st, *p, f.lay, *c, h, T, H, W, rgb); break;
        case F444_16: launch<F444_16, replicated>(q, st, *p, f.lay, *c, h, T, H, W, rgb); break;
        case F410: launch<F410, replicated>(q, st, *p, f.lay, *c, h, T, H, W, rgb); break;
        default: launch<FV210, replicated>(q, st, *p, f.lay, *c, h, T, H, W, rgb); break;
    }
    return (int)hipGetLastError();
}

extern "C" int tdc_yuv_packed_linear_to_rgb(const tdc_yuv_packed* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h, const tdc_chroma_site* s,
                                            int T, int H, int W, unsigned char* rgb, void* stream) {
    packed_fmt f;
    if (!chroma_site_ok(s) || !packed_args_ok(p, c, h, T, H, W, rgb, f)) return TDC_E_BADARG;
    if (f.family != F422_8 && f.family != F422_16 && f.family != FV210) return TDC_E_BADARG;      // 4:4:4: nothing to interpolate
    const packed_launch q = packed_launch_of(p, f.family, T, H, W, rgb);
    hipStream_t st = (hipStream_t)stream;
    switch (f.family) {
        case F422_8: launch<F422_8, interpolated_x>(q, st, *p, f.lay, *c, h, T, H, W, rgb, *s); break;
        case F422_16: launch<F422_16, interpolated_x>(q, st, *p, f.lay, *c, h, T, H, W, rgb, *s); break;
        default: launch<FV210, interpolated_x>(q, st, *p, f.lay, *c, h, T, H, W, rgb, *s); break;
    }
    return (int)hipGetLastError();
}
