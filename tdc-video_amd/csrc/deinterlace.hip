// One field of interlaced video rebuilt to a full-height frame: what stands between the half-height
// RGB picture of the kept field and the frame tdc_preprocess_frames takes.  With F[k], k in [0, Hf), the field's rows,
// p the parity (0: the field is the even rows of the frame, 1: the odd rows) and cl(i) = min(max(i, 0), Hf - 1), per byte
//   O[2k + p]     = F[k]                                                                     kept rows: copies
//   O[2k + 1 - p],  m = k - p:
//       linear   (F[cl(m)] + F[cl(m+1)] + 1) >> 1
//       cubic    clip_0_255((9 (F[cl(m)] + F[cl(m+1)]) - F[cl(m-1)] - F[cl(m+2)] + 8) >> 4)
// HBM-bound byte work, no LDS: 3 bytes read and 6 written per field pixel.  A thread owns a column of V bytes (16, 4 or 1)
// of the row and walks a run of RUN field rows = 2 RUN output rows.  It holds the window F[cl(m-1)] .. F[cl(m+2)] (linear:
// F[cl(m)], F[cl(m+1)]) in registers and slides it down, so a run loads RUN + 3 field rows (linear: RUN + 1): every row
// once plus the halo at the run's ends, clamped rows included - never a byte between two field rows.
// The arithmetic runs on the bytes where they lie.  linear: the rounded-up mean of four bytes in one word is
// (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7f), no byte borrows from its neighbour.  cubic: the even and the odd bytes of a word
// as two 16-bit lanes each; 9 (b + c) + 8 + 512 - (a + d) lies in [10, 5110], so no lane carries or borrows and the packed
// word is computed with 32-bit integer instructions; its shift by 4 is floor((..) / 16) + 32 - the bias 512 = 32 * 16 keeps
// the shifted value non-negative, so the rounding of a shift of a negative number never enters: every negative sum ends
// below 32 and clips to 0 - and clamping to [32, 287] before taking the 32 off is the clip to [0, 255].
// The host picks V from the alignment of src, both strides (one that is never applied - T = 1, Hf = 1 - left out), dst and
// 3 W alone; the forms produce the same bytes.
// Every byte offset is 64-bit.
#include "common.h"
#include "../../include/tdc_hip.h"

namespace {

enum { THREADS = 256, RUN = 16 };

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

template <int V> struct Col;                                         // a thread's V bytes of one row, as 32-bit words
template <> struct Col<16> { enum { N = 4 }; unsigned w[4]; };
template <> struct Col<4> { enum { N = 1 }; unsigned w[1]; };
template <> struct Col<1> { enum { N = 1 }; unsigned w[1]; };       // one byte, zero-extended

template <int V>
__device__ __forceinline__ Col<V> load(const unsigned char* p) {
    Col<V> c;
    if constexpr (V == 16) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p);
        c.w[0] = v[0]; c.w[1] = v[1]; c.w[2] = v[2]; c.w[3] = v[3];
    } else if constexpr (V == 4) {
        c.w[0] = *reinterpret_cast<const unsigned*>(p);
    } else {
        c.w[0] = *p;
    }
    return c;
}

template <int V>
__device__ __forceinline__ void store(unsigned char* p, const Col<V>& c) {
    if constexpr (V == 16) {
        *reinterpret_cast<u32x4*>(p) = (u32x4){c.w[0], c.w[1], c.w[2], c.w[3]};
    } else if constexpr (V == 4) {
        *reinterpret_cast<unsigned*>(p) = c.w[0];
    } else {
        *p = (unsigned char)c.w[0];
    }
}

// four bytes: (a + b + 1) >> 1 each
__device__ __forceinline__ unsigned mean4(unsigned a, unsigned b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }

// two 16-bit lanes holding bytes: clip_0_255((9 (b + c) - a - d + 8) >> 4) each
__device__ __forceinline__ unsigned cubic2(unsigned a, unsigned b, unsigned c, unsigned d) {
    // the 32-bit shift moves the high lane's low four bits into bits 12 .. 15 of the low lane: the mask takes them off again
    const unsigned x = (((b + c) * 9u + 0x02080208u - (a + d)) >> 4) & 0x0fff0fffu;      // floor(sum / 16) + 32, in [0, 319]
    u16x2 y = __builtin_bit_cast(u16x2, x);
    y = __builtin_elementwise_min(__builtin_elementwise_max(y, (u16x2){32, 32}), (u16x2){287, 287});
    return __builtin_bit_cast(unsigned, y) - 0x00200020u;
}

__device__ __forceinline__ unsigned cubic4(unsigned a, unsigned b, unsigned c, unsigned d) {
    const unsigned M = 0x00ff00ffu;
    return cubic2(a & M, b & M, c & M, d & M) | cubic2((a >> 8) & M, (b >> 8) & M, (c >> 8) & M, (d >> 8) & M) << 8;
}

// grid: x over the row's columns of V bytes, y over the runs of RUN field rows, z over the frames.  units = 3 W / V.
template <int V, bool CUBIC>
__global__ __launch_bounds__(THREADS) void field_to_frame_kernel(const unsigned char* __restrict__ src, long long frame_stride,
                                                                 long long row_stride, int Hf, int units, int parity,
                                                                 unsigned char* __restrict__ dst) {
    const int u = blockIdx.x * THREADS + threadIdx.x;
    if (u >= units) return;
    const int k0 = blockIdx.y * RUN;                                       // < Hf: the grid holds ceil(Hf / RUN) runs
    const long long col = (long long)u * V, orow = (long long)units * V;   // orow = 3 W, a row of dst
    const unsigned char* s = src + (long long)blockIdx.z * frame_stride + col;
    unsigned char* d = dst + ((long long)blockIdx.z * Hf + k0) * 2 * orow + col;
    const int last = Hf - 1;
    auto row = [&](int i) { return load<V>(s + (long long)(i < 0 ? 0 : (i > last ? last : i)) * row_stride); };
    int m = k0 - parity;                                                   // the filled row lies between F[m] and F[m + 1]
    Col<V> w0, w1 = row(m), w2, w3;
    if constexpr (CUBIC) {
        w0 = row(m - 1);
        w2 = row(m + 1);
    }
    const long long kept_at = parity ? orow : 0, fill_at = parity ? 0 : orow;
    // a rolled loop (the run ends at the field's last row): one load in flight per thread, the other waves hide its latency
    for (int i = 0; i < RUN; ++i) {
        if (k0 + i > last) break;
        Col<V> f;
        if constexpr (CUBIC) {
            w3 = row(m + 2);
#pragma unroll
            for (int j = 0; j < Col<V>::N; ++j) f.w[j] = cubic4(w0.w[j], w1.w[j], w2.w[j], w3.w[j]);
        } else {
            w2 = row(m + 1);
#pragma unroll
            for (int j = 0; j < Col<V>::N; ++j) f.w[j] = mean4(w1.w[j], w2.w[j]);
        }
        store<V>(d + kept_at, parity ? w2 : w1);                           // F[k0 + i]
        store<V>(d + fill_at, f);
        d += 2 * orow;
        ++m;
        if constexpr (CUBIC) { w0 = w1; w1 = w2; w2 = w3; } else { w1 = w2; }
    }
}

template <int V>
void launch(bool cubic, dim3 grid, hipStream_t st, const unsigned char* src, long long fs, long long rs, int Hf, int units,
            int parity, unsigned char* dst) {
    if (cubic) hipLaunchKernelGGL((field_to_frame_kernel<V, true>), grid, dim3(THREADS), 0, st, src, fs, rs, Hf, units, parity, dst);
    else hipLaunchKernelGGL((field_to_frame_kernel<V, false>), grid, dim3(THREADS), 0, st, src, fs, rs, Hf, units, parity, dst);
}

}  // namespace

extern "C" int tdc_field_to_frame(const unsigned char* src, long long frame_stride, long long row_stride, int T, int Hf, int W,
                                  int parity, int fill, unsigned char* dst, void* stream) {
    if (!src || !dst) return TDC_E_BADARG;
    if (T < 1 || T > 65535 || W < 1 || W > 65535 || Hf < 1 || Hf > 32767) return TDC_E_BADARG;
    if ((parity != 0 && parity != 1) || (fill != 0 && fill != 1)) return TDC_E_BADARG;
    const long long lim = 1ll << 40, row = 3ll * W;
    if (frame_stride < 0 || row_stride < 0 || frame_stride > lim || row_stride > lim) return TDC_E_BADARG;
    const long long frame = (long long)(Hf - 1) * row_stride + row;        // < 2^55: the bytes one frame's field spans
    if (row_stride < row || frame_stride < frame) return TDC_E_BADARG;
    const unsigned long long ns = (unsigned long long)(T - 1) * (unsigned long long)frame_stride + (unsigned long long)frame;   // < 2^57
    const unsigned long long nd = 2ull * (unsigned long long)T * (unsigned long long)Hf * (unsigned long long)row;              // < 2^50
    const unsigned long long a = (unsigned long long)src, b = (unsigned long long)dst;
    if (a < b + nd && b < a + ns) return TDC_E_BADARG;                     // the source extent and dst overlap
    // a stride that is never applied (one frame, one row) says nothing about any address and cannot narrow the form
    const unsigned long long al = a | b | (T > 1 ? (unsigned long long)frame_stride : 0ull) |
                                  (Hf > 1 ? (unsigned long long)row_stride : 0ull) | (unsigned long long)row;
    const int V = (al & 15) == 0 ? 16 : ((al & 3) == 0 ? 4 : 1);
    const int units = (int)(row / V);                                      // <= 196605
    const dim3 grid((units + THREADS - 1) / THREADS, (Hf + RUN - 1) / RUN, T);      // <= 768 x 2048 x 65535
    hipStream_t st = (hipStream_t)stream;
    if (V == 16) launch<16>(fill == 1, grid, st, src, frame_stride, row_stride, Hf, units, parity, dst);
    else if (V == 4) launch<4>(fill == 1, grid, st, src, frame_stride, row_stride, Hf, units, parity, dst);
    else launch<1>(fill == 1, grid, st, src, frame_stride, row_stride, Hf, units, parity, dst);
    return (int)hipGetLastError();
}
