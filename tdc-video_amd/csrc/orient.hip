// Display orientation of decoded RGB frames: what stands between the picture a decoder stores and the
// upright picture tdc_preprocess_frames takes.  A permutation of bytes, exact by construction: one of the eight elements of
// the dihedral group, written as (quarters clockwise, then a left-right mirror) in include/tdc_hip.h and reduced here to
//   transposing (quarters 1, 3):  O[y, x] = S[fr ? H-1-x : x, fc ? W-1-y : y]      O is [W, H]
//   row-keeping (quarters 0, 2):  O[y, x] = S[fr ? H-1-y : y, fc ? W-1-x : x]      O is [H, W]
// with (fr, fc) from the table in flips().  HBM-bound byte work: 3 bytes read and 3 written per pixel.
//   row-keeping  no LDS.  WORD form: a thread moves four pixels as three 4-byte words and reverses their order in registers
//                when fc; BYTE form: a thread moves one pixel as three bytes.
//   transposing  a workgroup moves a tile of 64 x 64 source pixels through LDS: source rows in (coalesced along the source
//                row), destination rows out (coalesced along the destination row).  The LDS pitch is 196 bytes = 49 dwords,
//                odd, so the byte reads of one output word walk down a tile column on distinct banks (32 consecutive rows
//                land on 32 different banks).  The global loads and the global stores each have a WORD form (4-byte
//                accesses) and a BYTE form, chosen independently.
// The host picks a WORD form from alignment facts alone - the pointer and the row length in bytes are multiples of 4, so every
// row of every frame and every tile's first byte are - and the forms move the same bytes to the same places.
// Every byte offset is 64-bit: a slab of 64 8K frames is 6.4 GB.
#include "common.h"
#include "../../include/tdc_hip.h"

namespace {

enum { TS = 64, PITCH = TS * 3 + 4, ROW_WORDS = TS * 3 / 4, ROW_BYTES = TS * 3, THREADS = 256 };

struct w3 { unsigned a, b, c; };    // four pixels; 4-byte aligned

__device__ __forceinline__ unsigned byte_of(const w3& w, int i) {      // byte i of the twelve, i a compile-time constant
    const unsigned v = i < 4 ? w.a : (i < 8 ? w.b : w.c);
    return (v >> (8 * (i & 3))) & 255u;
}

// four pixels p0 p1 p2 p3 -> p3 p2 p1 p0, the bytes of a pixel kept in order
__device__ __forceinline__ w3 reverse4(const w3& w) {
    unsigned o[12];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * p + c] = byte_of(w, 3 * (3 - p) + c);
    w3 r;
    r.a = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
    r.b = o[4] | o[5] << 8 | o[6] << 16 | o[7] << 24;
    r.c = o[8] | o[9] << 8 | o[10] << 16 | o[11] << 24;
    return r;
}

// grid: x over the frame's units (WORD: H rows of W / 4 groups of four pixels; BYTE: H rows of W pixels), y over the frames
template <bool WORD>
__global__ __launch_bounds__(THREADS) void orient_rows_kernel(const unsigned char* __restrict__ src, int T, int H, int W,
                                                              int fr, int fc, unsigned char* __restrict__ dst) {
    const int per_row = WORD ? W / 4 : W;
    const long long units = (long long)H * per_row;
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= units) return;
    const int oy = (int)(i / per_row), g = (int)(i - (long long)oy * per_row);
    const int sy = fr ? H - 1 - oy : oy, sg = fc ? per_row - 1 - g : g;
    const long long row = (long long)W * 3, frame = (long long)H * row;
    const int step = WORD ? 12 : 3;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const unsigned char* s = src + t * frame + sy * row + (long long)sg * step;
        unsigned char* d = dst + t * frame + oy * row + (long long)g * step;
        if (WORD) {
            const w3 w = *reinterpret_cast<const w3*>(s);
            *reinterpret_cast<w3*>(d) = fc ? reverse4(w) : w;
        } else {
            const unsigned char r = s[0], gg = s[1], b = s[2];
            d[0] = r; d[1] = gg; d[2] = b;
        }
    }
}

// grid: x, y over the 64 x 64 tiles of the SOURCE frame, z over the frames.  th x tw is the tile's extent (edge tiles are
// smaller); only lds[r][0 .. 3 tw) of rows r < th is written and only that is read.
template <bool LOADW, bool STOREW>
__global__ __launch_bounds__(THREADS) void orient_transpose_kernel(const unsigned char* __restrict__ src, int T, int H, int W,
                                                                   int fr, int fc, unsigned char* __restrict__ dst) {
    __shared__ __align__(16) unsigned char lds[TS * PITCH];
    const int tid = threadIdx.x;
    const int ys0 = blockIdx.y * TS, xs0 = blockIdx.x * TS;
    const int th = H - ys0 < TS ? H - ys0 : TS, tw = W - xs0 < TS ? W - xs0 : TS;
    const long long frame = (long long)H * W * 3;
    // where the tile lands: destination rows are source columns, destination pixels of a row are source rows
    const int ox0 = fr ? H - ys0 - th : ys0;
    for (int t = blockIdx.z; t < T; t += gridDim.z) {
        const unsigned char* s = src + t * frame + ((long long)ys0 * W + xs0) * 3;
        if (LOADW) {                        // W % 4 == 0: tw % 4 == 0, 3 tw / 4 whole words per row
            const int nw = tw * 3 / 4;
            for (int i = tid; i < TS * ROW_WORDS; i += THREADS) {
                const int r = i / ROW_WORDS, w = i - r * ROW_WORDS;
                if (r < th && w < nw)
                    *reinterpret_cast<unsigned*>(lds + r * PITCH + 4 * w) =
                        *reinterpret_cast<const unsigned*>(s + (long long)r * W * 3 + 4 * w);
            }
        } else {
            const int nb = tw * 3;
            for (int i = tid; i < TS * ROW_BYTES; i += THREADS) {
                const int r = i / ROW_BYTES, b = i - r * ROW_BYTES;
                if (r < th && b < nb) lds[r * PITCH + b] = s[(long long)r * W * 3 + b];
            }
        }
        __syncthreads();
        unsigned char* d = dst + t * frame;
        if (STOREW) {                       // H % 4 == 0: th % 4 == 0, 3 th / 4 whole words per destination row
            const int nw = th * 3 / 4;
            for (int i = tid; i < TS * ROW_WORDS; i += THREADS) {
                const int c = i / ROW_WORDS, w = i - c * ROW_WORDS;
                if (c < tw && w < nw) {
                    const int oy = fc ? W - 1 - (xs0 + c) : xs0 + c;
                    unsigned v = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int b = 4 * w + k, j = b / 3, ch = b - 3 * j;
                        const int r = fr ? th - 1 - j : j;
                        v |= (unsigned)lds[r * PITCH + c * 3 + ch] << (8 * k);
                    }
                    *reinterpret_cast<unsigned*>(d + ((long long)oy * H + ox0) * 3 + 4 * w) = v;
                }
            }
        } else {
            const int nb = th * 3;
            for (int i = tid; i < TS * ROW_BYTES; i += THREADS) {
                const int c = i / ROW_BYTES, b = i - c * ROW_BYTES;
                if (c < tw && b < nb) {
                    const int oy = fc ? W - 1 - (xs0 + c) : xs0 + c;
                    const int j = b / 3, ch = b - 3 * j;
                    const int r = fr ? th - 1 - j : j;
                    d[((long long)oy * H + ox0) * 3 + b] = lds[r * PITCH + c * 3 + ch];
                }
            }
        }
        __syncthreads();                    // the next frame's loads overwrite the tile
    }
}

inline bool aligned4(const void* p) { return ((unsigned long long)p & 3ull) == 0; }

// (fr, fc) of (quarters, hflip): which source axis runs backwards
inline void flips(int quarters, int hflip, int* fr, int* fc) {
    switch (quarters) {
        case 0: *fr = 0; *fc = hflip; break;             // S[y, x]           | S[y, W-1-x]
        case 1: *fr = !hflip; *fc = 0; break;            // S[H-1-x, y]       | S[x, y]
        case 2: *fr = 1; *fc = !hflip; break;            // S[H-1-y, W-1-x]   | S[H-1-y, x]
        default: *fr = hflip; *fc = 1; break;            // S[x, W-1-y]       | S[H-1-x, W-1-y]
    }
}

}  // namespace

extern "C" int tdc_orient_frames(const unsigned char* src, int T, int H, int W, int quarters, int hflip, unsigned char* dst,
                                 void* stream) {
    if (!src || !dst) return TDC_E_BADARG;
    if (T < 1 || H < 1 || W < 1 || T > 65535 || H > 65535 || W > 65535) return TDC_E_BADARG;
    if (quarters < 0 || quarters > 3 || (hflip != 0 && hflip != 1)) return TDC_E_BADARG;
    const unsigned long long n = 3ull * (unsigned long long)T * (unsigned long long)H * (unsigned long long)W;   // < 2^50
    const unsigned long long a = (unsigned long long)src, b = (unsigned long long)dst;
    if (a < b + n && b < a + n) return TDC_E_BADARG;      // the ranges overlap
    int fr, fc;
    flips(quarters, hflip, &fr, &fc);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(THREADS);
    if (quarters & 1) {
        // a row of the source is 3 W bytes, a row of the destination 3 H bytes; a tile starts 192 k bytes into its row
        const bool loadw = aligned4(src) && W % 4 == 0, storew = aligned4(dst) && H % 4 == 0;
        const dim3 grid((W + TS - 1) / TS, (H + TS - 1) / TS, T);       // <= 1024 x 1024 x 65535
        if (loadw && storew) hipLaunchKernelGGL((orient_transpose_kernel<true, true>), grid, block, 0, st, src, T, H, W, fr, fc, dst);
        else if (loadw) hipLaunchKernelGGL((orient_transpose_kernel<true, false>), grid, block, 0, st, src, T, H, W, fr, fc, dst);
        else if (storew) hipLaunchKernelGGL((orient_transpose_kernel<false, true>), grid, block, 0, st, src, T, H, W, fr, fc, dst);
        else hipLaunchKernelGGL((orient_transpose_kernel<false, false>), grid, block, 0, st, src, T, H, W, fr, fc, dst);
    } else {
        const bool word = aligned4(src) && aligned4(dst) && W % 4 == 0;
        const long long units = (long long)H * (word ? W / 4 : W);       // < 2^32
        const dim3 grid((unsigned)((units + THREADS - 1) / THREADS), T); // <= 2^24 x 65535
        if (word) hipLaunchKernelGGL(orient_rows_kernel<true>, grid, block, 0, st, src, T, H, W, fr, fc, dst);
        else hipLaunchKernelGGL(orient_rows_kernel<false>, grid, block, 0, st, src, T, H, W, fr, fc, dst);
    }
    return (int)hipGetLastError();
}
