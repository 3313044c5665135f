// Content fingerprints of byte rows (the frame cache's keys, tdc-video_amd/cache.py): one 128-bit value per listed row of a
// strided buffer, read where the rows lie (no gather copy of the selected frames first).
//   w_i  = little-endian u64 word i of the row (the tail zero-padded)
//   x_i  = w_i ^ (i * GOLDEN)
//   h_k  = mix(sum_i mix(x_i ^ S_k) ^ row_bytes), k = 1, 2; sums mod 2^64, mix = the splitmix64 finaliser
// The sums wrap, so they are associative and commutative: any split of a row into workgroups and any reduction order gives
// the same bits, and cache.fingerprint_rows_host reproduces them in numpy.
#include "common.h"
#include "../../include/tdc_hip.h"

namespace {

typedef unsigned long long u64;
constexpr u64 FP_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr u64 FP_S1 = 0x243F6A8885A308D3ull;
constexpr u64 FP_S2 = 0x13198A2E03707344ull;
constexpr int FP_MAX_CHUNKS = 64;             // workgroups per row at most (scratch: rows x 64 x 2 words)
constexpr long long FP_WORDS_PER_WG = 8192;   // 64 KB of a row per workgroup before the row is split further

__device__ __forceinline__ u64 fp_mix(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// word i of a row at p of `len` bytes whose address allows no wider load: bytes, zero past the end
__device__ __forceinline__ u64 fp_word_bytes(const unsigned char* p, long long i, long long len) {
    u64 w = 0;
    for (int b = 0; b < 8; ++b) {
        const long long o = i * 8 + b;
        if (o < len) w |= (u64)p[o] << (8 * b);
    }
    return w;
}

__device__ __forceinline__ void fp_add(u64 w, long long i, u64& h1, u64& h2) {
    const u64 x = w ^ ((u64)i * FP_GOLDEN);
    h1 += fp_mix(x ^ FP_S1);
    h2 += fp_mix(x ^ FP_S2);
}

inline int fp_chunks(long long words) {
    long long c = (words + FP_WORDS_PER_WG - 1) / FP_WORDS_PER_WG;
    return (int)(c < 1 ? 1 : c > FP_MAX_CHUNKS ? FP_MAX_CHUNKS : c);
}

// grid (chunks, n_rows): workgroup (ch, r) sums the words of its chunk of row rows[r]; thread k takes word pair k (one 16-byte
// load when the row start is 16-byte aligned and the pair lies inside the row, two 8-byte loads at 8-byte alignment, bytes
// otherwise and for the zero-padded tail)
__global__ __launch_bounds__(256) void fingerprint_partial(const unsigned char* base, long long stride, const int* rows,
                                                           long long len, int chunks, u64* part) {
    const int r = blockIdx.y, ch = blockIdx.x;
    const unsigned char* p = base + (long long)rows[r] * stride;
    const long long words = (len + 7) / 8, pairs = (words + 1) / 2;
    const long long per = (pairs + chunks - 1) / chunks;
    const long long lo = ch * per, hi = lo + per < pairs ? lo + per : pairs;
    const bool al16 = ((uintptr_t)p & 15) == 0, al8 = ((uintptr_t)p & 7) == 0;
    const long long full = len / 8;                           // words wholly inside the row
    u64 h1 = 0, h2 = 0;
    for (long long k = lo + threadIdx.x; k < hi; k += 256) {
        const long long i = 2 * k;
        u64 w0, w1 = 0;
        if (i + 2 <= full && al16) {
            const u32x4 v = *(const u32x4*)(p + i * 8);
            w0 = (u64)v[0] | ((u64)v[1] << 32);
            w1 = (u64)v[2] | ((u64)v[3] << 32);
        } else if (i + 2 <= full && al8) {
            w0 = *(const u64*)(p + i * 8);
            w1 = *(const u64*)(p + i * 8 + 8);
        } else {
            w0 = fp_word_bytes(p, i, len);
            if (i + 1 < words) w1 = fp_word_bytes(p, i + 1, len);
        }
        fp_add(w0, i, h1, h2);
        if (i + 1 < words) fp_add(w1, i + 1, h1, h2);
    }
    __shared__ u64 red[2][256];
    red[0][threadIdx.x] = h1;
    red[1][threadIdx.x] = h2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[((long long)r * FP_MAX_CHUNKS + ch) * 2] = red[0][0];
        part[((long long)r * FP_MAX_CHUNKS + ch) * 2 + 1] = red[1][0];
    }
}

__global__ void fingerprint_final(const u64* part, int n_rows, int chunks, long long len, u64* out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    u64 h1 = 0, h2 = 0;
    for (int c = 0; c < chunks; ++c) {
        h1 += part[((long long)r * FP_MAX_CHUNKS + c) * 2];
        h2 += part[((long long)r * FP_MAX_CHUNKS + c) * 2 + 1];
    }
    out[2 * r] = fp_mix(h1 ^ (u64)len);
    out[2 * r + 1] = fp_mix(h2 ^ (u64)len);
}

}  // namespace

extern "C" int tdc_fingerprint_rows(const void* base, long long row_stride, const int* rows, int n_rows, long long row_bytes,
                                    unsigned long long* out, void* scratch, void* stream) {
    if (!base || !rows || !out || !scratch || n_rows <= 0 || n_rows > 65535 || row_bytes <= 0 || row_stride < 0) return TDC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int chunks = fp_chunks((row_bytes + 7) / 8);
    hipLaunchKernelGGL(fingerprint_partial, dim3(chunks, n_rows), dim3(256), 0, st, (const unsigned char*)base, row_stride,
                       rows, row_bytes, chunks, (u64*)scratch);
    hipLaunchKernelGGL(fingerprint_final, dim3((n_rows + 255) / 256), dim3(256), 0, st, (const u64*)scratch, n_rows, chunks,
                       row_bytes, (u64*)out);
    return (int)hipGetLastError();
}
extern "C" size_t tdc_fingerprint_rows_scratch_bytes(int n_rows) { return (size_t)n_rows * FP_MAX_CHUNKS * 2 * sizeof(u64); }
