// Decoded PCM -> the mono 16 kHz waveform the BEATs front end takes: what stands between a decoder's
// audio (interleaved s16 or planar float32, any channel count, 8 .. 192 kHz) and tdc_fbank.  The conversion is the stated
// polyphase formula of include/tdc_hip.h - a Kaiser-windowed sinc table the host builds - and no library's.
//   y[n] = sum_j table[(n M) mod L][j] * x[floor(n M / L) + j],  j = -K+1 .. K,  x = 0 outside [0, n_in)
// One workgroup per tile of 256 consecutive outputs.  It stages the input span of the tile (at most 255 M / L + 2K samples)
// into LDS once - s16 -> f32, channel selected or averaged on the way in - and each lane then runs the 2K taps of its phase
// row in ascending j as one fp32 FMA chain.  The row comes from LDS when L == 1 (every lane shares it) and from the
// L2-resident table otherwise.  Two staging forms of ONE kernel, chosen on the host from stride and alignment facts alone:
//   SCALAR  one sample per load: any stride, any pointer
//   VEC     16-byte loads (8 s16 / 4 f32) of a dense channel, on groups aligned in the track and wholly inside [0, n_in);
//           the groups that cross an end of the track take the scalar loads
// A staged sample is the same float either way and the chain of output n reads only n, so the bits of an output depend
// neither on the form nor on out_lo, n_out or the tile it lands in.
#include "common.h"
#include "../../include/tdc_hip.h"

namespace {

enum { TILE = 256 };
enum { S16 = 0, F32 = 1 };

struct pcm_src {
    const void* p;
    long long n_in, sample_stride, channel_stride;   // strides in elements
    int c0, nc;                                       // the addressed channels c0 .. c0 + nc - 1
    int mean_of;                                      // 0: one channel as it is; else the channel count the sum is divided by
};

template <int FMT> struct Elem;
template <> struct Elem<S16> { typedef short type; enum { V = 8 }; };
template <> struct Elem<F32> { typedef float type; enum { V = 4 }; };

__device__ __forceinline__ float to_f32(short s) { return (float)s * (1.0f / 32768.0f); }   // exact
__device__ __forceinline__ float to_f32(float f) { return f; }

// the fp32 mean: the channels summed in ascending order, one division
__device__ __forceinline__ float finish(const pcm_src& s, float sum) { return s.mean_of ? sum / (float)s.mean_of : sum; }

// sample idx in [0, n_in) of the addressed channel(s)
template <int FMT>
__device__ __forceinline__ float load1(const pcm_src& s, long long idx) {
    typedef typename Elem<FMT>::type T;
    const T* p = reinterpret_cast<const T*>(s.p) + idx * s.sample_stride + (long long)s.c0 * s.channel_stride;
    float sum = to_f32(p[0]);
    for (int c = 1; c < s.nc; ++c) sum += to_f32(p[(long long)c * s.channel_stride]);
    return finish(s, sum);
}

// samples gs .. gs + V - 1 of a dense channel (sample_stride == 1), gs a multiple of V, all inside [0, n_in)
template <int FMT>
__device__ __forceinline__ void loadv(const pcm_src& s, long long gs, float (&v)[Elem<FMT>::V]) {
    typedef typename Elem<FMT>::type T;
    enum { V = Elem<FMT>::V };
    const T* p = reinterpret_cast<const T*>(s.p) + gs + (long long)s.c0 * s.channel_stride;
    for (int c = 0; c < s.nc; ++c) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(p + (long long)c * s.channel_stride);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float x;
            const unsigned word = FMT == S16 ? w[e >> 1] >> (16 * (e & 1)) : w[e];      // a copy: bit_cast of the element itself reads element 0
            if (FMT == S16) x = to_f32((short)word);
            else x = __builtin_bit_cast(float, word);
            v[e] = c == 0 ? x : v[e] + x;
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = finish(s, v[e]);
}

__device__ __forceinline__ long long floor_div(long long a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// LDS: xs[span] then, when L == 1, the 2K taps of the one row.  span >= (L - 1 + 255 M) / L + 2K (the host's bound).
template <int FMT, bool VEC>
__global__ __launch_bounds__(TILE) void pcm_resample_kernel(pcm_src s, int L, int M, const float* __restrict__ table, int K,
                                                            long long out_lo, long long n_out, void* out, int out_f32, int span) {
    extern __shared__ __align__(16) float lds[];
    float* xs = lds;
    const int tid = threadIdx.x;
    const long long n0 = out_lo + (long long)blockIdx.x * TILE;
    const long long left = out_lo + n_out - n0;                   // >= 1: the grid covers n_out
    const int cnt = left < TILE ? (int)left : TILE;
    const long long nm0 = n0 * M;                                 // < 2^60: the host bounds out_lo + n_out and M
    const long long base0 = nm0 / L;
    const unsigned r0 = (unsigned)(nm0 - base0 * L);
    const long long s0 = base0 - K + 1;                           // first staged sample (may lie before the track)
    const int s_len = (int)((r0 + (unsigned)(cnt - 1) * (unsigned)M) / (unsigned)L) + 2 * K;      // <= span

    enum { V = VEC ? (int)Elem<FMT>::V : 1 };
    const long long g0 = floor_div(s0, V) * V;
    const int groups = (int)((s0 + s_len - g0 + V - 1) / V);
    for (int g = tid; g < groups; g += TILE) {
        const long long gs = g0 + (long long)g * V;
        float v[V];
        bool whole = false;
        if constexpr (VEC) {
            whole = gs >= 0 && gs + V <= s.n_in;
            if (whole) loadv<FMT>(s, gs, v);
        }
        if (!whole) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const long long idx = gs + e;
                v[e] = idx >= 0 && idx < s.n_in ? load1<FMT>(s, idx) : 0.0f;
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const long long pos = gs + e - s0;
            if (pos >= 0 && pos < s_len) xs[pos] = v[e];
        }
    }
    const float* row = table;
    if (L == 1) {
        float* taps = lds + span;
        for (int j = tid; j < 2 * K; j += TILE) taps[j] = table[j];
        row = taps;
    }
    __syncthreads();
    if (tid >= cnt) return;
    const unsigned a = r0 + (unsigned)tid * (unsigned)M;          // <= 639 + 255 * 2^20
    const unsigned q = a / (unsigned)L, p = a - q * (unsigned)L;
    if (L != 1) row = table + (size_t)p * (size_t)(2 * K);
    const f32x2* row2 = reinterpret_cast<const f32x2*>(row);      // rows start at even floats of an 8-byte aligned table
    const float* x = xs + q;                                       // x[j'] = sample base - K + 1 + j', j' = 0 .. 2K - 1
    float acc = 0.0f;
    for (int j = 0; j < K; ++j) {
        const f32x2 w = row2[j];
        acc = __builtin_fmaf(w[0], x[2 * j], acc);
        acc = __builtin_fmaf(w[1], x[2 * j + 1], acc);
    }
    if (out_f32) reinterpret_cast<float*>(out)[n0 - out_lo + tid] = acc;
    else reinterpret_cast<f16*>(out)[n0 - out_lo + tid] = (f16)acc;
}

// L == M == 1: output n is sample n of the addressed channel(s), 0 past the track's end
template <int FMT>
__global__ __launch_bounds__(TILE) void pcm_select_kernel(pcm_src s, long long out_lo, long long n_out, void* out, int out_f32) {
    for (long long i = (long long)blockIdx.x * TILE + threadIdx.x; i < n_out; i += (long long)gridDim.x * TILE) {
        const long long idx = out_lo + i;
        const float v = idx < s.n_in ? load1<FMT>(s, idx) : 0.0f;
        if (out_f32) reinterpret_cast<float*>(out)[i] = v;
        else reinterpret_cast<f16*>(out)[i] = (f16)v;
    }
}

inline bool aligned(const void* p, unsigned a) { return ((unsigned long long)p & (a - 1)) == 0; }

template <int FMT>
int launch(const pcm_src& s, bool vec, int L, int M, const float* table, int K, long long out_lo, long long n_out, void* out,
           int out_f32, int span, size_t lds_bytes, hipStream_t st) {
    if (L == 1 && M == 1) {
        const long long blocks = (n_out + TILE - 1) / TILE;
        hipLaunchKernelGGL(pcm_select_kernel<FMT>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(TILE), 0, st, s, out_lo,
                           n_out, out, out_f32);
        return (int)hipGetLastError();
    }
    const dim3 grid((unsigned)((n_out + TILE - 1) / TILE)), block(TILE);
    if (vec) hipLaunchKernelGGL((pcm_resample_kernel<FMT, true>), grid, block, lds_bytes, st, s, L, M, table, K, out_lo, n_out, out, out_f32, span);
    else hipLaunchKernelGGL((pcm_resample_kernel<FMT, false>), grid, block, lds_bytes, st, s, L, M, table, K, out_lo, n_out, out, out_f32, span);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int tdc_pcm_resample(const void* pcm, int fmt, long long n_in, int channels, long long sample_stride,
                                long long channel_stride, int channel, int L, int M, const float* table, int K,
                                long long out_lo, long long n_out, void* out, int out_f32, void* stream) {
    if (!pcm || !table || !out) return TDC_E_BADARG;
    if (fmt != S16 && fmt != F32) return TDC_E_BADARG;
    const int esize = fmt == S16 ? 2 : 4;
    if (!aligned(pcm, esize) || !aligned(table, 8) || !aligned(out, out_f32 ? 4 : 2)) return TDC_E_BADARG;
    if (n_in < 1 || n_in > (1ll << 40) || channels < 1 || channels > 65535) return TDC_E_BADARG;
    if (channel < -1 || channel >= channels) return TDC_E_BADARG;
    if (sample_stride < 1 || channel_stride < 0 || sample_stride > (1ll << 20) || channel_stride > (1ll << 42)) return TDC_E_BADARG;
    if (K < 1 || L < 1 || L > 640 || M < 1 || M > (1 << 20)) return TDC_E_BADARG;
    if (out_lo < 0 || n_out < 0 || out_lo + n_out > (1ll << 40)) return TDC_E_BADARG;
    // the staged span of a tile and, at L == 1, the row beside it must fit the 64 KiB of LDS a workgroup can name
    const long long span = ((long long)(L - 1) + (long long)(TILE - 1) * M) / L + 2ll * K;
    const long long lds_bytes = (span + (L == 1 ? 2ll * K : 0)) * 4;
    const bool select = L == 1 && M == 1;
    if (!select && lds_bytes > 65536) return TDC_E_BADARG;
    if (n_out == 0) return 0;
    if ((n_out + TILE - 1) / TILE > 0x7fffffffll) return TDC_E_BADARG;

    pcm_src s;
    s.p = pcm; s.n_in = n_in; s.sample_stride = sample_stride; s.channel_stride = channel_stride;
    s.c0 = channel < 0 ? 0 : channel;
    s.nc = channel < 0 ? channels : 1;
    s.mean_of = channel < 0 ? channels : 0;
    // the vector form: a dense channel whose every 16-byte group of the track lands on its alignment, in every addressed channel
    bool vec = sample_stride == 1 && aligned((const char*)pcm + (long long)s.c0 * channel_stride * esize, 16) &&
               (s.nc == 1 || (channel_stride * esize) % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    if (fmt == S16) return launch<S16>(s, vec, L, M, table, K, out_lo, n_out, out, out_f32, (int)span, (size_t)lds_bytes, st);
    return launch<F32>(s, vec, L, M, table, K, out_lo, n_out, out, out_f32, (int)span, (size_t)lds_bytes, st);
}
