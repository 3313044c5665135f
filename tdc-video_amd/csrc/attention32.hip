// tdc_attention, long-sequence form for the ViT towers (S = 729 / 730 / 577, d = 64 / 72): flash-style
// softmax(Q K^T * scale) V on v_mfma_f32_32x32x16 tiles.
//
// Why a second kernel: the 16x16x32 form (attention.hip) is bound by the SIMD's vector issue port - per 64 x 64 score tile
// and wave it issues 64 MFMAs (8 issue cycles each) beside ~1000 cycles of softmax VALU work, and its row maximum needs
// two cross-lane exchanges per 16 values.  The 32x32x16 MFMA does twice the work per issue (8 of its 32 cycles), and in
// its C layout a lane holds 16 scores of ONE query (query = lane & 31, keys on the registers): the row maximum / row sum
// are in-register chains plus a single exchange between the two lane halves, the S accumulator converts in place into
// the B operand of the PV product (cdna_hip_programming.md 3, "An accumulator tile as the next MFMA's operand") and the
// output accumulator has the query on the lane again, so the rescale needs no cross-lane traffic either.
//
// Workgroup = 4 waves; a wave owns QB blocks of 32 query rows of one (batch, head); K / V tiles of 64 keys go
// global -> registers -> LDS, double buffered: the loads of tile t+2 are in flight and tile t+1 is written to the other
// buffer while tile t is computed; ONE barrier per tile.
//   S^T[key, q] = K Q^T      A = K rows from LDS (ds_read_b128; 16-byte chunks XOR-swizzled against the 16-lane groups of
//                            a b128 read), B = Q^T held in registers for the whole kernel
//   O^T[d, q] += V^T P^T     A = V^T through ds_read_b64_tr_b16 from the row-major V tile (k-slot (h, j) of step s <-> key
//                            16 s + 8 (j >> 2) + 4 h + (j & 3), the order the S accumulator has), B = P^T = exp2(S^T c - m)
//                            converted pairwise in place
// Head dim 72 runs with the QK^T contraction padded to 80 (5 k-steps of 16; the 16x16x32 form pads to 96) and 3 output
// blocks of 32.  Two query blocks per wave need 96 (O) + 64 (S) + 40 (Q) registers, which leaves none for staging, so at
// head dim exactly 72 (DMA = true) K / V go global -> LDS directly (global_load_lds_dwordx4, 16 bytes per lane).  A
// wave-instruction writes 64 consecutive chunks, so the LDS image is linear in the staging index and the layout is chosen
// through each lane's source address: K in 9-chunk (144-byte) rows, V in its 12-chunk rows.  Tile t+1's pieces are issued
// at the top of tile t into the other buffer and awaited (s_waitcnt vmcnt(0), in asm like the loads: the compiler does not
// see them) before the tile's single barrier.  P converts in place over S as above (the pf / s arrays share registers by
// liveness); Q fragments stay in registers.  The masked last tile takes the two query blocks one after the other.  Per-row
// arithmetic, tile order and the rounding of P are those of the register-staged one-block form, which head dim 80 still
// runs and -DATTN32_D72_QB1 selects for head dim 72 (A/B runs); -DATTN32_D64_DMA: the same staging at head dim 64 (A/B only).
#include "common.h"
#include "../../include/tdc_hip.h"
#include "attention_args.h"
#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ f32x16 mfma32(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <class T> __device__ __forceinline__ typename VecOf<T>::v4 tr_read32(const T* p) {
    s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
    return __builtin_bit_cast(typename VecOf<T>::v4, r);
}

// value of the other lane half (lane ^ 32)
__device__ __forceinline__ float other_half(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(((int)(threadIdx.x & 63) ^ 32) * 4, __builtin_bit_cast(int, v)));
}

constexpr int KT32 = 64;   // keys per tile (2 key blocks of 32)

// a pointer the compiler can prove wave-uniform (scalar registers): the base of an LDS-DMA load
__device__ __forceinline__ const char* uniform_ptr(const void* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (const char*)(((unsigned long long)hi << 32) | lo);
}

// One LDS-DMA piece: lane l's 16 bytes at base + off go to LDS byte address lds_dst + 16 l (global_load_lds_dwordx4; the
// destination base travels in M0, written and restored in the same statement because the compiler owns M0).  As asm the load
// is outside hipcc's wait bookkeeping: it neither drains it early (toolchain lesson 4) nor waits for it at all - the
// caller's own s_waitcnt vmcnt(0) and a barrier stand between a piece and the first read of its bytes.  The leading s_nop
// covers a base that a v_readfirstlane has only just written.
__device__ __forceinline__ void glds16(const char* base, unsigned off, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(off), "s"(base), "s"(lds_dst) : "memory");
}
// The DMA form calls do_tile from more places; not inlined it passes its register arrays through scratch and the DMA's scalar
// operands lose their uniformity (toolchain lesson 9).
#define ATTN32_INLINE __attribute__((always_inline))
#ifndef ATTN32_THR
#define ATTN32_THR 8.0f
#endif

// DK: QK^T contraction width (64 or 80), NDB: output blocks of 32 columns (2 or 3), QB: 32-row query blocks per wave,
// DMA: K / V tiles by LDS-DMA (head dim exactly 64 or 72) instead of through registers
template <class T, int DK, int NDB, int QB, bool DMA>
__global__ __launch_bounds__(256, 2) void attn32_kernel(AttnArgs p) {
    typedef typename VecOf<T>::v8 v8;
    typedef typename VecOf<T>::v4 v4;
    constexpr int KS = DK / 16;                              // k-steps of the QK^T product
    constexpr int DREAL = DK == 80 ? 72 : 64;                // DMA: the head dim itself, a compile-time constant
    constexpr int NCH = DMA ? DREAL / 8 : DK / 8;            // 16-B chunks staged per K row
    // chunks per K row in LDS: 8 (128-byte rows, XOR swizzle) at head dim 64; at head dim 72 an ODD number of chunks (11 = 176-byte
    // rows, no swizzle): the 16 lanes a ds_read_b128 cycle serves hold 16 keys that are distinct mod 16, and 11 key mod 16 is a
    // permutation, so they hit 16 distinct 16-byte slots - and the staging writes (consecutive lanes = consecutive chunks of
    // consecutive keys) wrap onto an occupied slot once per 16 lanes instead of six times as with round 4's 256-byte rows, where
    // every row started on bank 0 (the d = 72 launches' 3.5 M conflict cycles, profiles/r04_attention_pmc_summary.txt)
    // DMA, head dim 72: 9 chunks = 144-byte rows holding exactly the row's 72 columns.  9 is odd like 11, so the same
    // argument keeps the ds_read_b128 cycles conflict free; the tile shrinks from 11 to 9 KiB.  The fifth k-step's upper half
    // (columns 72-79, which meet zeroed Q columns) re-reads chunk 8 where the register path reads its clamped duplicate of
    // chunk 8: the same bits, and no read leaves the row.
    constexpr int KCH = (NCH <= 8) ? 8 : (NCH | 1);
    constexpr int KROW = KCH * 8;
    constexpr int VCH = NDB * 4;                             // 16-B chunks per V row (64 B per output block)
    constexpr int VROW = VCH * 8;                            // d = 64: 128-byte rows, swizzled; d = 72: 192-byte rows
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* Ks = (T*)smem_raw;                                    // [2][KT32 * KROW]
    T* Vs = Ks + 2 * KT32 * KROW;                            // [2][KT32 * VROW]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    // Workgroups are dispatched round-robin over the 8 XCDs (private L2s): every XCD takes a contiguous range of logical ids, so
    // that the query blocks of one (batch, head) - consecutive logical ids, which read the same K / V - run on ONE L2 and at
    // about the same time (cdna_hip_programming.md T1).  In dispatch order they land on different XCDs and each fetches that
    // head's K / V through the fabric for itself: measured 494 -> 532 TFLOP/s at head dim 72, 686 -> 707 at 64 (same box).
    const int nqb = (p.sq + 128 * QB - 1) / (128 * QB);
    const int nwg = gridDim.x, q8 = nwg >> 3, r8 = nwg & 7, xcd = blockIdx.x & 7;
    const int lid = ((xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
    const int bh = lid / nqb, qblk = lid - bh * nqb;
    const int b = bh / p.heads, h = bh - b * p.heads;
    const int q0 = qblk * (128 * QB) + wave * (32 * QB);
    const int d = p.d;
    const T* Q = (const T*)p.q + b * p.q_bs + h * d;
    // per-item K / V source and key count (tdc_attn_desc.kv_index / k_len), as in attention.hip: the item runs the tiling of a
    // uniform launch with sk = k_len[b]; keys at and beyond it are never loaded (row indices clamped to sk - 1)
    const int kvb = p.kv_index ? p.kv_index[b] : b;
    const int sk = p.k_len ? p.k_len[b] : p.sk;
    const T* K = (const T*)p.k + kvb * p.k_bs + h * d;
    const T* V = (const T*)p.v + kvb * p.v_bs + h * d;
    T* O = (T*)p.o + b * p.o_bs + h * d;

    // 8 elements row[c0 .. c0+7], address clamped into the row (head dim % 8 == 0: the launcher's vec_ok)
    auto load8 = [&](const T* row, int c0) -> v8 {
        const int cc = c0 < d ? c0 : d - 8;
        return *(const v8*)(row + cc);
    };

    // ---- Q^T fragments (B operand): lane (r, hh) holds Q[q0 + 32 qb + r][16 ks + 8 hh .. +7]; columns >= d zeroed
    v8 qf[QB][KS];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        int qr = q0 + qb * 32 + r;
        if (qr > p.sq - 1) qr = p.sq - 1;
        const T* row = Q + (long long)qr * p.q_rs;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int c0 = ks * 16 + hh * 8;
            v8 x = load8(row, c0);
            if (c0 >= d)
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = (T)0.f;
            qf[qb][ks] = x;
        }
    }

    // ---- staging: K tile 64 x NCH chunks, V tile 64 x VCH chunks (V columns >= d: clamped duplicates that only feed
    //      output columns >= d, which are never stored)
    constexpr int KLD = (KT32 * NCH + 255) / 256, VLD = (KT32 * VCH + 255) / 256;
    constexpr bool K_EXACT = (KT32 * NCH) % 256 == 0, V_EXACT = (KT32 * VCH) % 256 == 0;
    v8 kreg[KLD], vreg[VLD];
    auto issue_loads = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < KLD; ++i) {
            int idx = tid + i * 256;
            if (!K_EXACT && idx > KT32 * NCH - 1) idx = KT32 * NCH - 1;
            const int key = idx / NCH, c = idx - key * NCH;
            int kr = kv0 + key; if (kr > sk - 1) kr = sk - 1;
            kreg[i] = load8(K + (long long)kr * p.k_rs, c * 8);
        }
#pragma unroll
        for (int i = 0; i < VLD; ++i) {
            int idx = tid + i * 256;
            if (!V_EXACT && idx > KT32 * VCH - 1) idx = KT32 * VCH - 1;
            const int key = idx / VCH, c = idx - key * VCH;
            int kr = kv0 + key; if (kr > sk - 1) kr = sk - 1;
            vreg[i] = load8(V + (long long)kr * p.v_rs, c * 8);
        }
    };
    // K, 128-byte rows: physical chunk = chunk ^ ((key >> 1) & 7) - the 16 lanes one ds_read_b128 cycle serves ({0-3, 12-15,
    // 20-27} / {4-11, 16-19, 28-31} of each half) then hit 16 distinct 16-byte slots; 176-byte rows do that by their stride.
    // V: 128-byte rows (d = 64): the 64-byte half is XORed with (key >> 1) & 1 so that the four keys of one transposed read
    // fall on four different 64-byte bank groups; 192-byte rows (3 output blocks) do that by their stride.
    auto kswz = [](int key, int c) { return KCH == 8 ? (c ^ ((key >> 1) & 7)) : c; };
    auto vswz = [](int key, int c) { return NDB == 2 ? (c ^ (((key >> 1) & 1) << 2)) : c; };
    auto write_lds = [&](int buf) {
        T* kd = Ks + buf * (KT32 * KROW);
        T* vd = Vs + buf * (KT32 * VROW);
#pragma unroll
        for (int i = 0; i < KLD; ++i) {
            const int idx = tid + i * 256;
            const int key = idx / NCH, c = idx - key * NCH;
            if (K_EXACT || idx < KT32 * NCH) *(v8*)(kd + key * KROW + (kswz(key, c) << 3)) = kreg[i];
        }
#pragma unroll
        for (int i = 0; i < VLD; ++i) {
            const int idx = tid + i * 256;
            const int key = idx / VCH, c = idx - key * VCH;
            if (V_EXACT || idx < KT32 * VCH) *(v8*)(vd + key * VROW + (vswz(key, c) << 3)) = vreg[i];
        }
    };

    // ---- DMA staging: a wave-instruction writes 64 consecutive 16-byte chunks, so the LDS image is linear in the staging index
    //      idx = 64 piece + lane = KCH key + physical chunk (VCH for V), and the layouts above are reached through each lane's
    //      SOURCE address: physical chunk pc of a row holds logical chunk kswz(key, pc) / vswz(key, pc) (both are involutions).
    //      V keeps its 192-byte rows at head dim 72 (chunks 9-11: clamped duplicates of columns 64-71, as on the register path):
    //      the four keys of one ds_read_b64_tr_b16 sit 192 bytes apart, on four different 64-byte bank groups of the 256-byte
    //      bank cycle (0, 192, 128, 64); 160-byte rows (10 chunks) would put them at 0, 160, 64, 224, where the fourth wraps onto
    //      the first's banks, and 144-byte rows at 0, 144, 32, 176, which overlap pairwise.
    //      K: KT32 * KCH / 64 pieces (9 at head dim 72: wave 0 takes three, the others two), V: KT32 * VCH / 64 (12: three each).
    //      No staging registers: what stays live across the tile loop is one 32-bit source offset per piece.
    constexpr int KPC = KT32 * KCH / 64, VPC = KT32 * VCH / 64;
    constexpr int KPW = (KPC + 3) / 4, VPW = (VPC + 3) / 4;
    static_assert(!DMA || ((KT32 * KCH) % 64 == 0 && (KT32 * VCH) % 64 == 0 && NCH == KCH), "DMA pieces are whole wave-instructions");
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const char* Kb = nullptr; const char* Vb = nullptr;
    unsigned lds0 = 0;
    unsigned koff[KPW], voff[VPW];
    auto k_src = [&](int i, int kmax) __attribute__((always_inline)) -> unsigned {          // byte offset of this lane's chunk of K piece wave + 4 i within the tile
        const int idx = (wave_u + 4 * i) * 64 + lane;
        int key = idx / KCH;
        const int cc = kswz(key, idx - key * KCH);
        if (key > kmax) key = kmax;
        return (unsigned)(key * p.k_rs + cc * 8) * 2u;
    };
    auto v_src = [&](int i, int kmax) __attribute__((always_inline)) -> unsigned {
        const int idx = (wave_u + 4 * i) * 64 + lane;
        int key = idx / VCH;
        int c0 = vswz(key, idx - key * VCH) * 8;
        if (c0 > DREAL - 8) c0 = DREAL - 8;
        if (key > kmax) key = kmax;
        return (unsigned)(key * p.v_rs + c0) * 2u;
    };
    if (DMA) {
        Kb = uniform_ptr(K); Vb = uniform_ptr(V);
        lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(__attribute__((address_space(3))) char*)smem_raw);
#pragma unroll
        for (int i = 0; i < KPW; ++i) koff[i] = k_src(i, KT32 - 1);
#pragma unroll
        for (int i = 0; i < VPW; ++i) voff[i] = v_src(i, KT32 - 1);
    }
    // tile `tile` -> buffer tile & 1.  Keys at and beyond sk are never loaded: in the (at most one) tile that holds some, the row
    // index is clamped to sk - 1 as on the register path and the offsets are computed afresh.
    auto dma_tile = [&](int tile) __attribute__((always_inline)) {
        const int kv0 = tile * KT32, buf = tile & 1;
        const char* kb = Kb + (long long)kv0 * p.k_rs * 2;
        const char* vb = Vb + (long long)kv0 * p.v_rs * 2;
        const unsigned kd = lds0 + buf * (KT32 * KROW * 2), vd = lds0 + (2 * KT32 * KROW + buf * KT32 * VROW) * 2;
        if (kv0 + KT32 <= sk) {
#pragma unroll
            for (int i = 0; i < KPW; ++i)
                if (4 * i + 3 < KPC || wave_u + 4 * i < KPC) glds16(kb, koff[i], kd + (wave_u + 4 * i) * 1024);
#pragma unroll
            for (int i = 0; i < VPW; ++i)
                if (4 * i + 3 < VPC || wave_u + 4 * i < VPC) glds16(vb, voff[i], vd + (wave_u + 4 * i) * 1024);
        } else {
#pragma unroll
            for (int i = 0; i < KPW; ++i)
                if (4 * i + 3 < KPC || wave_u + 4 * i < KPC) glds16(kb, k_src(i, sk - 1 - kv0), kd + (wave_u + 4 * i) * 1024);
#pragma unroll
            for (int i = 0; i < VPW; ++i)
                if (4 * i + 3 < VPC || wave_u + 4 * i < VPC) glds16(vb, v_src(i, sk - 1 - kv0), vd + (wave_u + 4 * i) * 1024);
        }
    };

    f32x16 o_acc[QB][NDB];
    float m_run[QB], l_run[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        m_run[qb] = -INFINITY;
        l_run[qb] = 0.f;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int e = 0; e < 16; ++e) o_acc[qb][db][e] = 0.f;
    }

    const int ntiles = (sk + KT32 - 1) / KT32;
    const float c = p.scale_log2;

    // NQ = query blocks of this wave that hold at least one row < sq (the first NQ ones), NKB = key blocks of the tile that hold
    // at least one key < sk: S = 729 / 730 / 577 leave 32-row blocks past the end of the sequence on both sides (the last
    // workgroup of a head, the last tile of the keys), whose MFMAs and softmax are skipped whole
    // Query blocks Q0 .. NQ - 1 of the wave are worked on: all of them at once but for the masked last tile at two blocks per
    // wave and head dim 72, see run below.
    auto do_tile = [&](const int tile, auto partial_c, auto q0_c, auto nq_c, auto nkb_c) ATTN32_INLINE {
        constexpr bool PARTIAL = decltype(partial_c)::value;
        constexpr int Q0 = decltype(q0_c)::value, NQ = decltype(nq_c)::value, NKB = decltype(nkb_c)::value;
        // second pass over the masked tile: lane terms recomputed instead of being kept, and spilled, across the first pass
        // (toolchain lesson 7)
        int ln = lane;
        if (PARTIAL && DMA && QB > 1 && (Q0 > 0 || NKB == 2)) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const int r = ln & 31, hh = ln >> 5;
        const int buf = tile & 1;
        const T* kt_ = Ks + buf * (KT32 * KROW);
        const T* vt_ = Vs + buf * (KT32 * VROW);
        const int kv0 = tile * KT32;
        // tile t+1 (in registers since the previous iteration) -> the other buffer; every wave passed the barrier that ended
        // iteration t-1, so nobody reads that buffer any more.  Then the loads of tile t+2 go out.
        // DMA: there are no registers to park tile t+2 in, so what goes out here is tile t+1, straight into the other buffer
        // (free for the same reason), and it has this whole tile's compute to land in.
        if (!PARTIAL) {
            if (DMA) {
                dma_tile(tile + 1);
            } else {
                write_lds(buf ^ 1);
                if (tile + 2 < ntiles) issue_loads((tile + 2) * KT32);
            }
        }

        // ---- S^T = K Q^T: s[qb][kb] holds, for query r, keys kv0 + 32 kb + (e & 3) + 8 (e >> 2) + 4 hh
        f32x16 s[QB][2];
#pragma unroll
        for (int qb = Q0; qb < NQ; ++qb)
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) s[qb][kb][e] = 0.f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const int key = kb * 32 + r;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int ch = (DMA && ks * 2 + 1 > NCH - 1) ? NCH - 1 : ks * 2 + hh;
                const v8 kf = *(const v8*)(kt_ + key * KROW + (kswz(key, ch) << 3));
#pragma unroll
                for (int qb = Q0; qb < NQ; ++qb) s[qb][kb] = mfma32(kf, qf[qb][ks], s[qb][kb]);
            }
        }
        // ---- online softmax in base 2 on the raw scores; P^T fragments in place
        v8 pf[QB][2][2];
#pragma unroll
        for (int qb = Q0; qb < NQ; ++qb) {
            if (PARTIAL) {
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (kv0 + kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh >= sk) s[qb][kb][e] = -INFINITY;
            }
            float mx = fmaxf(s[qb][0][0], s[qb][0][1]);
#pragma unroll
            for (int e = 2; e < 16; e += 2) mx = __builtin_fmaxf(__builtin_fmaxf(mx, s[qb][0][e]), s[qb][0][e + 1]);
            if (NKB == 2) {
#pragma unroll
                for (int e = 0; e < 16; e += 2) mx = __builtin_fmaxf(__builtin_fmaxf(mx, s[qb][1][e]), s[qb][1][e + 1]);
            }
            mx = fmaxf(mx, other_half(mx));
            // deferred rescale (cdna_hip_programming.md T13): the running maximum only follows the tile's when that exceeds it by
            // more than ATTN32_THR (base-2 exponent units) - P stays <= 2^THR, O and l are rescaled in the first tile or two only
            const float m_cand = mx * c;
            const float m_new = (m_cand > m_run[qb] + ATTN32_THR) ? m_cand : m_run[qb];
            const float alpha = __builtin_amdgcn_exp2f(m_run[qb] - m_new);
            m_run[qb] = m_new;
#ifndef ATTN32_PACKED
            // exponent arguments and row sums as SINGLE-value fma / add (two accumulators): packed fp32 arithmetic (v_pk_fma_f32 /
            // v_pk_add_f32) halves the instruction count but never runs beside the partner wave's MFMAs (tools/mfma_valu_overlap.cpp,
            // MI355X_MICROARCH.md "packed f32 VALU ... an anti-lever beside MFMAs"); round 5, same box, three runs each
            // (profiles/r05_attention32_scalar_ab.log): d = 64 716-733 -> 744-756 TFLOP/s, d = 72 512-518 -> 512-522; s_setprio around the
            // softmax or around the MFMA sections: no gain.  The empty
            // asm keeps the SLP vectoriser from re-packing the pairs.  (-DATTN32_PACKED: the packed form of rounds 2-4.)
            float rs0 = 0.f, rs1 = 0.f;
            const float nm = -m_new;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int st = 0; st < 2; ++st)
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        float z0 = __builtin_fmaf(s[qb][kb][st * 8 + j], c, nm), z1 = __builtin_fmaf(s[qb][kb][st * 8 + j + 1], c, nm);
                        asm volatile("" : "+v"(z0), "+v"(z1));
                        const float e0 = __builtin_amdgcn_exp2f(z0), e1 = __builtin_amdgcn_exp2f(z1);
                        rs0 += e0; rs1 += e1;
                        const typename VecOf<T>::v2 e16 = cvt2<T>(e0, e1);
                        pf[qb][kb][st][j] = e16[0];
                        pf[qb][kb][st][j + 1] = e16[1];
                    }
            // masked tile at two query blocks per wave: the scheduler otherwise sinks the row-sum adds below the PV product and
            // spills the exponentials they wait for; the V reads stay below this point
            if (PARTIAL && DMA && QB > 1) asm volatile("" : "+v"(rs0), "+v"(rs1) : : "memory");
            if (PARTIAL && DMA && QB > 1) {      // ... and the conversions of P below the O rescale's branch
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) asm volatile("" : "+v"(pf[qb][kb][0]), "+v"(pf[qb][kb][1]));
            }
            l_run[qb] = l_run[qb] * alpha + (rs0 + rs1);
#else
            // exponent arguments and row sums on register pairs (v_pk_fma_f32 / v_pk_add_f32: one issue slot per two values)
            const f32x2_t c2 = {c, c}, nm2 = {-m_new, -m_new};
            f32x2_t rs2 = {0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int st = 0; st < 2; ++st)
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        const f32x2_t z = __builtin_elementwise_fma((f32x2_t){s[qb][kb][st * 8 + j], s[qb][kb][st * 8 + j + 1]}, c2, nm2);
                        const f32x2_t e = {__builtin_amdgcn_exp2f(z[0]), __builtin_amdgcn_exp2f(z[1])};
                        rs2 += e;
                        const typename VecOf<T>::v2 e16 = cvt2<T>(e[0], e[1]);     // one v_cvt_pk per pair, f16 too
                        pf[qb][kb][st][j] = e16[0];
                        pf[qb][kb][st][j + 1] = e16[1];
                    }
            l_run[qb] = l_run[qb] * alpha + (rs2[0] + rs2[1]);
#endif
            // the running max only moves in the first few tiles: skip the O rescale when no lane's max changed
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int db = 0; db < NDB; ++db)
#pragma unroll
                    for (int e = 0; e < 16; ++e) o_acc[qb][db][e] *= alpha;
            }
        }
        // ---- O^T += V^T P^T.  16-lane group G of the wave (r >> 4 within each half) reads the 4-key x 16-column block at keys
        //      32 kb + 16 st + 4 hh (+ 8), columns 32 db + 16 (r >> 4): lane 4 q + pp supplies row q, columns 4 pp ..
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            if (NQ == Q0) break;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const int li = r & 15, qq = li >> 2, pp = li & 3;
                    const int key = kb * 32 + st * 16 + hh * 4 + qq;
                    const int col = db * 32 + (r >> 4) * 16 + pp * 4;      // multiple of 4: chunk col >> 3, 8-byte half (col >> 2) & 1
                    const T* a0 = vt_ + key * VROW + (vswz(key, col >> 3) << 3) + (col & 4);
                    const T* a1 = vt_ + (key + 8) * VROW + (vswz(key + 8, col >> 3) << 3) + (col & 4);
                    const v4 lo = tr_read32<T>(a0);
                    const v4 hi = tr_read32<T>(a1);
                    v8 vf;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { vf[e] = lo[e]; vf[4 + e] = hi[e]; }
#pragma unroll
                    for (int qb = Q0; qb < NQ; ++qb) o_acc[qb][db] = mfma32(vf, pf[qb][kb][st], o_acc[qb][db]);
                }
        }
        // this wave's pieces of tile t+1 have landed (the DMA is invisible to the compiler's own waits); past the barrier so have
        // everyone's
        if (DMA && !PARTIAL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (!(DMA && PARTIAL)) __syncthreads();    // tile t+1 is visible; everyone is done reading tile t
    };

    // prologue: tile 0 -> buffer 0, tile 1 in registers (DMA: tile 0 only)
    if (DMA) {
        dma_tile(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        issue_loads(0);
        write_lds(0);
        if (ntiles > 1) issue_loads(KT32);
    }
    __syncthreads();
    int nq = (p.sq - q0 + 31) >> 5;                              // wave-uniform
    nq = nq < 0 ? 0 : (nq > QB ? QB : nq);
    const bool last_two = sk - (ntiles - 1) * KT32 > 32;       // the last tile's second key block holds valid keys
    auto run = [&](auto nq_c) ATTN32_INLINE {
        typedef std::integral_constant<int, 2> two;
        typedef std::integral_constant<int, 1> one;
        typedef std::integral_constant<int, 0> zero;
        constexpr int NQ = decltype(nq_c)::value;
        for (int tile = 0; tile < ntiles - 1; ++tile) do_tile(tile, std::false_type(), zero(), nq_c, two());
        if (DMA && NQ == 2 && NDB == 3) {
            // 96 O + 64 S + 40 Q registers leave no room for the mask's terms beside two blocks' scores (39 spilled VGPRs): the
            // masked tile - one in twelve at S = 729, and nothing follows it - takes the wave's two query blocks one after the
            // other, re-reading its K / V fragments.  Per-row arithmetic is what it is in the other order.
            // (the tile index is made opaque per call: what the four bodies have in common - the first K fragment reads, the
            // mask's compares - is otherwise hoisted above the branch into registers of its own, toolchain lesson 8)
            auto last = [&]() __attribute__((always_inline)) { int t = ntiles - 1; asm volatile("" : "+s"(t)); return t; };
            if (last_two) { do_tile(last(), std::true_type(), zero(), one(), two()); __builtin_amdgcn_sched_barrier(0); do_tile(last(), std::true_type(), one(), two(), two()); }
            else { do_tile(last(), std::true_type(), zero(), one(), one()); __builtin_amdgcn_sched_barrier(0); do_tile(last(), std::true_type(), one(), two(), one()); }
        } else {
            if (last_two) do_tile(ntiles - 1, std::true_type(), zero(), nq_c, two());
            else do_tile(ntiles - 1, std::true_type(), zero(), nq_c, one());
        }
    };
    if (nq >= QB) run(std::integral_constant<int, QB>());
    else if (QB > 1 && nq == 1) run(std::integral_constant<int, 1>());
    else run(std::integral_constant<int, 0>());

    // ---- finalise: lane (r, hh) holds O[q = q0 + 32 qb + r][32 db + 8 (e >> 2) + 4 hh + (e & 3)]
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        float l = l_run[qb];
        l += other_half(l);
        const float inv = 1.0f / l;
        const int qr = q0 + qb * 32 + r;
        if (qr >= p.sq) continue;
        T* orow = O + (long long)qr * p.o_rs;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int col = db * 32 + g4 * 8 + hh * 4;
                if (col + 3 < d) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = o_acc[qb][db][g4 * 4 + e] * inv;
                    *(v4*)(orow + col) = cvt4<T>(o);
                }
            }
    }
}

template <class T, int DK, int NDB, int QB, bool DMA>
int launch32(const AttnArgs& a, int batch, hipStream_t st) {
    constexpr int NCH = DMA ? (DK == 80 ? 9 : 8) : DK / 8;
    constexpr int KCH = (NCH <= 8) ? 8 : (NCH | 1);
    constexpr int lds = 2 * KT32 * (KCH * 8 + NDB * 32) * 2;
    static bool attr_dev[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_dev[dev]) {
        HIP_CHECK_RET(hipFuncSetAttribute((const void*)attn32_kernel<T, DK, NDB, QB, DMA>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_dev[dev] = true;
    }
    dim3 grid(((a.sq + 128 * QB - 1) / (128 * QB)) * a.heads * batch);   // 1-D: the kernel maps ids to (batch, head, query block)
    hipLaunchKernelGGL((attn32_kernel<T, DK, NDB, QB, DMA>), grid, dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

}  // namespace

// entry for attention.hip: returns -1 when this form does not apply (the caller falls through to the 16x16 kernels)
int tdc_attention32(const AttnArgs& a, int batch, int dtype, hipStream_t st) {
    if (a.bias || !a.vec_ok || a.sq < 256 || a.sk < 64) return -1;
#ifdef ATTN32_D64_DMA       // A/B only: head dim 64 with DMA staging (NOTES 2, tower attention)
    if (a.d == 64) return dtype == TDC_F16 ? launch32<f16, 64, 2, 2, true>(a, batch, st) : launch32<bf16, 64, 2, 2, true>(a, batch, st);
#else
    if (a.d == 64) return dtype == TDC_F16 ? launch32<f16, 64, 2, 2, false>(a, batch, st) : launch32<bf16, 64, 2, 2, false>(a, batch, st);
#endif
#ifndef ATTN32_D72_QB1      // -DATTN32_D72_QB1: head dim 72 on the register-staged one-block form below, for A/B runs
    if (a.d == 72) return dtype == TDC_F16 ? launch32<f16, 80, 3, 2, true>(a, batch, st) : launch32<bf16, 80, 3, 2, true>(a, batch, st);
#endif
    if (a.d > 64 && a.d <= 80) return dtype == TDC_F16 ? launch32<f16, 80, 3, 1, false>(a, batch, st) : launch32<bf16, 80, 3, 1, false>(a, batch, st);
    return -1;
}
