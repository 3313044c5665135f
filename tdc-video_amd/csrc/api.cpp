// Composite entry points of the C ABI: whole-stage launch sequences over the primitive kernels (no Python between the
// launches; graph-capturable: nothing here allocates or synchronises).
#include "../../include/tdc_hip.h"
#include "profile.h"
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <hip/hip_runtime.h>

namespace {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int pad64i(int x) { return (x + 63) / 64 * 64; }

struct VitWs {
    size_t patches, x32, h16, qkv, attn, mlp, part, stats, total;   // fp8 towers: h16 holds the e4m3 LayerNorm rows
};

// row stride of the 16-bit MLP hidden buffer: fc1's output width (SwiGLU halves it), at least fc2's (padded) K
int vit_mlp_ld(const tdc_vit_model* m) {
    if (!m->n_layers) return 0;
    const tdc_vit_layer& L = m->layers_host[0];
    const int n1 = m->act == TDC_ACT_SWIGLU ? L.fc1.n / 2 : L.fc1.n;
    return n1 > L.fc2.k ? n1 : L.fc2.k;
}

VitWs vit_layout(const tdc_vit_model* m, int B, int H, int W) {
    const int gh = H / m->patch, gw = W / m->patch;
    const size_t P = (size_t)gh * gw, S = P + m->has_cls, rows = (size_t)B * S;
    const int Dp = pad64i(m->dim);
    const int kp = m->patch_lin.k;
    const int qkv_w = m->n_layers ? m->layers_host[0].qkv.n : 0;
    const int mlp_w = vit_mlp_ld(m);
    VitWs w;
    size_t off = 0;
    w.patches = off; off += al256((size_t)B * P * kp * 2);
    w.x32 = off;     off += al256(rows * Dp * 4);
    w.h16 = off;     off += al256(rows * Dp * 2);
    {   // fp8 level 2 parks the e4m3 MLP hidden (rows x fc2.k bytes) in the qkv buffer
        size_t qb = rows * qkv_w * 2, mb = (m->fp8 >= 2 && m->n_layers) ? rows * (size_t)m->layers_host[0].fc2.k : 0;
        w.qkv = off; off += al256(qb > mb ? qb : mb);
    }
    w.attn = off;    off += al256(rows * Dp * 2);
    w.mlp = off;     off += al256(rows * mlp_w * 2);
    w.part = off;    off += m->fused ? al256(rows * (size_t)(Dp / 64) * 8) : 0;
    w.stats = off;   off += (m->fused || m->fp8) ? al256(rows * 8) * (m->fp8 >= 3 ? 2 : 1) : 0;   // level 3: fc1's out_stats
    w.total = off;
    return w;
}

#define RET_IF(x) do { int _rc = (x); if (_rc) { fprintf(stderr, "[tdc_hip] %s -> %d (%s:%d)\n", #x, _rc, __FILE__, __LINE__); return _rc; } } while (0)

// The one builder of tdc_gemm_desc: C[M, L.n] = A[M, L.k] L.w^T + L.b on 16-bit operands and a 16-bit C of type `dtype`, identity
// row maps.  Whatever else a launch does is named at its call site: Gemm(...).act(a).run(stream).
struct Gemm {
    tdc_gemm_desc d;
    Gemm(const void* A, int lda, const tdc_lin& L, void* C, int ldc, int M, int dtype) {
        memset(&d, 0, sizeof(d));
        d.A = A; d.lda = lda; d.W = L.w; d.ldw = L.k; d.C = C; d.ldc = ldc; d.bias = L.b;
        d.M = M; d.N = L.n; d.K = L.k; d.dtype = dtype;
    }
    Gemm& act(int a) { d.act = a; return *this; }
    Gemm& out_f32() { d.out_f32 = 1; return *this; }
    Gemm& ldw(int ld) { d.ldw = ld; return *this; }                               // a "weight" whose row stride is not its K
    Gemm& res(const void* r, int ld, int f32) { d.res = r; d.ldres = ld; d.res_f32 = f32; return *this; }
    Gemm& a_map(tdc_rowmap m) { d.a_map = m; return *this; }
    Gemm& c_map(tdc_rowmap m) { d.c_map = m; return *this; }
    Gemm& r_map(tdc_rowmap m) { d.r_map = m; return *this; }
    // LayerNorm fusion, consumer side: (mean, rstd) per row and the row sums of the gamma-folded weight; with in_fp8 the same two
    // operands carry the dequantisation scales (tdc_hip.h)
    Gemm& fold(const float* stats, const float* c1) { d.ln_stats = stats; d.ln_c1 = c1; return *this; }
    // ... producer side: the 16-bit copy of the updated rows (NULL over a 16-bit stream) and the per-slot (mean, M2) partials
    Gemm& emit(void* x16, int ldx16, float* part) { d.x16 = x16; d.ldx16 = ldx16; d.ln_part = part; return *this; }
    Gemm& in_fp8() { d.in_fp8 = 1; return *this; }
    // e4m3 output + out_stats for the fp8-operand GEMM (weight scale next_wscale) behind it
    Gemm& out_fp8(float* out_stats, float w2max, float bmax, float next_wscale) {
        d.out_fp8 = 1; d.out_stats = out_stats; d.out_w2max = w2max; d.out_bmax = bmax; d.out_wscale = next_wscale;
        return *this;
    }
    Gemm& c16(int type) { d.c16_dtype_p1 = type + 1; return *this; }              // 16-bit C / res of another type than `dtype`
    Gemm& c_pad8() { d.c_pad8 = 1; return *this; }
    int run(void* st) const { return tdc_gemm(&d, st); }
};

// The one builder of tdc_ln_desc: LayerNorm over `cols` columns of x [rows, ldx]; the outputs (y16 / y32 / y8) and the rest by name
struct Ln {
    tdc_ln_desc d;
    Ln(const void* x, int ldx, int x_f32, const float* g, const float* b, float eps, int rows, int cols, int dtype) {
        memset(&d, 0, sizeof(d));
        d.x = x; d.ldx = ldx; d.x_f32 = x_f32; d.gamma = g; d.beta = b; d.eps = eps; d.rows = rows; d.cols = cols; d.dtype = dtype;
    }
    Ln& y16(void* y, int ld) { d.y16 = y; d.ldy16 = ld; return *this; }
    Ln& y32(float* y, int ld) { d.y32 = y; d.ldy32 = ld; return *this; }
    // e4m3 rows + per-row scales (stats) for an fp8-operand GEMM with per-tensor weight scale `wscale`
    Ln& y8(void* y, int ld, float* stats, float wscale) { d.y8 = y; d.ldy8 = ld; d.y8_stats = stats; d.y8_wscale = wscale; return *this; }
    Ln& y_map(tdc_rowmap m) { d.y_map = m; return *this; }
    Ln& add(const float* table, int ld, int period, int mode) { d.add = table; d.ldadd = ld; d.add_period = period; d.add_mode = mode; return *this; }
    Ln& x_type(int type) { d.x_dtype_p1 = type + 1; return *this; }               // 16-bit x of another type than `dtype`
    int run(void* st) const { return tdc_layernorm(&d, st); }
};

// self-attention over a packed qkv buffer [batch * S, ldqkv] (q | k | v at columns 0, D, 2 D) -> o [batch * S, ldo]; k_len: optional
// per-item key count (tdc_attn_desc.k_len)
int self_attention(const char* qkv, int ldqkv, void* o, int ldo, int batch, int S, int heads, int head_dim, int D, float scale,
                   int dtype, void* st, const int* k_len = nullptr) {
    tdc_attn_desc a;
    memset(&a, 0, sizeof(a));
    a.q = qkv; a.k = qkv + (size_t)D * 2; a.v = qkv + (size_t)2 * D * 2; a.o = o;
    a.q_bs = a.k_bs = a.v_bs = (long long)S * ldqkv; a.o_bs = (long long)S * ldo;
    a.q_rs = a.k_rs = a.v_rs = ldqkv; a.o_rs = ldo;
    a.batch = batch; a.heads = heads; a.head_dim = head_dim; a.sq = S; a.sk = S; a.scale = scale; a.dtype = dtype;
    a.k_len = k_len;
    return tdc_attention(&a, st);
}

struct QfWs {
    size_t h32, h16, kv, vt, ldvt, qkv, ctx, ctxq, cq, t32, t32b, mq, mt, total;
};

// form of the cross-attention block (tdc_qformer_model.xattn_mode, 0 when the weights or the shape do not allow the request):
// 2 = the whole block in one kernel per layer, 1 = its output projection + residual + LayerNorm in one kernel, 0 = per-kernel
int qf_mode(const tdc_qformer_model* m, int K, int Nenc) {
    if (m->xattn_mode <= 0) return 0;
    bool q_t = true, o_t = true;
    for (int l = 0; l < m->n_layers; ++l)
        if (m->layers_host[l].has_cross) {
            q_t = q_t && m->layers_host[l].cross_q_tiled;
            o_t = o_t && m->layers_host[l].cross_out_tiled;
        }
    if (m->xattn_mode >= 2 && q_t && o_t && m->cross_k.w && m->cross_v.w && m->cross_k.n == m->cross_v.n &&
        m->cross_k.k == m->cross_v.k && tdc_qformer_xattn_supported(m->dim, m->heads, K, Nenc))
        return 2;
    if (o_t && tdc_qformer_xattn_supported(m->dim, m->heads, K, 8)) return 1;
    return 0;
}
bool qf_fused(const tdc_qformer_model* m, int K, int Nenc) { return qf_mode(m, K, Nenc) == 2; }

QfWs qf_layout(const tdc_qformer_model* m, int F, int K, int Lt, int Nenc) {
    const size_t S = (size_t)K + Lt, rows = (size_t)F * S, Dp = pad64i(m->dim);
    const size_t U = m->prompts ? (size_t)m->prompts->enc_frames : (size_t)F;   // frames the K/V projections run over
    const size_t ffn = m->layers_host[0].fq2.k;
    QfWs w;
    size_t off = 0;
    w.h32 = off;  off += al256(rows * Dp * 4);
    w.h16 = off;  off += al256(rows * Dp * 2);
    w.vt = 0; w.ldvt = 0;
    if (qf_fused(m, K, Nenc)) {     // keys [F*Nenc, n_cross*dim] and transposed values [n_cross*dim, ldvt]
        w.ldvt = (U * Nenc + 4 + 63) / 64 * 64;     // + 4: the half-valid last key group of a frame is read as 8 columns
        w.kv = off;   off += al256(U * Nenc * m->cross_k.n * 2);
        w.vt = off;   off += al256((size_t)m->cross_v.n * w.ldvt * 2);
    } else {
        w.kv = off;   off += al256(U * Nenc * m->cross_kv.n * 2);
    }
    w.qkv = off;  off += al256(rows * m->layers_host[0].qkv.n * 2);
    w.ctx = off;  off += al256(rows * Dp * 2);
    w.ctxq = off; off += al256((size_t)F * K * Dp * 2);
    w.cq = off;   off += al256((size_t)F * K * Dp * 2);
    w.t32 = off;  off += al256(rows * Dp * 4);
    w.t32b = off; off += al256((size_t)F * (Lt > 0 ? Lt : 1) * Dp * 4);
    w.mq = off;   off += al256((size_t)F * K * ffn * 2);
    w.mt = off;   off += al256((size_t)F * (Lt > 0 ? Lt : 1) * ffn * 2);
    w.total = off;
    return w;
}

}  // namespace

extern "C" size_t tdc_qformer_workspace_bytes(const tdc_qformer_model* m, int F, int K, int Lt, int Nenc) {
    if (!m || !m->layers_host || F <= 0 || K <= 0 || Nenc <= 0) return 0;
    if (m->prompts && m->prompts->enc_frames <= 0) return 0;
    return qf_layout(m, F, K, Lt, Nenc).total;
}

extern "C" int tdc_qformer_fwd(const tdc_qformer_model* m, const void* enc, int ldenc, int F, int Nenc,
                               const void* query, int ldq, const int* qsrc, const int* ids, int Lt, int K, void* out,
                               int ldo, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || !query || !qsrc || !out || !workspace || F <= 0 || K <= 0 || Lt < 0) return TDC_E_BADARG;
    // kept K/V (tdc_qformer_model.kv_keep): a caller-owned buffer takes the place of the workspace's K/V region; once it is
    // ready (kv_state 1) the stacked projection is skipped and enc is not read
    if (m->kv_keep ? (m->kv_state != 0 && m->kv_state != 1) || ((uintptr_t)m->kv_keep & 255) : m->kv_state != 0) return TDC_E_BADARG;
    const bool kv_ready = m->kv_keep && m->kv_state == 1;
    if (!enc && !kv_ready) return TDC_E_BADARG;
    // multi-prompt form (tdc_qformer_prompts): F virtual frames over U distinct ones
    const tdc_qformer_prompts* mp = m->prompts;
    if (mp && (mp->n_prompts <= 0 || mp->enc_frames <= 0 || !mp->kv_src || !mp->frame_prompt || !mp->prompt_len || !mp->self_len))
        return TDC_E_BADARG;
    const int U = mp ? mp->enc_frames : F;
    const QfWs w = qf_layout(m, F, K, Lt, Nenc);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return TDC_E_WORKSPACE;
    char* ws = (char*)workspace;
    const int D = m->dim, Dp = pad64i(D), dt = m->dtype, S = K + Lt, rows = F * S;
    const int hd = D / m->heads;
    float* h32 = (float*)(ws + w.h32);
    void* h16 = ws + w.h16;
    char* kv = m->kv_keep ? (char*)m->kv_keep : ws + w.kv;
    char* qkv = ws + w.qkv;
    void* ctx = ws + w.ctx;
    void* ctxq = ws + w.ctxq;
    void* cq = ws + w.cq;
    float* t32 = (float*)(ws + w.t32);
    float* t32b = (float*)(ws + w.t32b);
    void* mq = ws + w.mq;
    void* mt = ws + w.mt;
    const tdc_rowmap qmap = {K, S, 0, 1};
    const tdc_rowmap tmap = {Lt > 0 ? Lt : 1, S, K, 1};
    hipStream_t st = (hipStream_t)stream;
    // attention outputs only write the real columns: clear the K-padding columns once
    if (Dp != D) {
        if (hipMemsetAsync(ctx, 0, (size_t)rows * Dp * 2, st) != hipSuccess) return TDC_E_BADARG;
        if (hipMemsetAsync(ctxq, 0, (size_t)F * K * Dp * 2, st) != hipSuccess) return TDC_E_BADARG;
    }
    {
        tdc_qembed_desc e;
        memset(&e, 0, sizeof(e));
        e.query = query; e.ldq = ldq; e.qsrc = qsrc; e.word = m->word; e.pos = m->pos; e.ldw = m->ldw; e.ids = ids;
        e.Lt = Lt; e.gamma = m->emb_ln_g; e.beta = m->emb_ln_b; e.eps = m->eps; e.h32 = h32; e.h16 = h16; e.ld = Dp;
        e.F = F; e.K = K; e.cols = D; e.dtype = dt;
        if (mp) { e.frame_prompt = mp->frame_prompt; e.prompt_len = mp->prompt_len; e.ids_ld = Lt; }
        RET_IF(tdc_qformer_embed(&e, stream));
    }
    const int mode = qf_mode(m, K, Nenc);
    const bool fused = mode == 2;
    if (mp && fused) {
        fprintf(stderr, "[tdc_hip] tdc_qformer_fwd: the multi-prompt form runs xattn_mode 0 / 1 only\n");
        return TDC_E_BADARG;
    }
    if (m->kv_keep && fused) {
        fprintf(stderr, "[tdc_hip] tdc_qformer_fwd: kept K/V (kv_keep) runs xattn_mode 0 / 1 only\n");
        return TDC_E_BADARG;
    }
    {
    TdcProfTagGuard tag_kv(TDC_PROF_TAG_XATTN_BLOCK);   // the cross-attention block's launches, for tdc_profile_*
    if (fused) {
        // keys of all cross layers: one GEMM; values of all cross layers TRANSPOSED: one GEMM with the operands swapped
        // (A = Wv [n_cross*dim, H], "weight" = enc [F*Nenc, H]) - vt[c][f*Nenc + key], the A operand of the PV product
        RET_IF(Gemm(enc, ldenc, m->cross_k, kv, m->cross_k.n, F * Nenc, dt).run(stream));
        const tdc_lin enc_t = {enc, nullptr, F * Nenc, m->cross_v.k};
        RET_IF(Gemm(m->cross_v.w, m->cross_v.k, enc_t, ws + w.vt, (int)w.ldvt, m->cross_v.n, dt).ldw(ldenc).c_pad8().run(stream));
    } else if (!kv_ready) {
        RET_IF(Gemm(enc, ldenc, m->cross_kv, kv, m->cross_kv.n, U * Nenc, dt).run(stream));
    }
    }
    const float scale = (float)(1.0 / sqrt((double)hd));          // float(hd ** -0.5), correctly rounded (1.0f / sqrtf is 1 ulp off at 72, 96)
    for (int l = 0; l < m->n_layers; ++l) {
        const tdc_qformer_layer& L = m->layers_host[l];
        bool q16 = false;   // this layer's query rows between the cross-attention output and the FFN LayerNorm: 16-bit only (t32 holds 16-bit rows)
        RET_IF(Gemm(h16, Dp, L.qkv, qkv, L.qkv.n, rows, dt).run(stream));
        // multi-prompt: a frame's text rows end at K + its own prompt's length
        RET_IF(self_attention(qkv, L.qkv.n, ctx, Dp, F, S, m->heads, hd, D, scale, dt, stream, mp ? mp->self_len : nullptr));
        RET_IF(Gemm(ctx, Dp, L.attn_out, t32, Dp, rows, dt).out_f32().res(h32, Dp, 1).run(stream));
        RET_IF(Ln(t32, Dp, 1, L.attn_ln_g, L.attn_ln_b, m->eps, rows, D, dt).y16(h16, Dp).y32(h32, Dp).run(stream));
        {
        TdcProfTagGuard tag_x(L.has_cross ? TDC_PROF_TAG_XATTN_BLOCK : -1);
        if (L.has_cross && fused) {
            tdc_xattn_desc x;
            memset(&x, 0, sizeof(x));
            x.h16 = h16; x.h32 = h32; x.ldh = Dp; x.F = F; x.K = K; x.S = S;
            x.wq = L.cross_q_tiled; x.bq = L.cross_q.b; x.wo = L.cross_out_tiled; x.bo = L.cross_out.b;
            x.k = kv + (size_t)L.cross_idx * D * 2; x.ldk = m->cross_k.n;
            x.vt = ws + w.vt + (size_t)L.cross_idx * D * w.ldvt * 2; x.ldvt = (long long)w.ldvt;
            x.bv = m->cross_bv ? m->cross_bv + (size_t)L.cross_idx * D : nullptr;
            x.Nenc = Nenc; x.ln_g = L.cross_ln_g; x.ln_b = L.cross_ln_b; x.eps = m->eps;
            x.dim = D; x.heads = m->heads; x.scale = scale; x.dtype = dt;
            RET_IF(tdc_qformer_xattn(&x, stream));
        } else if (L.has_cross) {
            RET_IF(Gemm(h16, Dp, L.cross_q, cq, Dp, F * K, dt).a_map(qmap).run(stream));
            tdc_attn_desc c;
            memset(&c, 0, sizeof(c));
            const size_t koff = (size_t)L.cross_idx * 2 * D * 2;
            c.q = cq; c.k = kv + koff; c.v = kv + koff + (size_t)D * 2; c.o = ctxq;
            c.q_bs = (long long)K * Dp; c.k_bs = c.v_bs = (long long)Nenc * m->cross_kv.n; c.o_bs = (long long)K * Dp;
            c.q_rs = Dp; c.k_rs = c.v_rs = m->cross_kv.n; c.o_rs = Dp;
            c.batch = F; c.heads = m->heads; c.head_dim = hd; c.sq = K; c.sk = Nenc; c.scale = scale; c.dtype = dt;
            if (mp) c.kv_index = mp->kv_src;    // the K / V of the distinct frame this virtual frame stands for
            RET_IF(tdc_attention(&c, stream));
            if (mode == 1) {     // output projection + residual + LayerNorm of the K query rows in one kernel
                tdc_xattn_desc x;
                memset(&x, 0, sizeof(x));
                x.h16 = h16; x.h32 = h32; x.ldh = Dp; x.F = F; x.K = K; x.S = S;
                x.wo = L.cross_out_tiled; x.bo = L.cross_out.b; x.ln_g = L.cross_ln_g; x.ln_b = L.cross_ln_b; x.eps = m->eps;
                x.dim = D; x.heads = m->heads; x.Nenc = Nenc; x.dtype = dt; x.ctx = ctxq; x.ldctx = Dp;
                // the residual of this kernel and of the query FFN behind it is the 16-bit hidden state (tdc_xattn_desc.res16):
                // the fp32 copy of the query rows is not touched until the FFN's LayerNorm rewrites both copies
                x.res16 = 1; x.h32 = nullptr;
                q16 = true;
                RET_IF(tdc_qformer_xattn(&x, stream));
            } else {
                RET_IF(Gemm(ctxq, Dp, L.cross_out, t32, Dp, F * K, dt).out_f32().res(h32, Dp, 1).r_map(qmap).run(stream));
                RET_IF(Ln(t32, Dp, 1, L.cross_ln_g, L.cross_ln_b, m->eps, F * K, D, dt).y16(h16, Dp).y32(h32, Dp).y_map(qmap).run(stream));
            }
        }
        }
        RET_IF(Gemm(h16, Dp, L.fq1, mq, L.fq2.k, F * K, dt).act(TDC_ACT_GELU_ERF).a_map(qmap).run(stream));
        if (q16)
            RET_IF(Gemm(mq, L.fq2.k, L.fq2, t32, Dp, F * K, dt).res(h16, Dp, 0).r_map(qmap).run(stream));
        else
            RET_IF(Gemm(mq, L.fq2.k, L.fq2, t32, Dp, F * K, dt).out_f32().res(h32, Dp, 1).r_map(qmap).run(stream));
        if (Lt > 0) {
            RET_IF(Gemm(h16, Dp, L.ft1, mt, L.ft2.k, F * Lt, dt).act(TDC_ACT_GELU_ERF).a_map(tmap).run(stream));
            RET_IF(Gemm(mt, L.ft2.k, L.ft2, t32b, Dp, F * Lt, dt).out_f32().res(h32, Dp, 1).r_map(tmap).run(stream));
        }
        RET_IF(Ln(t32, Dp, q16 ? 0 : 1, L.fq_ln_g, L.fq_ln_b, m->eps, F * K, D, dt).y16(h16, Dp).y32(h32, Dp).y_map(qmap).run(stream));
        if (Lt > 0)
            RET_IF(Ln(t32b, Dp, 1, L.ft_ln_g, L.ft_ln_b, m->eps, F * Lt, D, dt).y16(h16, Dp).y32(h32, Dp).y_map(tmap).run(stream));
    }
    RET_IF(Gemm(h16, Dp, m->vision_proj, out, ldo, F * K, dt).a_map(qmap).run(stream));
    return tdc_l2_normalize(out, ldo, F * K, m->H, dt, stream);
}

// ---- ViT tower (a2-a4) ---------------------------------------------------------------------------------------------------
namespace {
// The residual stream x [rows, Dp] of a tower (the x32 region of the workspace): fp32 rows, or 16-bit rows of type `rt`
// (tdc_vit_model.res_dtype_p1) under GEMM operands of type `dt`.  Its operations are the ones VideoEncoder._tower_batch
// (pipeline.py) names - ln, update, the patch embedding, the final LayerNorm + resample - and everything in which the two streams
// differ is said here, once.
struct ResStream {
    void* x; bool f32; int rt;
    int rows, D, Dp, dt; float eps;      // shared by every launch: `rows` rows of D real columns (stride Dp), operands of type dt
    void* h16;                           // 16-bit operand rows: a LayerNorm's output (e4m3 bytes for ln8), the fp32 stream's row copy
    float* part;                         // the fold's per-slot (mean, M2) partials
    void* st;

    // a GEMM that writes rows of the stream: fp32 C, or 16-bit C of the stream's own type under operands of type dt
    Gemm into(const void* a, int lda, const tdc_lin& lin, int M) const {
        Gemm g(a, lda, lin, x, Dp, M, dt);
        if (f32) g.out_f32(); else g.c16(rt);
        return g;
    }
    // LayerNorm of the stream -> 16-bit operand rows in h16 (a 16-bit stream says its own type: it may differ from dt)
    int ln(const float* g, const float* b) const {
        Ln l(x, Dp, f32, g, b, eps, rows, D, dt);
        if (!f32) l.x_type(rt);
        return l.y16(h16, Dp).run(st);
    }
    // ... -> e4m3 rows in h16 (row stride ldy8 bytes) + per-row scales in `stats`, for an fp8-operand GEMM of weight scale `wscale`.
    // tdc_ln_desc.x_dtype_p1 excludes the e4m3 output; this form writes no 16-bit value, so `dtype` itself names the type of a
    // 16-bit stream's rows
    int ln8(const float* g, const float* b, int ldy8, float* stats, float wscale) const {
        return Ln(x, Dp, f32, g, b, eps, rows, D, f32 ? dt : rt).y8(h16, ldy8, stats, wscale).run(st);
    }
    // x <- x + a lin^T + b in place: the fp32 stream is read-modify-written (8 B per element), the 16-bit one rounds
    // acc + bias + float(x) once.  emit (LayerNorm fold): the epilogue also leaves the per-slot partials of the updated rows and - fp32
    // stream only - their 16-bit copy in h16 for the folded consumers; over a 16-bit stream those read the stream itself (fold_src)
    int update(const void* a, int lda, const tdc_lin& lin, bool emit = false) const {
        Gemm g = into(a, lda, lin, rows);
        g.res(x, Dp, f32);
        if (emit) g.emit(f32 ? h16 : nullptr, f32 ? Dp : 0, part);
        return g.run(st);
    }
    // ... on e4m3 operands a8 / lin.w with the dequantisation scales in `stats`.  tdc_gemm_desc.c16_dtype_p1 excludes fp8 operands;
    // with in_fp8 `dtype` types C / res only, so it names the type of a 16-bit stream
    int update8(const void* a8, int lda, const tdc_lin& lin, const float* stats, const float* zeros) const {
        Gemm g(a8, lda, lin, x, Dp, rows, f32 ? dt : rt);
        if (f32) g.out_f32();
        return g.res(x, Dp, f32).in_fp8().fold(stats, zeros).run(st);
    }
    // A operand of the folded consumers (qkv of the layers with qkv_c1, every fc1): the RAW rows - the fp32 stream's 16-bit copy, the
    // 16-bit stream itself (of the operands' type then, whole 64-column slots)
    const void* fold_src() const { return f32 ? h16 : x; }
    // patch embedding: GEMM over the im2col rows, position rows added in the epilogue, output rows skip the cls slot; then the cls row
    int embed(const tdc_vit_model* m, const void* patches, int B, int P, int S) const {
        const tdc_rowmap cmap = {P, S, m->has_cls, 1}, rmap = {P, 0, m->has_cls, 1};
        RET_IF(into(patches, m->patch_lin.k, m->patch_lin, B * P).res(m->pos, m->ldpos, 1).c_map(cmap).r_map(rmap).run(st));
        if (!m->has_cls) return 0;
        return f32 ? tdc_set_rows((float*)x, Dp, B, S, 0, m->cls_row, st) : tdc_set_rows16(x, Dp, B, S, 0, m->cls_row, rt, st);
    }
    // optional final LayerNorm, then the bilinear resample of the g x g token grid (cls dropped) into `out`
    int finish(const tdc_vit_model* m, int B, int g, void* out, int ldo, int out_grid, const int* idx0, const int* idx1,
               const float* frac, int out_dt) const {
        if (!m->lnf_g)
            return tdc_resample_tokens(x, f32, Dp, m->has_cls, g, out, ldo, out_grid, idx0, idx1, frac, B, D, f32 ? dt : rt, out_dt, st);
        RET_IF(ln(m->lnf_g, m->lnf_b));
        return tdc_resample_tokens(h16, 0, Dp, m->has_cls, g, out, ldo, out_grid, idx0, idx1, frac, B, D, dt, out_dt, st);
    }
};
}  // namespace

extern "C" size_t tdc_vit_workspace_bytes(const tdc_vit_model* m, int B, int H, int W) {
    if (!m || B <= 0 || !m->layers_host) return 0;
    return vit_layout(m, B, H, W).total;
}

extern "C" int tdc_vit_fwd(const tdc_vit_model* m, const void* px, int px_f32, int B, int H, int W, int out_grid,
                           const int* idx0, const int* idx1, const float* frac, void* out, int ldo, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!m || !px || !out || !workspace || B <= 0 || H != W || H < m->patch) return TDC_E_BADARG;  // "valid" conv: H % patch pixels dropped
    const VitWs w = vit_layout(m, B, H, W);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return TDC_E_WORKSPACE;
    char* ws = (char*)workspace;
    const int g = H / m->patch, P = g * g, S = P + m->has_cls, rows = B * S;
    const int D = m->dim, Dp = pad64i(D), dt = m->dtype;
    const int out_dt = m->out_dtype_p1 ? m->out_dtype_p1 - 1 : dt;
    void* patches = ws + w.patches;
    void* h16 = ws + w.h16;
    char* qkv = ws + w.qkv;
    void* attn = ws + w.attn;
    void* mlp = ws + w.mlp;
    float* stats = (float*)(ws + w.stats);                      // (mean, rstd) of the fold / the e4m3 rows' scales
    float* stats2 = stats + al256((size_t)rows * 8) / 4;        // fp8 level 3: fc1's out_stats
    const ResStream x = {ws + w.x32, !m->res_dtype_p1, m->res_dtype_p1 - 1, rows, D, Dp, dt, m->eps, h16, (float*)(ws + w.part), stream};
    // fused: the block's LayerNorms are folded into the GEMMs around them (tdc_gemm_desc: x16 / ln_part / ln_stats / ln_c1): no
    // LayerNorm kernel behind layer 0's first.  fp8: the LayerNorms emit e4m3 rows + scales, qkv / fc1 (level 2: out / fc2 too) run on them
    const bool fused = m->fused != 0;
    const int fp8 = m->fp8;
    // every refusal comes before the first launch
    if (!x.f32 && x.rt != TDC_F16 && x.rt != TDC_BF16) return TDC_E_BADARG;
    if (out_dt != TDC_F16 && out_dt != TDC_BF16) return TDC_E_BADARG;
    if (fp8 && (fused || D % 128 != 0)) return TDC_E_BADARG;
    if (fused && (D % 64 != 0 || (!x.f32 && x.rt != dt))) return TDC_E_BADARG;     // see ResStream::fold_src
    RET_IF(tdc_im2col(px, px_f32, patches, m->patch_lin.k, B, H, W, m->patch, dt, stream));
    // the attention writes the real columns only: its output's pad columns (K padding of the out-projection) are cleared once.  The
    // clear and the patch embedding touch different buffers; each stream keeps the order it has always enqueued them in
    const auto clear_attn_pad = [&]() { return Dp != D ? (int)hipMemsetAsync(attn, 0, (size_t)rows * Dp * 2, (hipStream_t)stream) : 0; };
    if (!x.f32) RET_IF(clear_attn_pad());
    RET_IF(x.embed(m, patches, B, P, S));
    if (x.f32) RET_IF(clear_attn_pad());
    const float scale = (float)(1.0 / sqrt((double)m->head_dim));  // float(head_dim ** -0.5), correctly rounded (1.0f / sqrtf is 1 ulp off at 72)
    const int slots = D / 64;
    // the loop body reads side by side with VideoEncoder._tower_batch (pipeline.py)
    for (int l = 0; l < m->n_layers; ++l) {
        const tdc_vit_layer& L = m->layers_host[l];
        if (fp8) {
            RET_IF(x.ln8(L.ln1_g, L.ln1_b, L.qkv.k, stats, L.qkv_wscale));
            RET_IF(Gemm(h16, L.qkv.k, L.qkv, qkv, L.qkv.n, rows, dt).in_fp8().fold(stats, L.zeros).run(stream));
        } else if (!fused || !L.qkv_c1) {       // layer 0 of a fused tower: its input comes from the patch embedding, no statistics yet
            RET_IF(x.ln(L.ln1_g, L.ln1_b));
            RET_IF(Gemm(h16, Dp, L.qkv, qkv, L.qkv.n, rows, dt).run(stream));
        } else {
            RET_IF(Gemm(x.fold_src(), Dp, L.qkv, qkv, L.qkv.n, rows, dt).fold(stats, L.qkv_c1).run(stream));
        }
        RET_IF(self_attention(qkv, L.qkv.n, attn, Dp, B, S, m->heads, m->head_dim, D, scale, dt, stream));
        if (fp8 >= 2) {     // attention output -> e4m3 rows (in h16: the LayerNorm rows are consumed) -> out-projection on fp8
            RET_IF(tdc_quantize_rows_fp8(attn, Dp, rows, Dp, dt, h16, L.out.k, stats, L.out_wscale, stream));
            RET_IF(x.update8(h16, L.out.k, L.out, stats, L.zeros));
        } else {
            RET_IF(x.update(attn, Dp, L.out, fused));
        }
        // fc1's output: the fp8 forms write it at the row stride the workspace was laid out with (fc1's width when that exceeds
        // fc2.k), the others - and every 16-bit-operand fc2, level 1's included - at fc2.k; one number for every real model
        const int mlp_ld = fp8 ? vit_mlp_ld(m) : L.fc2.k;
        const int mlp_n = m->act == TDC_ACT_SWIGLU ? L.fc1.n / 2 : L.fc1.n;     // columns fc1 writes (pad columns: 0)
        if (fused) {
            RET_IF(tdc_ln_finalize(x.part, slots, rows, m->eps, stats, stream));
            RET_IF(Gemm(x.fold_src(), Dp, L.fc1, mlp, mlp_ld, rows, dt).act(m->act).fold(stats, L.fc1_c1).run(stream));
        } else if (fp8) {
            RET_IF(x.ln8(L.ln2_g, L.ln2_b, L.fc1.k, stats, L.fc1_wscale));
            if (fp8 >= 3) {     // fc1 writes the e4m3 MLP hidden + its row scales itself (qkv buffer, second stats array)
                if (mlp_n != L.fc2.k) return TDC_E_BADARG;
                RET_IF(Gemm(h16, L.fc1.k, L.fc1, qkv, L.fc2.k, rows, dt).act(m->act).in_fp8().fold(stats, L.zeros)
                           .out_fp8(stats2, L.fc1_w2max, L.fc1_bmax, L.fc2_wscale).run(stream));
            } else {
                RET_IF(Gemm(h16, L.fc1.k, L.fc1, mlp, mlp_ld, rows, dt).act(m->act).in_fp8().fold(stats, L.zeros).run(stream));
            }
        } else {
            RET_IF(x.ln(L.ln2_g, L.ln2_b));
            RET_IF(Gemm(h16, Dp, L.fc1, mlp, mlp_ld, rows, dt).act(m->act).run(stream));
        }
        if (fp8 >= 3) {
            RET_IF(x.update8(qkv, L.fc2.k, L.fc2, stats2, L.zeros));
        } else if (fp8 == 2) {      // MLP hidden -> e4m3 rows (in the qkv buffer, free after the attention) -> fc2 on fp8
            RET_IF(tdc_quantize_rows_fp8(mlp, mlp_ld, rows, mlp_n, dt, qkv, L.fc2.k, stats, L.fc2_wscale, stream));
            RET_IF(x.update8(qkv, L.fc2.k, L.fc2, stats, L.zeros));
        } else if (fused && l + 1 < m->n_layers) {
            RET_IF(x.update(mlp, L.fc2.k, L.fc2, true));
            RET_IF(tdc_ln_finalize(x.part, slots, rows, m->eps, stats, stream));
        } else {                    // the last layer's statistics would have no consumer
            RET_IF(x.update(mlp, L.fc2.k, L.fc2));
        }
    }
    return x.finish(m, B, g, out, ldo, out_grid, idx0, idx1, frac, out_dt);
}

// ---- connector (a6-a9) -------------------------------------------------------------------------------------------------
namespace {
struct ConnWs {
    size_t h, y32, aux[2], ctx, cproj, cin, q16[2], qin, xn, kv[2], qn, qs, att, q2, mh, total;
};

ConnWs conn_layout(const tdc_connector_model* m, int T) {
    const size_t Cp = pad64i(m->C), P = (size_t)(m->side * m->r) * (m->side * m->r), nq = (size_t)m->side * m->side;
    const size_t rows = (size_t)T * P, qrows = (size_t)T * nq, Hp = m->mm1.n;
    ConnWs w;
    size_t off = 0;
    w.h = off;       off += al256(rows * Cp * 2);             // aux fc1 output
    w.y32 = off;     off += al256(rows * Cp * 4);             // aux fc2 output (fp32, LayerNorm input)
    for (int i = 0; i < 2; ++i) { w.aux[i] = off; off += al256(rows * Cp * 2); }
    w.ctx = off;     off += al256((size_t)T * Cp * 2);
    w.cproj = off;   off += al256((size_t)T * Cp * 2);
    w.cin = off;     off += al256((size_t)T * Cp * 4);
    for (int i = 0; i < 2; ++i) { w.q16[i] = off; off += al256(qrows * Cp * 2); }
    w.qin = off;     off += al256(qrows * Cp * 4);
    w.xn = off;      off += al256(rows * Cp * 2);
    for (int i = 0; i < 2; ++i) { w.kv[i] = off; off += al256(rows * 2 * Cp * 2); }
    w.qn = off;      off += al256(qrows * Cp * 2);
    w.qs = off;      off += al256(qrows * Cp * 2);
    w.att = off;     off += al256(qrows * Cp * 2);
    w.q2 = off;      off += al256(qrows * Cp * 4);
    w.mh = off;      off += al256(qrows * (Hp > Cp ? Hp : Cp) * 2);   // proj_out hidden / mm_projector hidden
    w.total = off;
    return w;
}

}  // namespace

extern "C" size_t tdc_connector_workspace_bytes(const tdc_connector_model* m, int T) {
    if (!m || T <= 0 || !m->layers_host) return 0;
    return conn_layout(m, T).total;
}

extern "C" int tdc_connector_fwd(const tdc_connector_model* m, const void* sig, int ld_s, const void* dino, int ld_d,
                                 int T, const unsigned char* mask, void* out, int ldo, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!m || !sig || !dino || !mask || !out || !workspace || T <= 0 || m->n_layers <= 0) return TDC_E_BADARG;
    const ConnWs w = conn_layout(m, T);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return TDC_E_WORKSPACE;
    char* ws = (char*)workspace;
    // kept aux rows (tdc_connector_model.aux_keep / ctx_keep): all three or none; caller-owned buffers take the place of the
    // workspace's aux / ctx regions for the launches that write them and for every later reader
    const int n_keep = (m->aux_keep[0] != nullptr) + (m->aux_keep[1] != nullptr) + (m->ctx_keep != nullptr);
    if (n_keep != 0 && n_keep != 3) return TDC_E_BADARG;
    if (n_keep && (((uintptr_t)m->aux_keep[0] | (uintptr_t)m->aux_keep[1] | (uintptr_t)m->ctx_keep) & 255)) return TDC_E_BADARG;
    char* const aux[2] = {n_keep ? (char*)m->aux_keep[0] : ws + w.aux[0], n_keep ? (char*)m->aux_keep[1] : ws + w.aux[1]};
    char* const ctx = n_keep ? (char*)m->ctx_keep : ws + w.ctx;
    const int C = m->C, Cp = pad64i(C), dt = m->dtype, side = m->side, r = m->r;
    const int P = side * r * side * r, nq = side * side, rows = T * P, qrows = T * nq;
    const float eps = 1e-5f;
    hipStream_t st = (hipStream_t)stream;
    // a6: mm_projector_aux_i = Linear + GELU(erf), Linear, LayerNorm(1e-5); global context = mean over the tokens of aux_0
    const void* feats[2] = {sig, dino};
    const int lds[2] = {ld_s, ld_d};
    for (int i = 0; i < 2; ++i) {
        const tdc_aux_proj& a = m->aux[i];
        RET_IF(Gemm(feats[i], lds[i], a.fc1, ws + w.h, Cp, rows, dt).act(TDC_ACT_GELU_ERF).run(stream));
        RET_IF(Gemm(ws + w.h, Cp, a.fc2, ws + w.y32, Cp, rows, dt).out_f32().run(stream));
        RET_IF(Ln(ws + w.y32, Cp, 1, a.ln_g, a.ln_b, eps, rows, C, dt).y16(aux[i], Cp).run(stream));
    }
    RET_IF(tdc_token_mean(aux[0], P, Cp, ctx, T, dt, stream));
    // queries start as vision_query broadcast to every window of every frame (cambrian_arch.py:1018-1023)
    RET_IF(tdc_fill_rows(m->vision_query, ws + w.q16[0], Cp, qrows, stream));
    int cur = 0;
    for (int l = 0; l < m->n_layers; ++l) {
        const tdc_sva_layer& L = m->layers_host[l];
        char* q16 = ws + w.q16[cur];
        char* q16n = ws + w.q16[cur ^ 1];
        RET_IF(Gemm(ctx, Cp, L.proj_context, ws + w.cproj, Cp, T, dt).run(stream));
        RET_IF(Gemm(ws + w.cproj, Cp, L.proj_in_c, ws + w.cin, Cp, T, dt).out_f32().run(stream));
        {   // proj_in(cat[q, ctx]) = proj_in_q(q) + (per-frame) proj_in_c(ctx)
            const tdc_rowmap rmap = {nq, 1, 0, 0};
            RET_IF(Gemm(q16, Cp, L.proj_in_q, ws + w.qin, Cp, qrows, dt).out_f32().res(ws + w.cin, Cp, 1).r_map(rmap).run(stream));
        }
        for (int tw = 0; tw < 2; ++tw) {    // un-affine LayerNorm of the tower's tokens + window position (the affines live in kv[tw])
            RET_IF(Ln(aux[tw], Cp, 0, m->ones_C, m->zeros_C, eps, rows, C, dt).y16(ws + w.xn, Cp)
                       .add(L.pos[tw], L.ldpos, P, 1).run(stream));
            RET_IF(Gemm(ws + w.xn, Cp, L.kv[tw], ws + w.kv[tw], L.kv[tw].n, rows, dt).run(stream));
        }
        RET_IF(Ln(ws + w.qin, Cp, 1, L.q_ln_g, L.q_ln_b, eps, qrows, C, dt).y16(ws + w.qn, Cp).run(stream));
        RET_IF(Gemm(ws + w.qn, Cp, L.q_proj, ws + w.qs, Cp, qrows, dt).run(stream));
        {
            tdc_sva_attn_desc a;
            memset(&a, 0, sizeof(a));
            a.q = ws + w.qs; a.ldq = Cp; a.kv[0] = ws + w.kv[0]; a.kv[1] = ws + w.kv[1]; a.ldkv = L.kv[0].n;
            a.mask = mask; a.out = ws + w.att; a.ldo = Cp;
            a.T = T; a.side = side; a.r = r; a.n_towers = 2; a.dim = C; a.heads = m->heads; a.dtype = dt;
            if (Cp != C && hipMemsetAsync(ws + w.att, 0, (size_t)qrows * Cp * 2, st) != hipSuccess) return TDC_E_BADARG;
            RET_IF(tdc_sva_attention(&a, stream));
        }
        RET_IF(Gemm(ws + w.att, Cp, L.o_proj, ws + w.q2, Cp, qrows, dt).out_f32().res(ws + w.qin, Cp, 1).run(stream));
        RET_IF(Ln(ws + w.q2, Cp, 1, L.norm_g, L.norm_b, eps, qrows, C, dt).y16(ws + w.qn, Cp).run(stream));
        RET_IF(Gemm(ws + w.qn, Cp, L.out1, ws + w.mh, Cp, qrows, dt).act(TDC_ACT_GELU_ERF).run(stream));
        RET_IF(Gemm(ws + w.mh, Cp, L.out2, q16n, Cp, qrows, dt).res(q16, Cp, 0).run(stream));
        cur ^= 1;
    }
    // a9: mm_projector
    RET_IF(Gemm(ws + w.q16[cur], Cp, m->mm1, ws + w.mh, m->mm1.n, qrows, dt).act(TDC_ACT_GELU_ERF).run(stream));
    return Gemm(ws + w.mh, m->mm1.n, m->mm2, out, ldo, qrows, dt).run(stream);
}
