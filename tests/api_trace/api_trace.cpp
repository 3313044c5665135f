// CPU launch trace of the three composites of csrc/api.cpp (tdc_vit_fwd, tdc_qformer_fwd, tdc_connector_fwd).
//
// api.cpp holds no kernel: it compiles with a plain host compiler and calls the library's leaf entry points.  This program
// links api.o alone, defines every one of those entry points (and hipMemsetAsync) as a stub that prints one line per call -
// the function's name and every non-zero field of its descriptor / argument list -, and runs the composites over a matrix of
// tiny models.  Nothing touches a GPU and no model pointer is dereferenced: the workspace and the weights are fake
// addresses that print as `ws+0x..` / `<name>+0x..`, so the output is deterministic.  tests/test_api_trace.py compares it
// byte for byte with tests/golden/api_trace.txt (written by tests/golden/make_api_trace.py): a reorganisation of api.cpp
// that changes a launch, an operand or the order shows up as a diff of that file.
#include "../../include/tdc_hip.h"
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

namespace {

// ---- fake addresses ------------------------------------------------------------------------------------------------------
const uintptr_t WS = 0x700000000000ull;        // the workspace (256-aligned); everything up to WS_SPAN behind it prints as ws+off
const uintptr_t WS_SPAN = 1ull << 36;
const uintptr_t TAG0 = 0x100000000000ull;      // model pointers: one 256-MiB slot per name, so name+offset stays recognisable
const int TAG_SHIFT = 28;
void* const STREAM = (void*)0x5717ull;
std::vector<std::string> g_tags;

void* tag(const std::string& name) {
    g_tags.push_back(name);
    return (void*)(TAG0 + ((uintptr_t)(g_tags.size() - 1) << TAG_SHIFT));
}
const float* ftag(const std::string& name) { return (const float*)tag(name); }
const int* itag(const std::string& name) { return (const int*)tag(name); }

// ---- printing --------------------------------------------------------------------------------------------------------------
void P(const char* n, const void* p) {
    const uintptr_t a = (uintptr_t)p;
    if (!a) return;
    if (a >= WS && a < WS + WS_SPAN) { printf(" %s=ws+0x%zx", n, (size_t)(a - WS)); return; }
    const uintptr_t i = (a - TAG0) >> TAG_SHIFT, off = (a - TAG0) & (((uintptr_t)1 << TAG_SHIFT) - 1);
    if (a >= TAG0 && i < g_tags.size()) {
        if (off) printf(" %s=%s+0x%zx", n, g_tags[i].c_str(), (size_t)off);
        else printf(" %s=%s", n, g_tags[i].c_str());
        return;
    }
    printf(" %s=0x%zx", n, (size_t)a);
}
void I(const char* n, long long v) { if (v) printf(" %s=%lld", n, v); }
void F(const char* n, double v) { if (v != 0.0) printf(" %s=%.9g", n, v); }
void M(const char* n, const tdc_rowmap& m) {
    if (m.seg || m.stride || m.off || m.inner) printf(" %s={%d,%d,%d,%d}", n, m.seg, m.stride, m.off, m.inner);
}
void S(void* stream) { if (stream != STREAM) printf(" stream=UNEXPECTED"); }
void begin(const char* fn) { printf("%s", fn); }
int end(void* stream) { S(stream); printf("\n"); return 0; }

int g_xattn_ok = 0;      // what tdc_qformer_xattn_supported answers in the current case
int g_prof_tag = 0;

}  // namespace

// ---- the recording stubs -----------------------------------------------------------------------------------------------------
extern "C" {

hipError_t hipMemsetAsync(void* dst, int value, size_t sizeBytes, hipStream_t stream) {
    begin("hipMemsetAsync"); P("dst", dst); I("value", value); I("sizeBytes", (long long)sizeBytes);
    end((void*)stream);
    return hipSuccess;
}

int tdc_gemm(const tdc_gemm_desc* d, void* stream) {
    begin("tdc_gemm");
    P("A", d->A); I("lda", d->lda); P("W", d->W); I("ldw", d->ldw); P("C", d->C); I("ldc", d->ldc); P("bias", d->bias);
    P("res", d->res); I("ldres", d->ldres); I("M", d->M); I("N", d->N); I("K", d->K);
    I("dtype", d->dtype); I("out_f32", d->out_f32); I("res_f32", d->res_f32); I("act", d->act);
    M("a_map", d->a_map); M("c_map", d->c_map); M("r_map", d->r_map);
    P("x16", d->x16); I("ldx16", d->ldx16); P("ln_part", d->ln_part); P("ln_stats", d->ln_stats); P("ln_c1", d->ln_c1);
    I("in_fp8", d->in_fp8); I("out_fp8", d->out_fp8); P("out_stats", d->out_stats); F("out_w2max", d->out_w2max);
    F("out_bmax", d->out_bmax); F("out_wscale", d->out_wscale); I("c_pad8", d->c_pad8); I("c16_dtype_p1", d->c16_dtype_p1);
    return end(stream);
}

int tdc_layernorm(const tdc_ln_desc* d, void* stream) {
    begin("tdc_layernorm");
    P("x", d->x); I("ldx", d->ldx); I("x_f32", d->x_f32); P("y16", d->y16); I("ldy16", d->ldy16); P("y32", d->y32);
    I("ldy32", d->ldy32); P("gamma", d->gamma); P("beta", d->beta); F("eps", d->eps);
    P("add", d->add); I("ldadd", d->ldadd); I("add_period", d->add_period); I("add_mode", d->add_mode);
    I("rows", d->rows); I("cols", d->cols); I("dtype", d->dtype); M("x_map", d->x_map); M("y_map", d->y_map);
    P("y8", d->y8); I("ldy8", d->ldy8); P("y8_stats", d->y8_stats); F("y8_wscale", d->y8_wscale); I("x_dtype_p1", d->x_dtype_p1);
    return end(stream);
}

int tdc_attention(const tdc_attn_desc* d, void* stream) {
    begin("tdc_attention");
    P("q", d->q); P("k", d->k); P("v", d->v); P("o", d->o);
    I("q_bs", d->q_bs); I("k_bs", d->k_bs); I("v_bs", d->v_bs); I("o_bs", d->o_bs);
    I("q_rs", d->q_rs); I("k_rs", d->k_rs); I("v_rs", d->v_rs); I("o_rs", d->o_rs);
    I("batch", d->batch); I("heads", d->heads); I("head_dim", d->head_dim); I("sq", d->sq); I("sk", d->sk);
    F("scale", d->scale); I("dtype", d->dtype);
    P("bias", d->bias); I("bias_hs", d->bias_hs); I("bias_rs", d->bias_rs); P("gate", d->gate); I("gate_rs", d->gate_rs);
    P("key_mask", d->key_mask); I("key_mask_bs", d->key_mask_bs); I("form", d->form);
    P("k_len", d->k_len); P("kv_index", d->kv_index);
    return end(stream);
}

int tdc_sva_attention(const tdc_sva_attn_desc* d, void* stream) {
    begin("tdc_sva_attention");
    P("q", d->q); I("ldq", d->ldq); P("kv0", d->kv[0]); P("kv1", d->kv[1]); I("ldkv", d->ldkv); P("mask", d->mask);
    P("out", d->out); I("ldo", d->ldo); I("T", d->T); I("side", d->side); I("r", d->r); I("n_towers", d->n_towers);
    I("dim", d->dim); I("heads", d->heads); I("dtype", d->dtype);
    return end(stream);
}

int tdc_qformer_embed(const tdc_qembed_desc* d, void* stream) {
    begin("tdc_qformer_embed");
    P("query", d->query); I("ldq", d->ldq); P("qsrc", d->qsrc); P("word", d->word); P("pos", d->pos); I("ldw", d->ldw);
    P("ids", d->ids); I("Lt", d->Lt); P("gamma", d->gamma); P("beta", d->beta); F("eps", d->eps);
    P("h32", d->h32); P("h16", d->h16); I("ld", d->ld); I("F", d->F); I("K", d->K); I("cols", d->cols); I("dtype", d->dtype);
    P("frame_prompt", d->frame_prompt); P("prompt_len", d->prompt_len); I("ids_ld", d->ids_ld);
    return end(stream);
}

int tdc_qformer_xattn(const tdc_xattn_desc* d, void* stream) {
    begin("tdc_qformer_xattn");
    P("h16", d->h16); P("h32", d->h32); I("ldh", d->ldh); I("F", d->F); I("K", d->K); I("S", d->S);
    P("wq", d->wq); P("bq", d->bq); P("wo", d->wo); P("bo", d->bo); P("k", d->k); I("ldk", d->ldk);
    P("vt", d->vt); I("ldvt", d->ldvt); P("bv", d->bv); I("Nenc", d->Nenc); P("ln_g", d->ln_g); P("ln_b", d->ln_b);
    F("eps", d->eps); I("dim", d->dim); I("heads", d->heads); F("scale", d->scale); I("dtype", d->dtype);
    P("ctx", d->ctx); I("ldctx", d->ldctx); I("res16", d->res16);
    return end(stream);
}

int tdc_qformer_xattn_supported(int dim, int heads, int K, int Nenc) {
    begin("tdc_qformer_xattn_supported"); I("dim", dim); I("heads", heads); I("K", K); I("Nenc", Nenc);
    printf(" -> %d\n", g_xattn_ok);
    return g_xattn_ok;
}

int tdc_profile_tag(int tag) {
    const int prev = g_prof_tag;
    g_prof_tag = tag;
    printf("tdc_profile_tag tag=%d prev=%d\n", tag, prev);
    return prev;
}

int tdc_quantize_rows_fp8(const void* x, int ldx, int rows, int cols, int dtype, void* y8, int ldy8, float* stats,
                          float wscale, void* stream) {
    begin("tdc_quantize_rows_fp8"); P("x", x); I("ldx", ldx); I("rows", rows); I("cols", cols); I("dtype", dtype);
    P("y8", y8); I("ldy8", ldy8); P("stats", stats); F("wscale", wscale);
    return end(stream);
}

int tdc_ln_finalize(const float* ln_part, int slots, int rows, float eps, float* stats, void* stream) {
    begin("tdc_ln_finalize"); P("ln_part", ln_part); I("slots", slots); I("rows", rows); F("eps", eps); P("stats", stats);
    return end(stream);
}

int tdc_im2col(const void* px, int px_f32, void* patches, int ldp, int B, int H, int W, int patch, int dtype, void* stream) {
    begin("tdc_im2col"); P("px", px); I("px_f32", px_f32); P("patches", patches); I("ldp", ldp); I("B", B); I("H", H);
    I("W", W); I("patch", patch); I("dtype", dtype);
    return end(stream);
}

int tdc_set_rows(float* x32, int ld, int B, int S_, int row, const float* vec, void* stream) {
    begin("tdc_set_rows"); P("x32", x32); I("ld", ld); I("B", B); I("S", S_); I("row", row); P("vec", vec);
    return end(stream);
}

int tdc_set_rows16(void* x16, int ld, int B, int S_, int row, const float* vec, int dtype, void* stream) {
    begin("tdc_set_rows16"); P("x16", x16); I("ld", ld); I("B", B); I("S", S_); I("row", row); P("vec", vec); I("dtype", dtype);
    return end(stream);
}

int tdc_resample_tokens(const void* x, int x_f32, int ldx, int tok_off, int n_in, void* y, int ldy, int n_out,
                        const int* idx0, const int* idx1, const float* frac, int B, int cols, int dtype, int out_dtype,
                        void* stream) {
    begin("tdc_resample_tokens"); P("x", x); I("x_f32", x_f32); I("ldx", ldx); I("tok_off", tok_off); I("n_in", n_in);
    P("y", y); I("ldy", ldy); I("n_out", n_out); P("idx0", idx0); P("idx1", idx1); P("frac", frac); I("B", B);
    I("cols", cols); I("dtype", dtype); I("out_dtype", out_dtype);
    return end(stream);
}

int tdc_token_mean(const void* x, int P_, int ld, void* y, int B, int dtype, void* stream) {
    begin("tdc_token_mean"); P("x", x); I("P", P_); I("ld", ld); P("y", y); I("B", B); I("dtype", dtype);
    return end(stream);
}

int tdc_fill_rows(const void* row, void* out, int ld, int rows, void* stream) {
    begin("tdc_fill_rows"); P("row", row); P("out", out); I("ld", ld); I("rows", rows);
    return end(stream);
}

int tdc_l2_normalize(void* x, int ld, int rows, int cols, int dtype, void* stream) {
    begin("tdc_l2_normalize"); P("x", x); I("ld", ld); I("rows", rows); I("cols", cols); I("dtype", dtype);
    return end(stream);
}

}  // extern "C"

namespace {

int pad64(int x) { return (x + 63) / 64 * 64; }

tdc_lin lin(const std::string& name, int n, int k) {
    tdc_lin l;
    l.w = tag(name + ".w"); l.b = ftag(name + ".b"); l.n = n; l.k = k;
    return l;
}

void open_case(const std::string& name) {
    g_tags.clear();
    g_prof_tag = 0;
    g_xattn_ok = 0;
    printf("== %s\n", name.c_str());
}

void close_case(int rc, size_t bytes) { printf("-> rc=%d workspace_bytes=%zu\n", rc, bytes); }

// ---- tdc_vit_fwd ------------------------------------------------------------------------------------------------------------
enum Stream { S32, S16_SAME, S16_MIXED };      // fp32 stream; 16-bit stream of the operand type; bf16 operands over an fp16 stream
const char* const STREAM_NAME[] = {"fp32", "res16", "bf16_over_fp16"};

struct VitCase {
    int stream = S32, fused = 0, fp8 = 0, D = 128;
    bool cls = true;             // true: cls row, GELU(erf), final LayerNorm, out_dtype_p1 set; false: none of them, SwiGLU
    int fc1_n = 0;               // 0: fc1's (halved) output width == fc2.k; else fc1.n as given
    int res_dtype_p1 = -1;       // -1: from `stream`
    int H = 4, W = 4;
    long ws_short = 0, ws_skew = 0;
};

void run_vit(const std::string& name, const VitCase& c) {
    open_case(name);
    const int D = c.D, Dp = pad64(D), patch = 2, hidden = 256;
    tdc_vit_layer layers[2];
    memset(layers, 0, sizeof(layers));
    for (int l = 0; l < 2; ++l) {
        const std::string p = "L" + std::to_string(l) + ".";
        tdc_vit_layer& L = layers[l];
        L.ln1_g = ftag(p + "ln1_g"); L.ln1_b = ftag(p + "ln1_b"); L.ln2_g = ftag(p + "ln2_g"); L.ln2_b = ftag(p + "ln2_b");
        L.qkv = lin(p + "qkv", 3 * D, Dp);
        L.out = lin(p + "out", Dp, Dp);
        L.fc1 = lin(p + "fc1", c.fc1_n ? c.fc1_n : (c.cls ? hidden : 2 * hidden), Dp);
        L.fc2 = lin(p + "fc2", Dp, hidden);
        L.qkv_c1 = l ? ftag(p + "qkv_c1") : nullptr;      // layer 0's LayerNorm 1 runs as a kernel
        L.fc1_c1 = ftag(p + "fc1_c1");
        L.zeros = ftag(p + "zeros");
        L.qkv_wscale = 0.5f + l; L.fc1_wscale = 0.25f + l; L.out_wscale = 0.125f + l; L.fc2_wscale = 0.0625f + l;
        L.fc1_w2max = 3.0f + l; L.fc1_bmax = 7.0f + l;
    }
    tdc_vit_model m;
    memset(&m, 0, sizeof(m));
    m.dtype = c.stream == S16_MIXED ? TDC_BF16 : TDC_F16;
    m.dim = D; m.heads = 2; m.head_dim = D / 2; m.n_layers = 2; m.patch = patch; m.has_cls = c.cls;
    m.act = c.cls ? TDC_ACT_GELU_ERF : TDC_ACT_SWIGLU;
    m.eps = 1e-6f;
    m.patch_lin = lin("patch", Dp, pad64(3 * patch * patch));
    m.pos = ftag("pos"); m.ldpos = Dp;
    if (c.cls) { m.cls_row = ftag("cls_row"); m.lnf_g = ftag("lnf_g"); m.lnf_b = ftag("lnf_b"); }
    m.layers_host = layers;
    m.fused = c.fused; m.fp8 = c.fp8;
    m.out_dtype_p1 = c.cls ? TDC_BF16 + 1 : 0;
    m.res_dtype_p1 = c.res_dtype_p1 >= 0 ? c.res_dtype_p1 : c.stream == S32 ? 0 : c.stream == S16_SAME ? m.dtype + 1 : TDC_F16 + 1;
    const int B = 2;
    const size_t bytes = tdc_vit_workspace_bytes(&m, B, c.H, c.W);
    const int rc = tdc_vit_fwd(&m, tag("px"), 1, B, c.H, c.W, 3, itag("idx0"), itag("idx1"), ftag("frac"), tag("out"), Dp,
                               (void*)(WS + c.ws_skew), bytes - c.ws_short, STREAM);
    close_case(rc, bytes);
}

void vit_cases() {
    const struct { const char* name; int fused, fp8; } forms[] = {{"plain", 0, 0}, {"fused", 1, 0}, {"fp8_1", 0, 1}, {"fp8_2", 0, 2}, {"fp8_3", 0, 3}};
    for (int s = S32; s <= S16_MIXED; ++s)
        for (const auto& f : forms)
            for (int cls = 1; cls >= 0; --cls) {
                VitCase c;
                c.stream = s; c.fused = f.fused; c.fp8 = f.fp8; c.cls = cls != 0;
                // SwiGLU models but level 3 (whose fc1 output IS fc2's operand): fc1 wider than fc2.k, which no real model is - the
                // MLP hidden's row stride then differs between the forms that take it from the workspace layout and from fc2.k
                if (!cls && f.fp8 != 3) c.fc1_n = 768;
                run_vit(std::string("vit ") + STREAM_NAME[s] + " " + f.name + (cls ? " cls_gelu_lnf" : " nocls_swiglu"), c);
            }
    for (int s = S32; s <= S16_MIXED; ++s) {   // Dp != D: the attention buffer's pad columns are cleared
        VitCase c;
        c.stream = s; c.D = 96;
        run_vit(std::string("vit ") + STREAM_NAME[s] + " plain D96", c);
    }
    // refusals
    for (int s = S32; s <= S16_SAME; ++s) {
        const std::string on = std::string(" over ") + STREAM_NAME[s];
        VitCase c;
        c.stream = s; c.fused = 1; c.fp8 = 1;
        run_vit("vit refused: fp8 with fused" + on, c);
        c = VitCase(); c.stream = s; c.fp8 = 1; c.D = 192;
        run_vit("vit refused: fp8 with D % 128 != 0" + on, c);
        c = VitCase(); c.stream = s; c.fused = 1; c.D = 96;
        run_vit("vit refused: fused with D % 64 != 0" + on, c);
        c = VitCase(); c.stream = s; c.fp8 = 3; c.fc1_n = 512;
        run_vit("vit refused: fp8 level 3 with fc1 width != fc2.k" + on, c);
        c = VitCase(); c.stream = s; c.H = 4; c.W = 6;
        run_vit("vit refused: H != W" + on, c);
        c = VitCase(); c.stream = s; c.ws_short = 1;
        run_vit("vit refused: workspace one byte short" + on, c);
        c = VitCase(); c.stream = s; c.ws_skew = 128;
        run_vit("vit refused: workspace misaligned by 128" + on, c);
    }
    VitCase c;
    c.stream = S16_MIXED; c.fused = 1;
    run_vit("vit refused: fused over a 16-bit stream of another type", c);
    c = VitCase(); c.res_dtype_p1 = 3;
    run_vit("vit refused: residual stream type 2", c);
}

// ---- tdc_qformer_fwd ----------------------------------------------------------------------------------------------------------
void run_qformer(const std::string& name, int mode, int Lt, int D, bool prompts) {
    open_case(name);
    const int Dp = pad64(D), H = 160, Hp = pad64(H), ffn = 256, K = 16, Nenc = 12, n_cross = 2;
    tdc_qformer_layer layers[2];
    memset(layers, 0, sizeof(layers));
    for (int l = 0; l < 2; ++l) {
        const std::string p = "L" + std::to_string(l) + ".";
        tdc_qformer_layer& L = layers[l];
        L.qkv = lin(p + "qkv", 3 * D, Dp); L.attn_out = lin(p + "attn_out", Dp, Dp);
        L.attn_ln_g = ftag(p + "attn_ln_g"); L.attn_ln_b = ftag(p + "attn_ln_b");
        L.has_cross = l == 1; L.cross_idx = l == 1 ? n_cross - 1 : 0;       // the LAST of two stacked cross layers: offsets show
        if (L.has_cross) {
            L.cross_q = lin(p + "cross_q", Dp, Dp); L.cross_out = lin(p + "cross_out", Dp, Dp);
            L.cross_ln_g = ftag(p + "cross_ln_g"); L.cross_ln_b = ftag(p + "cross_ln_b");
            if (mode >= 2) L.cross_q_tiled = tag(p + "cross_q_tiled");
            if (mode >= 1) L.cross_out_tiled = tag(p + "cross_out_tiled");
        }
        L.fq1 = lin(p + "fq1", ffn, Dp); L.fq2 = lin(p + "fq2", Dp, ffn);
        L.fq_ln_g = ftag(p + "fq_ln_g"); L.fq_ln_b = ftag(p + "fq_ln_b");
        L.ft1 = lin(p + "ft1", ffn, Dp); L.ft2 = lin(p + "ft2", Dp, ffn);
        L.ft_ln_g = ftag(p + "ft_ln_g"); L.ft_ln_b = ftag(p + "ft_ln_b");
    }
    tdc_qformer_prompts mp;
    memset(&mp, 0, sizeof(mp));
    mp.n_prompts = 2; mp.enc_frames = 2;
    mp.kv_src = itag("kv_src"); mp.frame_prompt = itag("frame_prompt"); mp.prompt_len = itag("prompt_len"); mp.self_len = itag("self_len");
    tdc_qformer_model m;
    memset(&m, 0, sizeof(m));
    m.dtype = TDC_F16; m.dim = D; m.heads = 2; m.n_layers = 2; m.H = H; m.eps = 1e-12f;
    m.word = ftag("word"); m.pos = ftag("pos"); m.ldw = Dp;
    m.emb_ln_g = ftag("emb_ln_g"); m.emb_ln_b = ftag("emb_ln_b");
    m.cross_kv = lin("cross_kv", n_cross * 2 * D, Hp);
    m.vision_proj = lin("vision_proj", Hp, Dp);
    m.layers_host = layers;
    m.cross_k = lin("cross_k", n_cross * D, Hp);
    m.cross_v = lin("cross_v", n_cross * D, Hp); m.cross_v.b = nullptr;
    m.cross_bv = ftag("cross_bv");
    // the request is always the whole-block kernel; the weights' tiled copies and the shape check decide what runs
    m.xattn_mode = 2;
    m.prompts = prompts ? &mp : nullptr;
    const int F_ = prompts ? 4 : 3;
    g_xattn_ok = mode > 0;
    const size_t bytes = tdc_qformer_workspace_bytes(&m, F_, K, Lt, Nenc);
    g_xattn_ok = mode > 0;
    // enc's row stride is wider than the projections' K: the transposed value GEMM, whose "weight" operand enc is, shows which it takes
    const int rc = tdc_qformer_fwd(&m, tag("enc"), Hp + 64, F_, Nenc, tag("query"), Dp, itag("qsrc"), Lt ? itag("ids") : nullptr, Lt, K,
                                   tag("out"), Hp, (void*)WS, bytes, STREAM);
    close_case(rc, bytes);
}

void qformer_cases() {
    for (int mode = 0; mode <= 2; ++mode)
        for (int Lt = 0; Lt <= 3; Lt += 3)
            for (int D = 96; D <= 128; D += 32)
                for (int prompts = 0; prompts <= 1; ++prompts)
                    run_qformer("qformer mode" + std::to_string(mode) + " Lt" + std::to_string(Lt) + " D" + std::to_string(D) +
                                (prompts ? (mode == 2 ? " prompts (refused)" : " prompts") : ""), mode, Lt, D, prompts != 0);
    // xattn_mode 0 in the model: the shape check is not asked
    open_case("qformer xattn_mode 0 requested");
    {
        tdc_qformer_layer layers[1];
        memset(layers, 0, sizeof(layers));
        layers[0].qkv = lin("L0.qkv", 384, 128); layers[0].attn_out = lin("L0.attn_out", 128, 128);
        layers[0].fq1 = lin("L0.fq1", 256, 128); layers[0].fq2 = lin("L0.fq2", 128, 256);
        tdc_qformer_model m;
        memset(&m, 0, sizeof(m));
        m.dtype = TDC_BF16; m.dim = 128; m.heads = 2; m.n_layers = 1; m.H = 128; m.eps = 1e-12f;
        m.cross_kv = lin("cross_kv", 256, 128); m.vision_proj = lin("vision_proj", 128, 128);
        m.layers_host = layers;
        g_xattn_ok = 1;
        const size_t bytes = tdc_qformer_workspace_bytes(&m, 1, 16, 0, 12);
        const int rc = tdc_qformer_fwd(&m, tag("enc"), 128, 1, 12, tag("query"), 128, itag("qsrc"), nullptr, 0, 16, tag("out"), 128,
                                       (void*)WS, bytes, STREAM);
        close_case(rc, bytes);
    }
}

// ---- tdc_connector_fwd --------------------------------------------------------------------------------------------------------
void run_connector(int C) {
    open_case("connector C" + std::to_string(C));
    const int Cp = pad64(C), Hp = 192;
    tdc_sva_layer layers[2];
    memset(layers, 0, sizeof(layers));
    for (int l = 0; l < 2; ++l) {
        const std::string p = "L" + std::to_string(l) + ".";
        tdc_sva_layer& L = layers[l];
        L.proj_context = lin(p + "proj_context", Cp, Cp); L.proj_in_c = lin(p + "proj_in_c", Cp, Cp); L.proj_in_q = lin(p + "proj_in_q", Cp, Cp);
        L.pos[0] = ftag(p + "pos0"); L.pos[1] = ftag(p + "pos1"); L.ldpos = Cp;
        L.kv[0] = lin(p + "kv0", 2 * Cp, Cp); L.kv[1] = lin(p + "kv1", 2 * Cp, Cp);
        L.q_ln_g = ftag(p + "q_ln_g"); L.q_ln_b = ftag(p + "q_ln_b");
        L.q_proj = lin(p + "q_proj", Cp, Cp); L.o_proj = lin(p + "o_proj", Cp, Cp);
        L.norm_g = ftag(p + "norm_g"); L.norm_b = ftag(p + "norm_b");
        L.out1 = lin(p + "out1", Cp, Cp); L.out2 = lin(p + "out2", Cp, Cp);
    }
    tdc_connector_model m;
    memset(&m, 0, sizeof(m));
    m.dtype = TDC_F16; m.C = C; m.side = 2; m.r = 2; m.heads = 2; m.n_layers = 2;
    for (int i = 0; i < 2; ++i) {
        const std::string p = "aux" + std::to_string(i) + ".";
        m.aux[i].fc1 = lin(p + "fc1", Cp, 64 * (i + 2)); m.aux[i].fc2 = lin(p + "fc2", Cp, Cp);
        m.aux[i].ln_g = ftag(p + "ln_g"); m.aux[i].ln_b = ftag(p + "ln_b");
    }
    m.vision_query = tag("vision_query"); m.ones_C = ftag("ones_C"); m.zeros_C = ftag("zeros_C");
    m.layers_host = layers;
    m.mm1 = lin("mm1", Hp, Cp); m.mm2 = lin("mm2", Hp, Hp);
    const int T = 2;
    const size_t bytes = tdc_connector_workspace_bytes(&m, T);
    const int rc = tdc_connector_fwd(&m, tag("sig"), 128, tag("dino"), 192, T, (const unsigned char*)tag("mask"), tag("out"), Hp,
                                     (void*)WS, bytes, STREAM);
    close_case(rc, bytes);
}

}  // namespace

int main() {
    vit_cases();
    qformer_cases();
    run_connector(96);
    run_connector(128);
    return 0;
}
