// CPU launch trace of tdc_qformer_fwd with kept cross-attention K/V (tdc_qformer_model.kv_keep / kv_state).
//
// The recording stubs, the fake addresses and the printing are those of tests/api_trace/api_trace.cpp, taken in as they are
// (its main() is renamed and never called); this program runs the Q-Former composite over xattn_mode 0 / 1, with and without
// text, single- and multi-prompt, three times each - plain (kv_keep NULL), fill (kv_state 0) and ready (kv_state 1, enc NULL) -
// and the refusals.  tests/test_kv_cache.py compares the three traces of a case with each other: no fixture is recorded.
#define main api_trace_main
#include "../api_trace/api_trace.cpp"
#undef main

namespace {

enum Keep { PLAIN, FILL, READY };

struct KvCase {
    int mode = 1, Lt = 3;
    bool prompts = false;
    int keep = PLAIN;
    int kv_state = -1;          // -1: from `keep`
    long kv_skew = 0;           // bytes added to the kept buffer's address
    bool enc_null = false;
};

void run_kv(const std::string& name, const KvCase& c) {
    open_case(name);
    const int D = 96, Dp = pad64(D), H = 160, Hp = pad64(H), ffn = 256, K = 16, Nenc = 12, n_cross = 2;
    tdc_qformer_layer layers[2];
    memset(layers, 0, sizeof(layers));
    for (int l = 0; l < 2; ++l) {
        const std::string p = "L" + std::to_string(l) + ".";
        tdc_qformer_layer& L = layers[l];
        L.qkv = lin(p + "qkv", 3 * D, Dp); L.attn_out = lin(p + "attn_out", Dp, Dp);
        L.attn_ln_g = ftag(p + "attn_ln_g"); L.attn_ln_b = ftag(p + "attn_ln_b");
        L.has_cross = l == 1; L.cross_idx = l == 1 ? n_cross - 1 : 0;
        if (L.has_cross) {
            L.cross_q = lin(p + "cross_q", Dp, Dp); L.cross_out = lin(p + "cross_out", Dp, Dp);
            L.cross_ln_g = ftag(p + "cross_ln_g"); L.cross_ln_b = ftag(p + "cross_ln_b");
            if (c.mode >= 2) L.cross_q_tiled = tag(p + "cross_q_tiled");
            if (c.mode >= 1) L.cross_out_tiled = tag(p + "cross_out_tiled");
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
    m.xattn_mode = 2;       // as api_trace: the tiled copies and the shape check decide what runs
    m.prompts = c.prompts ? &mp : nullptr;
    void* enc = c.enc_null || c.keep == READY ? nullptr : tag("enc");
    if (c.keep != PLAIN) m.kv_keep = (char*)tag("kv_keep") + c.kv_skew;
    m.kv_state = c.kv_state >= 0 ? c.kv_state : c.keep == READY ? 1 : 0;
    const int F_ = c.prompts ? 4 : 3;
    g_xattn_ok = c.mode > 0;
    const size_t bytes = tdc_qformer_workspace_bytes(&m, F_, K, c.Lt, Nenc);
    g_xattn_ok = c.mode > 0;
    const int rc = tdc_qformer_fwd(&m, enc, Hp + 64, F_, Nenc, tag("query"), Dp, itag("qsrc"), c.Lt ? itag("ids") : nullptr, c.Lt, K,
                                   tag("out"), Hp, (void*)WS, bytes, STREAM);
    close_case(rc, bytes);
}

}  // namespace

int main() {
    const char* const keep_name[] = {"plain", "fill", "ready"};
    for (int mode = 0; mode <= 1; ++mode)
        for (int Lt = 0; Lt <= 3; Lt += 3)
            for (int prompts = 0; prompts <= 1; ++prompts)
                for (int keep = PLAIN; keep <= READY; ++keep) {
                    KvCase c;
                    c.mode = mode; c.Lt = Lt; c.prompts = prompts != 0; c.keep = keep;
                    run_kv("kv mode" + std::to_string(mode) + " Lt" + std::to_string(Lt) + (prompts ? " prompts " : " single ") +
                           keep_name[keep], c);
                }
    KvCase c;
    c.mode = 2; c.keep = FILL;
    run_kv("refused: whole-block kernel, fill", c);
    c.keep = READY;
    run_kv("refused: whole-block kernel, ready", c);
    c = KvCase(); c.keep = FILL; c.kv_state = 2;
    run_kv("refused: kv_state 2", c);
    c = KvCase(); c.keep = FILL; c.kv_state = 0; c.kv_skew = 128;
    run_kv("refused: kv_keep misaligned by 128", c);
    c = KvCase(); c.keep = PLAIN; c.kv_state = 1; c.enc_null = false;
    run_kv("refused: kv_state 1 without kv_keep", c);
    c = KvCase(); c.keep = FILL; c.enc_null = true;
    run_kv("refused: fill without enc", c);
    c = KvCase(); c.keep = PLAIN; c.enc_null = true;
    run_kv("refused: plain without enc", c);
    return 0;
}
