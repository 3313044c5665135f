// CPU launch trace of tdc_connector_fwd with kept aux rows (tdc_connector_model.aux_keep / ctx_keep).
//
// The recording stubs, the fake addresses and the printing are those of tests/api_trace/api_trace.cpp, taken in as they are
// (its main() is renamed and never called); this program runs the connector composite at C = 96 and 128 twice each - plain
// (the three fields NULL) and keep (all three set) - and the refusals: every partial set and a misaligned buffer.
// tests/test_aux_outputs.py compares the two traces of a case with each other: no fixture is recorded.
#define main api_trace_main
#include "../api_trace/api_trace.cpp"
#undef main

namespace {

// keep: bit 0 aux_keep[0], bit 1 aux_keep[1], bit 2 ctx_keep; skew: bytes added to aux_keep[1]'s address
void run_aux(const std::string& name, int C, int keep, long skew = 0) {
    open_case(name);
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
    if (keep & 1) m.aux_keep[0] = tag("aux_keep0");
    if (keep & 2) m.aux_keep[1] = (char*)tag("aux_keep1") + skew;
    if (keep & 4) m.ctx_keep = tag("ctx_keep");
    const int T = 2;
    const size_t bytes = tdc_connector_workspace_bytes(&m, T);
    const int rc = tdc_connector_fwd(&m, tag("sig"), 128, tag("dino"), 192, T, (const unsigned char*)tag("mask"), tag("out"), Hp,
                                     (void*)WS, bytes, STREAM);
    close_case(rc, bytes);
}

}  // namespace

int main() {
    for (int C = 96; C <= 128; C += 32) {
        run_aux("aux C" + std::to_string(C) + " plain", C, 0);
        run_aux("aux C" + std::to_string(C) + " keep", C, 7);
    }
    for (int keep = 1; keep <= 6; ++keep)
        run_aux("refused: partial set " + std::to_string(keep), 96, keep);
    run_aux("refused: aux_keep[1] misaligned by 128", 96, 7, 128);
    return 0;
}
