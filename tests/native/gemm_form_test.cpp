// csrc/gemm_form.h on the host: which GEMM form every precision mode and launch shape selects, against the rule written out
// here a second time (vetoes first, the other way round from the header).  g++ -I csrc gemm_form_test.cpp && ./a.out
#include <stdio.h>

#include "gemm_form.h"

using namespace mpe;

static const char *name(GemmForm f) {
    static const char *n[] = {"F32", "F32_ACC64", "SB16", "SB16_F64", "BF16", "F64MM"};
    return n[(int)f];
}

static int bad = 0;

static void check(const char *what, GemmForm got, GemmForm want) {
    if (got == want) return;
    if (++bad <= 20) printf("%s: got %s, want %s\n", what, name(got), name(want));
}

// in_dim x acc64_mink -> does the sum count as long?  (K > mink, 0 = never)
static const int IN_DIMS[4] = {40, 512, 513, 902};
static const int MINKS[2] = {0, 512};
static const bool LONG_K[2][4] = {{false, false, false, false}, {false, false, true, true}};

static GemmForm expect(const GatGemmQuery &q, bool long_k) {
    if (q.gat_reduced) return GemmForm::BF16;                    // the reduced mode: every launch on the plain bf16 MFMA
    const bool f64 = q.gat_acc64 || long_k;
    const GemmForm mfma = f64 ? GemmForm::F32_ACC64 : GemmForm::F32, split = f64 ? GemmForm::SB16_F64 : GemmForm::SB16;
    if (!q.gat_split) return mfma;
    if (q.gathered || q.l0_view) return mfma;                    // layer-0 fc1 per camera
    if (q.gat_acc64 && q.is_l0_fc2) return mfma;                 // explicit f64-sum mode: layer-0 fc2 flushes per stage
    if (q.out_half && (q.leaky || f64 || !q.sb16_tile)) return mfma;     // fp16 rows: the split tile kernel's fp32-chain launches only
    return split;
}

int main() {
    long n = 0;
    for (int bits = 0; bits < 1 << 9; ++bits)
        for (int k = 0; k < 4; ++k)
            for (int mk = 0; mk < 2; ++mk) {
                GatGemmQuery q;
                q.gat_split = bits & 1;
                q.gat_reduced = bits & 2;
                q.gat_acc64 = bits & 4;
                q.out_half = bits & 8;
                q.leaky = bits & 16;
                q.gathered = bits & 32;
                q.l0_view = bits & 64;
                q.is_l0_fc2 = bits & 128;
                q.sb16_tile = bits & 256;
                q.acc64_mink = MINKS[mk];
                q.in_dim = IN_DIMS[k];
                char what[96];
                snprintf(what, sizeof what, "gat bits %#x in_dim %d mink %d", bits, q.in_dim, q.acc64_mink);
                check(what, gat_gemm_form(q), expect(q, LONG_K[mk][k]));
                ++n;
            }

    // the MLP modes of mpe_set_precision, by number
    const GemmForm mlp[6] = {GemmForm::F32, GemmForm::F32_ACC64, GemmForm::BF16, GemmForm::SB16_F64, GemmForm::SB16_F64, GemmForm::F64MM};
    for (int mode = 0; mode < 6; ++mode) check("mlp mode", mlp_gemm_form(static_cast<MlpMode>(mode)), mlp[mode]);
    if (split_flush_stages(MlpMode::Split) != 2 || split_flush_stages(MlpMode::SplitMaxAcc) != 1) {
        printf("flush stages of MLP modes 3 / 4: %d / %d, want 2 / 1\n", split_flush_stages(MlpMode::Split), split_flush_stages(MlpMode::SplitMaxAcc));
        ++bad;
    }

    // the deployed network: fc2 of layer 0 (K = 902) in the default mode, and with f64 sums everywhere
    GatGemmQuery fc2{};
    fc2.gat_split = true;
    fc2.acc64_mink = 512;
    fc2.in_dim = 902;
    fc2.is_l0_fc2 = true;
    fc2.sb16_tile = true;
    check("layer-0 fc2, default mode", gat_gemm_form(fc2), GemmForm::SB16_F64);
    fc2.gat_acc64 = true;
    check("layer-0 fc2, gat_acc64", gat_gemm_form(fc2), GemmForm::F32_ACC64);
    // the per-camera gathered fc1 of layer 0 (K = J * 10): fp32 MFMA whatever gat_split says
    for (int split = 0; split < 2; ++split) {
        GatGemmQuery fc1{};
        fc1.gat_split = split;
        fc1.acc64_mink = 512;
        fc1.in_dim = 180;
        fc1.leaky = true;
        fc1.gathered = true;
        check("gathered layer-0 fc1", gat_gemm_form(fc1), GemmForm::F32);
    }
    printf("tested %ld bad %d\n", n, bad);
    return bad ? 1 : 0;
}
