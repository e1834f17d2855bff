// Which GEMM form an nn.Linear launch runs on: the one statement of it, as pure functions of the precision mode and the launch's
// shape (no HIP here: tests/native/gemm_form_test.cpp builds this header with the host compiler).  api.hip: gemm() launches the form.
#pragma once
#include <stdint.h>

namespace mpe {

enum class GemmForm {
    F32,         // fp32 MFMA, one fp32 chain (gemm.hip)
    F32_ACC64,   // fp32 MFMA with f64 running sums per 32-deep K stage
    SB16,        // split-bf16 (gemm_sb16.hip): fp32-accurate products on the bf16 matrix pipe, fp32 chain
    SB16_F64,    // split-bf16 with f64 sums (a flush every `flush_stages` K stages)
    BF16,        // plain bf16 MFMA (reduced-precision modes)
    F64MM        // exact products + f64 accumulation on the f64 matrix pipe (gemm_f64.hip)
};

// the MLP modes of mpe_set_precision, by their numbers
enum class MlpMode : int32_t {
    F32 = 0,           // fp32 MFMA, one fp32 chain
    F32Acc64 = 1,      // fp32 MFMA with f64 running sums per K stage (the parity mode of rounds 1-3)
    Bf16 = 2,          // reduced precision: bf16 MFMA
    Split = 3,         // DEFAULT: three bf16 planes per operand, six products, f64 sums every second stage
    SplitMaxAcc = 4,   // the split form with an f64 flush per K stage (maximum accuracy)
    F64 = 5            // every launch on the f64 matrix pipe
};

inline GemmForm mlp_gemm_form(MlpMode mode) {
    switch (mode) {
    case MlpMode::F64: return GemmForm::F64MM;
    case MlpMode::Split:
    case MlpMode::SplitMaxAcc: return GemmForm::SB16_F64;
    case MlpMode::Bf16: return GemmForm::BF16;
    case MlpMode::F32Acc64: return GemmForm::F32_ACC64;
    default: return GemmForm::F32;
    }
}
// MLP modes 3 / 4: K stages per f64 flush of the split form (2 = default, 1 = the maximum-accuracy mode)
inline int split_flush_stages(MlpMode mode) { return mode == MlpMode::SplitMaxAcc ? 1 : 2; }

// What a GEMM of a GAT layer is chosen by
struct GatGemmQuery {
    bool gat_split, gat_reduced, gat_acc64;   // the GAT precision mode (mpe_ctx)
    int acc64_mink;                           // MPE_GAT_ACC64_MINK (default 512; 0 = never)
    int in_dim;                               // K of the layer
    bool out_half;                            // result rows stored as fp16 (the fp16-attention mode)
    bool leaky;
    bool gathered;                            // a_rows || c_rows: layer-0 fc1 per camera
    bool l0_view;                             // the weights are a view into the per-camera matrices (l0_w)
    bool is_l0_fc2;                           // fc2 of layer 0
    bool sb16_tile;                           // linear_sb16_uses_tile_kernel(m, out_dim, false)
};

inline GemmForm gat_gemm_form(const GatGemmQuery &q) {
    // Long sums (K > 512: fc2 of layer 0, K = 902 / 1082, on head rows only -- no measurable cost) always
    // run with f64 running sums: a single fp32 chain of that length was the largest contribution to the
    // score noise (ARPLAB frames of random shape: 3.2e-5 from the reference with it, 2.3e-5 without, where
    // the reference's own fp32 scores sit 1.8e-5 from the float64 network).  MPE_GAT_ACC64_MINK overrides
    // the threshold (0 = never), mpe_set_precision(ctx, 1, .) extends it to every GAT GEMM.
    const bool long_sum = q.gat_acc64 || (q.acc64_mink > 0 && q.in_dim > q.acc64_mink);
    // (fp16 result rows exist in the split TILE kernel only: the fc2 launches at batch sizes the tile kernel takes, without f64
    // sums; every other launch of the fp16-attention mode stays on the fp32 MFMA, whose tile and wave-per-tile kernels all store
    // fp16 rows)
    const bool half_ok = !q.out_half || (!q.leaky && !long_sum && q.sb16_tile);
    // In the explicit f64-sum mode (mpe_set_precision GAT 1 on top of the split form) layer 0's fc2 keeps the fp32 MFMA with a
    // flush per 32-deep stage: the split form flushes every second stage, and on the K = 902 sum of the steep layer-0 features
    // that cadence left one 5x4 fixture frame 1.46x the reference's own distance from the f64 network where the mode promises
    // <= 1 (tests/test_gpu_stages.py::test_score_noise_against_the_f64_network; 0.79 with the flush per stage).
    const bool l0_fc2_f64_mode = q.gat_acc64 && q.is_l0_fc2;
    // (launches with gathered rows -- layer-0 fc1 per camera -- stay on the fp32 MFMA; the grouped layer-0 launch does not come here)
    if (q.gat_split && !q.gat_reduced && half_ok && !q.gathered && !q.l0_view && !l0_fc2_f64_mode)
        // split-bf16 form (gemm_sb16.hip): fp32-accurate products on the bf16 matrix pipe; f64 sums where the fp32 path has them
        return long_sum ? GemmForm::SB16_F64 : GemmForm::SB16;
    // (out_half here = the fp16-attention mode: fp32 MFMA GEMM, result rows stored as fp16)
    if (!q.gat_reduced) return long_sum ? GemmForm::F32_ACC64 : GemmForm::F32;
    return GemmForm::BF16;       // reduced precision: bf16 MFMA with an optional fp16 result
}

}  // namespace mpe
