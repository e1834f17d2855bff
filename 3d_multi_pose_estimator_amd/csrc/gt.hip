// Ground truth of the metrics scripts from the bodies parsed on the device (include/mpe.h: mpe_gt_from_bodies;
// test/metrics_from_model.py:126-174, harness/common.py:ground_truth / pack_ground_truth).
//
// One workgroup per frame.  Thread 0 picks the camera -- the first entry, replaced by a later one only when it holds
// STRICTLY more bodies, over all entries of the frame, configured or not -- and finds that entry's first row (k_body_layout's
// order: configured cameras first, the others behind them); then a thread per (body, joint) converts and transforms.
// The arithmetic is the header's, written out: the f64 division by 100, one rounding to f32, and per 4x4 product row one
// product and three fmaf.  harness/groundtruth.py states the same in numpy with exact fractions; the two agree bit for bit,
// and that statement is held to torch's CPU matmul by tests/test_groundtruth_host.py.
#include "mpe_internal.h"

namespace mpe {

struct Mat4 {
    float m[16];
};

#pragma clang fp contract(off)
__device__ __forceinline__ float row4(const float *T, float x0, float x1, float x2, float x3) {
    float acc = T[0] * x0;
    acc = __fmaf_rn(T[1], x1, acc);
    acc = __fmaf_rn(T[2], x2, acc);
    acc = __fmaf_rn(T[3], x3, acc);
    return acc;
}

__global__ __launch_bounds__(128) void k_gt_from_bodies(mpe_gt_args a, Mat4 Ti) {
    __shared__ int s_base, s_n;
    const int f = blockIdx.x;
    if (threadIdx.x == 0) {
        const int e0 = a.d_frame_entry_off[f], e1 = a.d_frame_entry_off[f + 1];
        int sel = -1, best = 0;
        for (int e = e0; e < e1; ++e) {
            const int c = a.d_entry_count[e];
            if (sel < 0 || c > best) {
                sel = e;
                best = c;
            }
        }
        long base = 0;
        if (sel >= 0) {
            const bool conf = a.d_entries[sel].cam >= 0;
            for (int e = e0; e < e1; ++e) {
                const bool ce = a.d_entries[e].cam >= 0;
                if (conf ? (ce && e < sel) : (ce || e < sel)) base += a.d_entry_count[e];
            }
        }
        // a frame over scap has raised the parser's capacity bit and is not to be used: stay inside the arrays all the same
        long n = best;
        if (base > a.scap) base = a.scap;
        if (n > a.scap - base) n = a.scap - base;
        if (n > a.gcap) n = a.gcap;
        s_base = (int)base;
        s_n = (int)n;
        a.d_n_gt_in[f] = (int32_t)n;
    }
    __syncthreads();
    const int base = s_base, n = s_n, J = a.n_joints;
    for (int g = threadIdx.x; g < a.gcap; g += blockDim.x)
        a.d_gt_valid[(size_t)f * a.gcap + g] = g < n ? a.d_m1[(size_t)f * a.scap + base + g] : (uint8_t)0;
    const float *Td = a.d_T_d + (size_t)a.d_file_of_frame[f] * 16;
    for (int i = threadIdx.x; i < a.gcap * J; i += blockDim.x) {
        const int g = i / J, j = i - g * J;
        const size_t o = ((size_t)f * a.gcap + g) * J + j;
        float w0 = 0.f, w1 = 0.f, w2 = 0.f;
        uint8_t has = 0;
        if (g < n) {
            const size_t r = (size_t)f * a.scap + base + g;
            has = (uint8_t)(a.d_mask[r] >> j & 1u);
            if (has) {
                const double *v = a.d_xyz + (r * MPE_GT_KEY_SLOTS + j) * 3;
                const float x0 = (float)(v[0] / 100.0), x1 = (float)(v[1] / 100.0), x2 = (float)(v[2] / 100.0);
                const float y0 = row4(Td + 0, x0, x1, x2, 1.f), y1 = row4(Td + 4, x0, x1, x2, 1.f), y2 = row4(Td + 8, x0, x1, x2, 1.f),
                            y3 = row4(Td + 12, x0, x1, x2, 1.f);
                w0 = row4(Ti.m + 0, y0, y1, y2, y3);
                w1 = row4(Ti.m + 4, y0, y1, y2, y3);
                w2 = row4(Ti.m + 8, y0, y1, y2, y3);
            }
        }
        a.d_gt_joint[o] = has;
        a.d_gt_xyz[o * 3 + 0] = w0;
        a.d_gt_xyz[o * 3 + 1] = w1;
        a.d_gt_xyz[o * 3 + 2] = w2;
    }
}

}  // namespace mpe

using namespace mpe;

extern "C" int mpe_gt_from_bodies(mpe_ctx *ctx, void *stream, const mpe_gt_args *a) {
    if (!ctx || !a || a->n_frames < 0 || a->scap < 1 || a->gcap < 1 || a->n_joints < 1 || a->n_files < 1) return MPE_ERR_INVALID;
    if (a->gcap < a->scap || a->n_joints > MPE_GT_M1_SLOT) return MPE_ERR_CAPACITY;
    if (a->n_frames == 0) return MPE_OK;
    if (!a->d_frame_entry_off || !a->d_xyz || !a->d_mask || !a->d_m1 || !a->d_T_d || !a->d_file_of_frame || !a->T_i1 || !a->d_gt_xyz ||
        !a->d_gt_joint || !a->d_gt_valid || !a->d_n_gt_in || !a->d_entries || !a->d_entry_count)
        return MPE_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return MPE_ERR_HIP;
    Mat4 Ti;
    for (int i = 0; i < 16; ++i) Ti.m[i] = a->T_i1[i];
    hipLaunchKernelGGL(k_gt_from_bodies, dim3((unsigned)a->n_frames), dim3(128), 0, static_cast<hipStream_t>(stream), *a, Ti);
    return hipGetLastError() == hipSuccess ? MPE_OK : MPE_ERR_HIP;
}
