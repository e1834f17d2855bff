/*
 * mpe.h — C ABI of libmpe_hip.so, the MI355X (gfx950) implementation of the per-frame
 * inference path of gnns4hri/3D_multi_pose_estimator:
 *
 *   2D skeletons per camera -> graph featurisation -> 5-layer graph attention network
 *   -> greedy person clustering -> { MLP 3D regression | pairwise-DLT triangulation }
 *   [-> regrouping of the proposals by reprojection consistency (mpe_regroup_batch), split persons merged and new ones
 *   founded from free skeletons (mpe_consolidate_batch) -> the 3D stage again].
 *
 * The reference has no FFI: its operator API is the set of Python symbols that
 * test/metrics_from_model.py:12-24 and test/metrics_from_triangulation.py:13-23 import.
 * Each entry point below names the reference code it replaces; the Python mirror of
 * those symbols (the .py files of 3d_multi_pose_estimator_amd) is a thin ctypes layer over this
 * file (see INTEGRATION.md for the binding a maintainer would add to the reference).
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions across the boundary;
 *   - every call returns 0 on success or a negative mpe_status; mpe_last_error(ctx)
 *     gives the message of the last failure on that context;
 *   - pointers named d_* are DEVICE pointers owned by the caller (e.g. torch
 *     tensor.data_ptr()); everything else is host memory, copied during the call;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all batch
 *     entry points are asynchronous with respect to the host and allocate nothing;
 *   - one mpe_ctx may be used from one thread at a time.
 */
#ifndef MPE_H
#define MPE_H

#include <stddef.h>     /* size_t */
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPE_MAX_CAMERAS 32      /* camera sets are kept as 32-bit masks in the clustering kernel */
#define MPE_MAX_JOINTS 32       /* joint presence is a 32-bit mask per skeleton */
#define MPE_MAX_GAT_LAYERS 8
#define MPE_MAX_MLP_LAYERS 16

typedef enum {
    MPE_OK = 0,
    MPE_ERR_INVALID = -1,       /* bad argument / shape mismatch                      */
    MPE_ERR_CAPACITY = -2,      /* batch exceeds the capacity given to mpe_create     */
    MPE_ERR_STATE = -3,         /* weights not uploaded yet                           */
    MPE_ERR_HIP = -4,           /* a HIP runtime call failed                          */
    MPE_ERR_NOMEM = -5,
    MPE_ERR_UNSUPPORTED = -6    /* input the device-side parser leaves to the host parser */
} mpe_status;

typedef struct mpe_ctx mpe_ctx;

/* Static configuration = reference `parameters` (parameters.py:12-45) plus the calibration
 * globals the hot-path modules derive at import time (graph_generator.py:32-52,
 * pose_estimator_dataset_from_json.py:28-47).  Cameras are indexed by their position in
 * parameters.used_cameras_skeleton_matching (== used_cameras == camera_names for the
 * shipped presets). */
typedef struct {
    int32_t n_cameras;          /* V_cfg                                               */
    int32_t n_joints;           /* J = len(parameters.joint_list) (18)                 */
    int32_t image_width;        /* parameters.image_width                              */
    int32_t image_height;       /* parameters.image_height                             */
    int32_t numbers_per_joint;  /* parameters.numbers_per_joint (14)                   */
    int32_t min_views;          /* parameters.min_number_of_views                      */
    int32_t median_axis;        /* parameters.axes_3D['Y'][0]                          */
    uint32_t used_joint_mask;   /* bit j set for j in parameters.used_joints           */
    float threshold;            /* CLASSIFICATION_THRESHOLD (0.5)                      */
    double median_window;       /* 0.05 m, compared in f64 as the reference does (pose_estimator_utils.py:73); a double
                                 * (a float until mpe-hip 0.1): float(0.05) = 0.05000000074505806 keeps pairs the
                                 * reference drops; the struct grew by 8 bytes with it, see mpe_version            */
    /* capacities of one batch (workspace is sized from these at mpe_create) */
    int32_t max_frames;
    int32_t max_heads;          /* total 2D skeletons in a batch                       */
    int32_t max_edge_nodes;     /* total cross-camera skeleton pairs in a batch        */
    int32_t max_heads_per_frame;
    int32_t max_persons_per_frame;  /* Pcap, >= floor(max_heads_per_frame / min_views) */
    /* calibration, row-major, host pointers */
    const float *Kinv;          /* [V][9]  torch.inverse(camera_matrix) f32            */
    const float *K;             /* [V][9]  camera_matrix f32                           */
    const float *T_i;           /* [V][16] get_transform(cam,"root") cast to f32       */
    const double *P;            /* [V][12] get_transform("root",cam)[0:3,:] f64        */
    const double *dist;         /* [V][5]  k1,k2,p1,p2,k3 f64 (OpenCV order)           */
} mpe_config;

/* One batch of frames in packed, structure-of-arrays form.  A "head" is one 2D skeleton
 * with at least one joint; heads of a frame are numbered in the reference's order
 * (cameras in the frame dict's key order, then list order; graph_generator.py:583-601).
 * A "slot" is one camera of that dict order.  All pointers are device pointers. */
typedef struct {
    int32_t n_frames;
    int32_t n_heads;                 /* total heads in the batch                        */
    int32_t n_edge_nodes;            /* total edge-nodes (cross-slot head pairs)        */
    const int32_t *d_frame_head_off; /* [n_frames+1] exclusive prefix of heads          */
    const int32_t *d_frame_en_off;   /* [n_frames+1] exclusive prefix of edge-nodes     */
    const int32_t *d_slot_cam;       /* [n_frames][V] camera index of slot s, -1 unused */
    const int32_t *d_slot_n;         /* [n_frames][V] number of heads in slot s         */
    const int32_t *d_head_cam;       /* [n_heads] camera index                          */
    const uint32_t *d_joint_mask;    /* [n_heads] bit j: joint j present in the dict    */
    const uint32_t *d_tri_mask;      /* [n_heads] bit j: present and values[0] > 0      */
    const double *d_xy;              /* [n_heads][J][2] pixel x,y (values[1], values[2])*/
    const float *d_vp;               /* [n_heads][J][2] values[3] (valid), values[4]    */
    /* Optional EXPLICIT edge-node list, NULL = the implicit one of process_test (every cross-slot head pair once,
     * graph_generator.py:854-864).  [n_edge_nodes][2] frame-local head ids (h1, h2) of edge-node m, frames back to back
     * as d_frame_en_off says; edge-node X = (h1,h2) carries the edges (h1,X),(X,h1),(h2,X),(X,h2),(X,X) in that order
     * (add_edge_node_to_graph, :627-656).  This is the topology of MergedMultipleHumansDataset.process_training
     * (:672-810; mode 'test_generated' of test/sm_metrics_without_gt.py:108): heads grouped by person instead of by
     * camera slot and one edge-node per ORDERED head pair -- or any other pair list.  The heads may then come in any
     * order; d_slot_cam / d_slot_n are not read and may be NULL.  Per-frame limits, checked on the device and reported by
     * mpe_sync_status: heads <= max_heads_per_frame, edge-nodes <= the power of two >= max(512, max_heads_per_frame^2 / 2 + 1),
     * every pair inside its frame with h1 != h2 (else MPE_ERR_INVALID).  A process_training-style graph holds one edge-node per ORDERED
     * cross-camera head pair, up to H^2 (V - 1) / V of them: with V = 5 a frame of H heads fits while 0.8 H^2 <= that power of two
     * (H <= 35 at max_heads_per_frame = 40, whose capacity is 1024) -- a larger frame is reported (MPE_ERR_CAPACITY), never
     * truncated; raise max_heads_per_frame to make room.  Available on contexts with
     * max_heads_per_frame <= 1024 whose per-frame node ids fit 16 bits (MPE_ERR_UNSUPPORTED otherwise). */
    const int32_t *d_en_pair;
    /* What the caller changes (to any other value) whenever it REWRITES the contents of the arrays above in place: same
     * addresses, another batch.  The library cannot see such a rewrite; it compares this number where it keeps something it
     * computed from the arrays from one call to the next (today: mpe_mlp3d_batch, which has the rule).  0 is a value like
     * any other; a host that never reuses an address between mpe_match_batch and mpe_mlp3d_batch may leave it alone. */
    uint64_t generation;
} mpe_batch;

/* ---- environment switches of the library (diagnostics; none is needed in production) -------------------------------------------
 * The list is FROZEN (round 5; round 6 added the two MPE_LATENCY_* switches with the small-batch launches): these are all the variables
 * csrc/ reads.  Read once per process unless marked "per call".
 *   kernel selection, each a cross-check path the GPU suite is run under (tools/run_switch_matrix.sh):
 *     MPE_SKINNY_WAVES=<n>        16 x 16 tiles up to which the wave-per-tile GEMM kernels run (default 1024; 0 = tile kernels always)
 *     MPE_GEMM_NARROW=0           narrow outputs (<= 16 / 64 features) on the tile kernels as well
 *     MPE_GAT_ACC64_MINK=<k>      GAT launches with K > k get f64 running sums (default 512: fc2 of layer 0; 0 = never -- that CHANGES the
 *                                 numerics: the 2e-5 score bound rests on these sums, profiles/r05_switch_matrix.txt; not a cross-check path)
 *     MPE_L0_GROUPED=0            layer-0 fc1 dense over the whole 902-wide row instead of per camera block
 *     MPE_NO_COEF_EPILOGUE        (per call) attention coefficients from k_attn_coef instead of the fc2 epilogue
 *     MPE_NO_FUSED_ATTENTION      (per call) the general attention kernels for every frame size
 *     MPE_FUSED_NO_OVERLAP        (per call) plain staging in k_gat_fused
 *     MPE_NO_HEAD_SRC_TABLE       (per call) in-edge sources derived in the kernels instead of read from the per-batch table
 *     MPE_CLUSTER_KERNEL=wave|block|lds|big   (per call) clustering kernel
 *     MPE_HALF_VEC=4              fp16 rows of the general attention kernels read 4 columns per thread instead of 8
 *     MPE_JSON_WGS=<n>            workgroups of the device-side JSON walk
 *     MPE_LATENCY_PATH=0          (per call) batches of at most 16 frames through the batch path's own small-batch kernels instead of the
 *                                 latency launches of csrc/lat.hip / gat.hip (k_lat_l0a, k_lat_gemm, k_lat_attention; persons' prefix and
 *                                 decode folded into their neighbours): same bits either way (tests/test_gpu_latency.py)
 *   host packer (threads, timing prints): MPE_PACK_THREADS, MPE_SCAN_THREADS, MPE_SCAN_CHUNK_KB, MPE_PACK_NO_SIMD, MPE_PACK_TIMING,
 *     MPE_STAGE_TIMING
 * Gone since round 5 (their code left the library): MPE_GEMM_TUNE, MPE_GEMM_BN, MPE_GEMM_LOADER, MPE_SB_GAT_MW, MPE_SB_PERS,
 * MPE_SB_LDS_PAD, and the compile-time ablation switches MPE_EXP / MPE_SBEXP.  `make exp EXPFLAGS=-DMPE_SB_CLOCK` builds the one
 * diagnostic variant left: in-kernel clock stamps of the split-bf16 tile kernel (tools/sb_clock_probe.py).
 * Round 6 built and removed two experiments with their switches (MPE_LATENCY_MLP, MPE_MLP_CHAIN, mpe_linear flag bit 6): the records are
 * profiles/r06_mlp_fp32_weights_experiment.txt and profiles/r06_mlp_chain_experiment.txt, the code is in commit 102284c. */

/* ---- lifetime ------------------------------------------------------------------------ */
int mpe_create(const mpe_config *cfg, mpe_ctx **out);
void mpe_destroy(mpe_ctx *ctx);
const char *mpe_last_error(const mpe_ctx *ctx);
const char *mpe_version(void);           /* "mpe-hip 0.3 ...": 0.2 = mpe_config.median_window is a double (the layout of 0.1 had a float); 0.3 = mpe_batch ends with `generation` */

/* ---- weights (host pointers, copied once; ctx owns padded device copies) ---------------
 * GAT2 state-dict tensors of layer l (gat2.py:18-48): fc1.weight [in][in], fc1.bias [in],
 * fc2.weight [heads*out][in], fc2.bias [heads*out], attn_l / attn_r [heads][out].
 * Limits: 2 <= n_layers <= MPE_MAX_GAT_LAYERS (mpe_set_gat_params); any in_dim / out_dim, at most 16 attention heads per layer;
 * the last layer is 1 head x 1 output (n_classes = 1: one score per node).  The last two are checked at the first batch call,
 * before anything is allocated or launched: MPE_ERR_INVALID.  (tests/test_gpu_gat_archs.py runs other shapes than the deployed one.) */
int mpe_set_gat_params(mpe_ctx *ctx, int32_t n_layers, float alpha, float hidden_slope);
int mpe_set_gat_layer(mpe_ctx *ctx, int32_t layer, int32_t in_dim, int32_t heads, int32_t out_dim,
                      const float *fc1_w, const float *fc1_b, const float *fc2_w, const float *fc2_b,
                      const float *attn_l, const float *attn_r);
/* PoseEstimatorMLP (utils/mlp.py:8-28): layer l = Linear(in,out) [+ LeakyReLU(slope)] */
int mpe_set_mlp_params(mpe_ctx *ctx, int32_t n_layers, float slope);
int mpe_set_mlp_layer(mpe_ctx *ctx, int32_t layer, int32_t in_dim, int32_t out_dim,
                      const float *w, const float *b);

/* Arithmetic of the GEMMs.  0 = one fp32 MFMA chain over the whole K; 1 = fp32 MFMA, every 32-deep K stage flushed into f64
 * running sums, so a dot product carries about one rounding, like a blocked CPU sgemm.  MLP mode 3 (the MLP DEFAULT since round
 * 4) = the same accuracy class on the bf16 matrix pipe: every fp32 operand is taken as the exact sum of three bf16 numbers, the
 * six significant partial products run on v_mfma_f32_16x16x32_bf16 with fp32 accumulators flushed into f64 sums every second
 * stage (csrc/gemm_sb16.hip; measured error against exactly evaluated dot products: that of mode 1 or below, 1.35x faster
 * launches).  MLP mode 4 = mode 3 with an f64 flush after EVERY stage: the maximum-accuracy form (rms error of a launch 0.13-0.18
 * instead of 0.24-0.26 ulp of its output scale; the MLP launches take ~7 % longer).  MLP mode 5 = the f64-evaluated network: exact
 * fp32 x fp32 products accumulated in f64 over the whole K on the f64 matrix pipe (v_mfma_f64_16x16x4_f64, csrc/gemm_f64.hip), bias and
 * LeakyReLU in f64, fp32 rounding between layers; several times slower, for parity work.  Its LeakyReLU multiplies by the network's
 * parameter as a double: the seven-digit decimal that rounds to the fp32 slope given to mpe_set_mlp_params (0.1 for
 * nn.LeakyReLU(0.1), utils/mlp.py:11), or that fp32 value itself when no such decimal exists -- the network, not a replay of the
 * reference's fp32 kernel (which multiplies by (float)0.1).  Defaults: GAT 4 (below), MLP 3 (the MLP's K is up to 3072 and its 3D output is compared with the reference at the
 * micrometre level: DESIGN.md section 5; mode 1 stays selectable).  MLP mode 2 is the
 * reduced-precision variant of BASELINE.json configs[4]: weights and staged activations in
 * bf16, v_mfma_f32_16x16x32_bf16 with fp32 accumulation (~3 significant digits; not parity).
 * GAT mode 2 is the other half of that config: fc1/fc2 on the bf16 MFMA and the transformed
 * features (ft2) stored as fp16 rows for the attention stage (coefficients, softmax and sums
 * stay fp32; the layer-0 edge-node constants stay fp32).  GAT mode 3 is configs[4] as BASELINE.json words it
 * ("fp16 GATv2 attention + bf16 MLP" with MLP mode 2): only the ft2 rows are fp16 -- fc2 stores them from its fp32
 * results, the attention coefficients a1/a2 still come from the fp32 values in the GEMM epilogue -- and fc1/fc2 stay
 * on the fp32 MFMA.  GAT modes 4 (the GAT DEFAULT since round 4), 5 and 6 are modes 0, 1 and 3 with fc1 / fc2 of the layers
 * >= 1 in the split-bf16 form of MLP mode 3 (fp32-accurate: rms error of a launch at or below the fp32 MFMA chain's, 1.5x
 * faster launches; without f64 sums where mode 0 has none); layer 0's gathered launches stay on the fp32 MFMA.  In mode 6 the
 * fc2 launches store their fp16 rows from the split tile kernel when the batch is large enough for it (more than
 * MPE_SKINNY_WAVES = 1024 16 x 16 tiles, more than one 16-wide output tile); every other fp16-row launch (small batches, the
 * 1-wide last layer, f64-sum launches) stays on the fp32 MFMA, whose kernels all store fp16 rows. */
int mpe_set_precision(mpe_ctx *ctx, int32_t gat_acc64, int32_t mlp_acc64);

/* ---- batch entry points ---------------------------------------------------------------
 * mpe_match_batch replaces, per frame: MergedMultipleHumansDataset(mode='test', alt='3')
 * (graph_generator.py:813-876), GAT2.forward (gat2.py:137-149) and
 * get_person_proposal_from_network_output (skeleton_matching_utils.py:12-132).
 *   d_scores   [n_edge_nodes]  sigmoid output of every edge-node (may be NULL)
 *   d_persons  [n_frames][Pcap][V] frame-local head id per camera, -1 = None
 *   d_n_persons[n_frames]
 * Non-finite input.  A detection may be inf, NaN, or finite as a double and infinite as a float (1e39 is a legal JSON number;
 *   d_xy is f64 and the network's rows are f32).  Values of a joint whose bit in d_joint_mask is CLEARED are never read: whatever
 *   they hold, no result of any frame changes.  A non-finite value under a SET bit affects its own frame only: every other frame
 *   of the batch keeps every bit of its scores, persons and count.  The frame's own scores may be NaN (a NaN score is below every
 *   threshold); its person table stays structurally valid -- 0 <= n <= Pcap, every entry -1 or a frame-local head of that column's
 *   camera, no head twice.  The call returns MPE_OK and raises no status bit.  Nothing survives into later calls on the context:
 *   the batches after a bad one give the bits a fresh context gives (tests/test_gpu_nonfinite.py; which workspace columns that
 *   rests on: DESIGN.md 5.1).
 * A batch of zero frames is accepted by every batch entry point and does nothing. */
int mpe_match_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b,
                    float *d_scores, int32_t *d_persons, int32_t *d_n_persons);

/* 3D stage A: PoseEstimatorDataset dict branch (pose_estimator_dataset_from_json.py:237-298,
 * incl. get_3D_from_triangulation :63-101) + PoseEstimatorMLP + x10 decode
 * (metrics_from_model.py:243-294).
 *   d_poses [n_frames][Pcap][J][3] f32 metres, d_valid [n_frames][Pcap] 1 = person row kept
 * Small batches (<= 16 frames): mpe_match_batch has already solved every cross-camera skeleton pair of its batch beside its clustering
 * launch, and the row kernel here fetches them instead of solving (same function, same arguments: same bits) -- in ONE case only: this
 * call is the context's first batch call after that mpe_match_batch, and it is handed the same batch (every array pointer, the
 * generation and the three counts equal) and the d_persons / d_n_persons arrays that call wrote.  The hand-off is used once: any batch
 * entry point of the context (every function that takes an mpe_batch, this one included) ends it, and everything else solves its pairs
 * itself.  Results never depend on which of the two happens.
 * Non-finite input.  As at mpe_match_batch, per PERSON: values under a cleared mask bit are never read; a non-finite value under a
 *   set bit affects the slots of the persons that hold its head and no other slot of the frame or the batch (poses and flags, bit
 *   for bit).  d_valid of such a slot is what the reference's own test sum(|row|) > 1 gives on its row: 0 when the row holds a NaN,
 *   1 when it holds infinities only; the pose under a set flag is then whatever the network makes of the row.  MPE_OK, no status
 *   bit, and nothing survives into later calls (rows of NaN in the MLP workspaces included, with more or fewer persons after).
 * THE CALLER'S RULE.  One thing the library cannot see: new contents written into the same arrays between the two calls (a copy into
 * a reused arena, a kernel of the caller's) with equal counts, and persons at the same address.  A caller that rewrites a batch's
 * arrays between mpe_match_batch and mpe_mlp3d_batch -- instead of matching the new contents first, as the pipeline's call order does --
 * must change mpe_batch::generation with the rewrite.  (Python: DeviceBatch.upload / rebind and every new DeviceBatch / ParsedOnDevice
 * take a fresh generation; code that copies into a batch's buffer by hand calls rebind.) */
int mpe_mlp3d_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b,
                    const int32_t *d_persons, const int32_t *d_n_persons,
                    float *d_poses, uint8_t *d_valid);

/* 3D stage B: caller gather + triangulate (metrics_from_triangulation.py:234-272,
 * pose_estimator_utils.py:52-75).
 *   d_poses [n_frames][Pcap][J][3] f64, d_joint_valid [n_frames][Pcap][J] 1 = joint emitted
 * Non-finite input.  As at mpe_match_batch, per person: values under a cleared mask bit are never read; a non-finite value under a
 *   set bit affects the joints of the persons that hold its head (the pair solves run a fixed number of sweeps, the median search
 *   ends without a result on NaN) and no other slot.  MPE_OK, no status bit; the call keeps nothing on the context.
 *   flags bit 0: emit every triangulated joint (what `triangulate` itself returns); otherwise
 *   joints outside parameters.used_joints come back as zeros, as the caller's copy does.
 *   flags bit 1: gather only joints whose values[0] (the joint id) is > 0, as the caller in
 *   test/reprojection_error.py:296-300 does (joint 0 is then never triangulated). */
int mpe_triangulate_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b,
                          const int32_t *d_persons, const int32_t *d_n_persons,
                          double *d_poses, uint8_t *d_joint_valid, uint32_t flags);

/* Evaluation: error table and pose-to-ground-truth assignment of the callers' scoring loop
 * (metrics_from_model.py:303-337, metrics_from_triangulation.py:281-320), per frame of a batch.
 * Detections of frame f: persons p < d_n_persons[f] in order; with joint_flags == 0 (MLP mode) only those with
 * d_flags[f][p] != 0, all joints present; with joint_flags == 1 (triangulation) all of them, joint j present when
 * d_flags[f][p][j] != 0.  Detection r of a frame is its r-th such person.
 *   d_table[f][g][r] f64 [n_frames][gcap][pcap]: mean over the used joints of GT body g (d_gt_joint != 0 and bit j of
 *   used_joint_mask, increasing j) that the detection has, of |pose - gt|; 0 if there is none.  pose_f64 == 0: f32
 *   poses, the f32 arithmetic of numpy's float32 dot / norm and a f32 mean; pose_f64 == 1: f64 poses minus the f32 GT,
 *   f64 throughout.  d_invalid[f][r] = 1 when a used joint of any GT body is missing from detection r.
 *   d_assign[f][r] = the GT row of detection r in the first permutation (itertools order over range(max(G, R)))
 *   whose left-fold f64 sum is the minimum below 10000., -1 if none; d_err[f][r] = d_table[f][g][r] for that row.
 *   d_n_gt / d_n_res / d_status per frame.  A frame with d_skip[f] != 0 (d_skip may be NULL) gets status
 *   MPE_EVAL_SKIPPED and no rows.  The search runs on the device for max(G, R) <= 64 within a fixed node budget;
 *   other frames get MPE_EVAL_OVER_CAP / MPE_EVAL_OVER_BUDGET and their rows of d_assign stay -1: the caller
 *   finishes them from d_table.  MPE_ERR_CAPACITY for pcap > 1024, gcap > 1024 or n_joints > MPE_MAX_JOINTS. */
enum {
    MPE_EVAL_SKIPPED = 1,
    MPE_EVAL_OVER_CAP = 2,
    MPE_EVAL_OVER_BUDGET = 4,
    MPE_EVAL_NO_ASSIGNMENT = 8
};
typedef struct {
    int32_t n_frames, pcap, n_joints, gcap;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t used_joint_mask;
    const void *d_poses;
    const uint8_t *d_flags;
    const int32_t *d_n_persons;    /* [n_frames] */
    const float *d_gt_xyz;         /* [n_frames][gcap][J][3] world, metres */
    const uint8_t *d_gt_joint;     /* [n_frames][gcap][J] */
    const uint8_t *d_gt_valid;     /* [n_frames][gcap] (not read: carried for the caller's bookkeeping) */
    const int32_t *d_n_gt_in;      /* [n_frames] bodies per frame, <= gcap */
    const uint8_t *d_skip;         /* [n_frames] or NULL */
    double *d_table;               /* [n_frames][gcap][pcap] */
    int32_t *d_assign;             /* [n_frames][pcap] */
    double *d_err;                 /* [n_frames][pcap] */
    uint8_t *d_invalid;            /* [n_frames][pcap] */
    int32_t *d_n_gt, *d_n_res, *d_status;   /* [n_frames] */
} mpe_eval_args;
int mpe_eval_batch(mpe_ctx *ctx, void *stream, const mpe_eval_args *a);

/* Reprojection residuals: how well a 3D pose agrees with the 2D detections it came from (test/reprojection_error.py:
 * 89-107, 350-420) -- a quality signal that needs no ground truth.
 *   d_res[f][p][c][j] f64 [n_frames][pcap][V][J]: the pixel distance between the projection of joint j of person p into
 *   camera c and the detection of that joint in the skeleton d_persons[f][p][c] names; -1 (a negative sentinel) where
 *   nothing is counted: p >= d_n_persons[f], the camera has no head for the person, bit j of joint_mask is clear, the
 *   person's flag (joint_flags == 0: d_flags[f][p]) or the joint's flag (joint_flags == 1: d_flags[f][p][j]) is 0, joint
 *   j is absent from that skeleton (d_joint_mask of the batch), or its `valid` (d_vp, fp32) is not > threshold (strict,
 *   :365).  The script's rows: `est` = the MLP poses (f32, person flags, used_joint_mask); `triang` = the triangulated
 *   poses (f64, joint flags, all joints); `GT` = ground-truth bodies as f32 poses with a one-bit joint_mask.
 * Arithmetic: get_projected_coordinates (:89-107) in fp32, f64 poses rounded to fp32 first (:405); every operation rounded
 * on its own (nothing fused), quotients and roots correctly rounded, in this order (harness/reprojection.py states the same
 * on the host, and the two agree bit for bit):
 *   T  = (float) cfg.P[c] ; kd = (float) cfg.dist[c][0], [1], [4]         radial terms only
 *   pc_i = ((T[i][0]*X + T[i][1]*Y) + T[i][2]*Z) + T[i][3]                i = 0..2
 *   h0 = pc_0 / pc_2 ; h1 = pc_1 / pc_2 ; n = sqrt(h0*h0 + h1*h1) ; r = n*n
 *   f  = ((1 + kd0*r) + (kd1*r)*r) + ((kd2*r)*r)*r ; d0 = h0*f ; d1 = h1*f
 *   u_i = (K[c][i][0]*d0 + K[c][i][1]*d1) + K[c][i][2] ; px = u_0 / u_2 ; py = u_1 / u_2
 *   res = sqrt(((double)px - x)*((double)px - x) + ((double)py - y)*((double)py - y))          f64 (:366)
 * n_frames must equal the batch's, n_joints the context's. */
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t joint_mask;           /* bit j: joint j is projected                                    */
    float threshold;               /* 0.5 in the script                                              */
    const int32_t *d_persons;      /* [n_frames][pcap][V], as the matching stage writes them         */
    const int32_t *d_n_persons;    /* [n_frames]                                                     */
    const void *d_poses;
    const uint8_t *d_flags;
    double *d_res;                 /* [n_frames][pcap][V][J]                                         */
} mpe_reproject_args;
int mpe_reproject_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_reproject_args *a);

/* Per-camera statistics of one or more residual buffers of the layout above (the script's np.mean / np.median per camera
 * over a whole run, :422-430; medians do not compose across batches, so the buffers of all batches are kept and read
 * here once).  Per camera c of the context:
 *   d_count[c]      i64  entries >= 0
 *   d_nonfinite[c]  i64  entries that are NaN or infinite
 *   d_sum[c]        f64  sum of the entries that are not negative, reduced in a fixed order (the same input gives the
 *                        same bits); NaN when an entry is NaN -- mean and median of that camera are then NaN, as numpy's
 *   d_mid[c][2]     f64  the elements of rank (n-1)/2 and n/2 among the n entries >= 0 in ascending order, EXACT (a radix
 *                        select over the 64-bit patterns, which order like the non-negative doubles they encode; +inf is
 *                        the largest; an entry of -0.0 counts as 0 and comes back as +0.0); np.median is
 *                        (d_mid[c][0] + d_mid[c][1]) / 2.  NaN when n == 0.
 * d_res and n_groups are HOST arrays of n_buffers entries: the device pointer and n_frames * pcap of each buffer (0 =
 * skipped).  MPE_ERR_CAPACITY beyond 2^32 - 1 entries per camera.  The select state, the histograms and the partial sums
 * are workspace of the context: one call at a time per context, also across streams (as for every batch entry point,
 * one mpe_ctx serves one thread and one stream of work at a time). */
typedef struct {
    int32_t n_buffers, n_joints;
    const double *const *d_res;
    const int64_t *n_groups;
    int64_t *d_count, *d_nonfinite;    /* [V]    */
    double *d_sum;                     /* [V]    */
    double *d_mid;                     /* [V][2] */
} mpe_residual_stats_args;
int mpe_residual_stats(mpe_ctx *ctx, void *stream, const mpe_residual_stats_args *a);

/* Refinement: every joint of every pose moved to the point that minimises its reprojection error over all cameras that saw
 * it (the non-linear "optimal triangulation" step; the DLT stage is a median of two-view solutions, the MLP never looks at
 * the pixels again).  One 3-unknown Levenberg-Marquardt problem per (frame, person, joint), all binary64, every operation
 * named below rounded on its own (nothing fused), quotients and roots correctly rounded.  harness/refine.py states the same
 * in numpy, and the two agree bit for bit.
 * Observations.  Camera c observes joint j of person p of frame f exactly when mpe_reproject_batch, given the same
 *   d_persons / d_n_persons / d_poses / d_flags / pose_f64 / joint_flags / joint_mask / threshold, would count
 *   d_res[f][p][c][j] (the rule above).  n_views = the number of such cameras; x, y = that detection (d_xy, f64).
 * Projection of X = (X0, X1, X2) into camera c, with T = cfg.P[c] as stored, kd0, kd1, kd2 = cfg.dist[c][0], [1], [4] and
 *   K = (double) cfg.K[c] (all three rows as stored):
 *   pc_i = ((T[i][0]*X0 + T[i][1]*X1) + T[i][2]*X2) + T[i][3]             i = 0..2
 *   h0 = pc_0 / pc_2 ; h1 = pc_1 / pc_2 ; r = h0*h0 + h1*h1
 *   f  = ((1 + kd0*r) + (kd1*r)*r) + ((kd2*r)*r)*r ; d0 = h0*f ; d1 = h1*f
 *   u_i = (K[i][0]*d0 + K[i][1]*d1) + K[i][2] ; px = u_0 / u_2 ; py = u_1 / u_2
 *   rx = px - x ; ry = py - y ; e = sqrt(rx*rx + ry*ry)
 * Jacobian of (px, py) by X_k, k = 0..2 (the derivative of exactly the lines above):
 *   fd = (kd0 + (2*kd1)*r) + ((3*kd2)*r)*r
 *   a_k = (T[0][k] - h0*T[2][k]) / pc_2 ; b_k = (T[1][k] - h1*T[2][k]) / pc_2
 *   q_k = fd * (2 * (h0*a_k + h1*b_k)) ; m_k = a_k*f + h0*q_k ; n_k = b_k*f + h1*q_k
 *   v_ik = K[i][0]*m_k + K[i][1]*n_k                                      i = 0..2
 *   jx_k = (v_0k - px*v_2k) / u_2 ; jy_k = (v_1k - py*v_2k) / u_2
 * Cost.  C(X) = the left-fold sum, over the observing cameras in increasing c from 0.0, of rho(e_c):
 *   rho(e) = e*e when huber_px <= 0 or e <= huber_px, else (2*huber_px)*e - huber_px*huber_px;
 *   the weight w_c is 1 in the first case and huber_px / e in the second.  huber_px = 0 is plain least squares.
 * Iteration.  X = the input joint widened to f64, lambda = 1e-3, C = C(X).  At most max_iters times:
 *   A_kl (k <= l) and g_k start at 0.0 and take, per observing camera in increasing c,
 *     A_kl = A_kl + w_c * (jx_k*jx_l + jy_k*jy_l) ; g_k = g_k + w_c * (jx_k*rx + jy_k*ry)
 *   M_kk = A_kk + lambda*A_kk, M_kl = A_kl; (A + lambda diag A) delta = -g by LDL^T:
 *     D0 = M_00 ; L10 = M_01 / D0 ; L20 = M_02 / D0 ; D1 = M_11 - L10*M_01 ; t = M_12 - L20*M_01 ; L21 = t / D1
 *     D2 = (M_22 - L20*M_02) - L21*t
 *     z0 = -g_0 ; z1 = -g_1 - L10*z0 ; z2 = (-g_2 - L20*z0) - L21*z1
 *     delta_2 = z2 / D2 ; delta_1 = z1 / D1 - L21*delta_2 ; delta_0 = (z0 / D0 - L10*delta_1) - L20*delta_2
 *   A pivot D0, D1 or D2 that is not > 0, or a delta that is not finite, rejects the iteration.  Otherwise the trial point
 *   is X + delta; it is accepted only if pc_2 > 0 there in every observing camera and C(trial) < C (strict; a NaN rejects).
 *   Accepted: X = trial, C = C(trial), lambda = max(lambda / 10, 1e-12), and the loop ends when max |delta_k| < step_tol
 *   (metres; step_tol = 0 runs every iteration).  Rejected: lambda = lambda * 10.
 * The result is X in the type of d_poses (f32: rounded once); a joint that never moved keeps its input bits.
 * Not solved -- the joint is copied through bit for bit, d_cost0 = d_cost1 = -1, d_iters = 0: no observing camera (status
 *   0); one observing camera (MPE_REFINE_FEW_VIEWS); a start that is not finite, or that has pc_2 <= 0 (or NaN) in an
 *   observing camera (MPE_REFINE_BAD_START).
 * Outputs per [n_frames][pcap][J]: d_status (bits below; MPE_REFINE_MOVED: at least one accepted step; _CONVERGED: ended
 *   by step_tol), d_cost0 / d_cost1 (C at the start and at the result, on the f64 point; d_cost1 <= d_cost0 and, without
 *   _MOVED, equal), d_iters (iterations run, rejected ones included), d_n_views.  d_poses_out may be d_poses itself.
 * One launch, ordered on `stream`; neither synchronises nor allocates; n_frames == 0 does nothing.  MPE_ERR_INVALID for
 * max_iters outside 1..64, a negative (or NaN) step_tol or huber_px, n_frames other than the batch's or n_joints other
 * than the context's. */
enum {
    MPE_REFINE_SOLVED = 1,
    MPE_REFINE_MOVED = 2,
    MPE_REFINE_CONVERGED = 4,
    MPE_REFINE_FEW_VIEWS = 8,
    MPE_REFINE_BAD_START = 16
};
#define MPE_REFINE_MAX_ITERS 64
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t joint_mask;           /* bit j: joint j is refined                                      */
    float threshold;               /* 0.5, as for mpe_reproject_batch                                */
    int32_t max_iters;             /* 1 .. MPE_REFINE_MAX_ITERS                                      */
    double step_tol;               /* metres, >= 0                                                   */
    double huber_px;               /* pixels, >= 0; 0: plain least squares                           */
    const int32_t *d_persons;      /* [n_frames][pcap][V]                                            */
    const int32_t *d_n_persons;    /* [n_frames]                                                     */
    const void *d_poses;
    const uint8_t *d_flags;
    void *d_poses_out;             /* [n_frames][pcap][J][3], the type of d_poses                    */
    uint8_t *d_status;             /* [n_frames][pcap][J]                                            */
    double *d_cost0, *d_cost1;     /* [n_frames][pcap][J]                                            */
    uint8_t *d_iters, *d_n_views;  /* [n_frames][pcap][J]                                            */
} mpe_refine_args;
int mpe_refine_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_refine_args *a);

/* Uncertainty: the 3 x 3 covariance of every joint of every pose, in metres^2, from the cameras that saw it -- how far a
 * joint can be trusted: five well-spread cameras and two nearly parallel ones leave mpe_refine_batch with the same flag.
 * With independent pixel noise of standard deviation sigma_px in x and in y, the covariance of the minimiser of the
 * reprojection cost is Sigma = sigma_px^2 * A^-1, A = sum_c w_c J_c^T J_c at that point: the Gauss-Newton approximation.
 * With a Huber weight it is the usual weighted approximation, not the sandwich estimator.  It is the covariance of the
 * per-frame estimate: untimed (camera lags are ignored, as in the DLT), and it says nothing about what smoothing or a
 * bone-length fit do afterwards.  It describes d_poses as the minimum of the cost; on poses that are not refined it is the
 * covariance the refined joint would have, to first order.  All binary64, every operation named below rounded on its own
 * (nothing fused), quotients and roots correctly rounded.  harness/uncertainty.py states the same in numpy, and the two
 * agree bit for bit; csrc/cov3.h holds the inverse for host and device.
 * Inputs per (frame, person, joint): the observing cameras, n_views, x, y, the projection of X = the joint widened to f64,
 *   rx, ry, e, the Jacobian jx_k, jy_k and the weight w_c are exactly those of mpe_refine_batch at its start, given the
 *   same batch, d_persons / d_n_persons / d_poses / d_flags / pose_f64 / joint_flags / joint_mask / threshold / huber_px.
 * Normal matrix.  A_kl (k <= l) starts at 0.0 and takes, per observing camera in increasing c,
 *   A_kl = A_kl + w_c * (jx_k*jx_l + jy_k*jy_l)                           (the line of mpe_refine_batch)
 * Inverse.  A = L D L^T by the lines of mpe_refine_batch without damping, then S = A^-1 written out:
 *   D0 = A_00 ; L10 = A_01 / D0 ; L20 = A_02 / D0 ; D1 = A_11 - L10*A_01 ; t = A_12 - L20*A_01 ; L21 = t / D1
 *   D2 = (A_22 - L20*A_02) - L21*t
 *   i0 = 1 / D0 ; i1 = 1 / D1 ; i2 = 1 / D2 ; m = L10*L21 - L20
 *   S22 = i2 ; S12 = -L21*i2 ; S02 = m*i2
 *   S11 = i1 - L21*S12 ; S01 = (-L10)*i1 + m*S12
 *   S00 = (i0 + (L10*L10)*i1) + m*S02
 * Outputs.  s2 = sigma_px*sigma_px ; cov_kl = s2 * S_kl ; sigma = sqrt((cov_00 + cov_11) + cov_22), metres.
 * Status per joint: no observing camera: 0.  Exactly one: MPE_POSECOV_FEW_VIEWS (A has rank 2; nothing is invented).  Two
 *   or more and a pose that is not finite, or pc_2 <= 0 (or NaN) in an observing camera: _BAD_POSE.  Otherwise a pivot D0,
 *   D1 or D2 that is not > 0, or an entry of cov or sigma that is not finite: _SINGULAR.  Otherwise _COMPUTED.  A joint
 *   that is not computed gets cov = 0, sigma = -1 and n_views as counted.
 * Gate.  With gate_m > 0 a COMPUTED joint whose sigma > gate_m takes _GATED as well (cov and sigma stay).  d_flags_out,
 *   when given, receives d_flags with the GATED joints cleared and every other entry copied; it needs joint_flags = 1, is
 *   [n_frames][pcap][J], and may be d_flags itself.  A joint that is not COMPUTED keeps its flag: the stage does not judge
 *   what it cannot measure.
 * Outputs per [n_frames][pcap][J]: d_cov [..][6] in the order (00, 01, 02, 11, 12, 22), d_sigma, d_status, d_n_views.
 * One launch, ordered on `stream`; neither synchronises nor allocates; n_frames == 0 does nothing.  MPE_ERR_INVALID for a
 * sigma_px that is not > 0 or not finite, a negative (or NaN) gate_m or huber_px, d_flags_out with joint_flags = 0,
 * n_frames other than the batch's or n_joints other than the context's. */
enum {
    MPE_POSECOV_COMPUTED = 1,
    MPE_POSECOV_FEW_VIEWS = 8,
    MPE_POSECOV_BAD_POSE = 16,
    MPE_POSECOV_SINGULAR = 32,
    MPE_POSECOV_GATED = 64
};
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t joint_mask;           /* bit j: joint j is measured                                     */
    float threshold;               /* 0.5, as for mpe_reproject_batch                                */
    double huber_px;               /* pixels, >= 0; 0: every weight is 1                             */
    double sigma_px;               /* pixels, > 0: the noise of a detection in x and in y            */
    double gate_m;                 /* metres, >= 0; 0: no gate                                       */
    const int32_t *d_persons;      /* [n_frames][pcap][V]                                            */
    const int32_t *d_n_persons;    /* [n_frames]                                                     */
    const void *d_poses;
    const uint8_t *d_flags;
    double *d_cov;                 /* [n_frames][pcap][J][6]                                         */
    double *d_sigma;               /* [n_frames][pcap][J]                                            */
    uint8_t *d_status, *d_n_views; /* [n_frames][pcap][J]                                            */
    uint8_t *d_flags_out;          /* [n_frames][pcap][J] or NULL                                    */
} mpe_posecov_args;
int mpe_posecov_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_posecov_args *a);

/* Calibration: the camera extrinsics refined from a recording's own poses -- the other half of bundle adjustment: the 3D
 * joints are held fixed and every camera is moved to the minimum of the reprojection cost of the joints it observed.  A
 * pass (mpe_calib_batch over every batch of the recording) reduces all observations into one 6 x 6 system per camera on the
 * device; mpe_calib_step solves the systems on the host (Levenberg-Marquardt per camera; the cameras are independent
 * because the points are fixed) and sets the extrinsics the next pass is taken at.  Alternated with mpe_triangulate_batch /
 * mpe_refine_batch under the new extrinsics this is a bundle adjustment of the rig; the global similarity gauge stays free
 * (hold one camera to keep the rig where it was).  The context's own calibration is never modified.
 * All binary64, every operation named below rounded on its own (nothing fused), quotients and roots correctly rounded;
 * harness/calibrate.py states the same in numpy: the sums agree bit for bit, and so does the step's delta.
 * State.  A trial extrinsic E[c] (3 x 4) per camera, cfg.P[c] at create; the 28 sums per camera of the pass so far.
 * One pass, per observation.  Camera c observes joint j of person p of frame f exactly when mpe_reproject_batch, given the
 *   same d_persons / d_n_persons / d_poses / d_flags / pose_f64 / joint_flags / joint_mask / threshold, would count
 *   d_res[f][p][c][j]; X = that joint widened to f64, x, y = that detection.  With T = E[c], kd and K as for
 *   mpe_refine_batch, the projection lines of mpe_refine_batch give pc_0..2, h0, h1, r, f, u_2, px, py, rx, ry, e.  Then
 *   a = (1/pc_2, 0, (-h0)/pc_2) ; b = (0, 1/pc_2, (-h1)/pc_2)                 the derivative by pc_k, k = 0..2
 *   fd, q_k, m_k, n_k, v_ik as for mpe_refine_batch from these a_k, b_k
 *   cx_k = (v_0k - px*v_2k) / u_2 ; cy_k = (v_1k - py*v_2k) / u_2
 *   the camera perturbed as pc + w x pc + tau, xi = (w_0, w_1, w_2, tau_0, tau_1, tau_2):
 *   Jx_0 = cx_2*pc_1 - cx_1*pc_2 ; Jx_1 = cx_0*pc_2 - cx_2*pc_0 ; Jx_2 = cx_1*pc_0 - cx_0*pc_1 ; Jx_{3+k} = cx_k
 *   Jy likewise from cy; the weight w and rho(e) as for mpe_refine_batch (Huber; huber_px = 0: plain least squares).
 *   An observation whose joint is not finite, for which pc_2 > 0 does not hold, or whose px or py is not finite is not
 *   summed and is counted in n_skipped[c].  Every other one adds 28 numbers to camera c (q = 0..27):
 *     A_kl += w*(Jx_k*Jx_l + Jy_k*Jy_l)   k <= l, row by row: (0,0) (0,1) .. (0,5) (1,1) .. (5,5)       q = 0..20
 *     g_k  += w*(Jx_k*rx + Jy_k*ry)                                                                  q = 21..26
 *     C    += rho(e)                                                                                 q = 27
 *   and 1 to n_obs[c].
 * Order.  Per frame, S_f[c][q] is the left fold from 0.0 of these terms over p increasing, then j increasing.  A call takes
 *   acc[c][q] = acc[c][q] + S_f[c][q] for its frames in increasing f -- every frame, whether its partial is zero or not --
 *   and calls count in the order made: the sums do not depend on how a recording is cut into batches, bit for bit.
 * mpe_calib_batch: two launches whatever the frame count, ordered on `stream`; neither synchronises nor allocates; n_frames
 *   == 0 does nothing.  MPE_ERR_INVALID as for mpe_refine_batch: n_frames other than the batch's, n_joints other than the
 *   context's, a negative (or NaN) huber_px.
 * mpe_calib_step synchronises `stream`, reads the sums, runs the rule below per camera (csrc/calib_solve.h: the order of
 *   every sum is written out there), stores the new trial extrinsics on the device and zeroes the sums.  Per camera the
 *   state keeps the accepted extrinsics E_a with their cost C_a and sums A_a, g_a, lambda (1e-3 at the start) and n_obs of
 *   the first pass.
 *   Held: bit c of hold_mask (MPE_CALIB_HELD), or n_obs < min_obs (MPE_CALIB_HELD | MPE_CALIB_FEW_OBS; min_obs >= 6, else
 *     MPE_ERR_INVALID).  A held camera has its sums and cost reported; its trial stays its accepted state.
 *   n_obs other than the first pass's, in any camera: MPE_ERR_INVALID ("the passes did not see the same data"); the sums are
 *     zeroed, nothing else changes.
 *   First pass: accepted.  Later passes: accepted iff C < C_a (strict; NaN rejects).  Accepted: E_a = the trial, C_a, A_a,
 *     g_a = the pass's, lambda = max(lambda / 10, 1e-12) (not after the first pass); if the step that led here had
 *     |w| < rot_tol and max |tau_k| < trans_tol the camera is MPE_CALIB_CONVERGED and stops.  Rejected: lambda = lambda * 10.
 *   Trial (after either): M = A_a + lambda*diag(A_a), M delta = -g_a by unpivoted LDL^T; a pivot that is not > 0 or a delta
 *     that is not finite multiplies lambda by 10 and retries, at most 8 times, then the camera is MPE_CALIB_STALLED and
 *     stops.  E_t = [exp(w) R_a | exp(w) t_a + tau], exp by Rodrigues' formula (series below |w| = 1e-8).
 *   A camera that stopped keeps trial = accepted; later passes leave it alone.  all_done: every camera is held or stopped.
 * mpe_calib_set_extrinsics: host E [V][12]; accepted = trial = E, the Levenberg-Marquardt state and the sums start afresh.
 * mpe_calib_reset: the same with cfg.P.  mpe_calib_get_extrinsics: host copies [V][12] of the accepted and the trial set
 * (either may be NULL).  mpe_calib_read: synchronises and returns the sums of the pass so far, [V][28], and the counts [V]
 * (any may be NULL).  One state serves one thread and one stream of work at a time. */
typedef struct mpe_calib_state mpe_calib_state;
enum {
    MPE_CALIB_HELD = 1,
    MPE_CALIB_FEW_OBS = 2,
    MPE_CALIB_CONVERGED = 4,
    MPE_CALIB_STALLED = 8,
    MPE_CALIB_ACCEPTED = 16,       /* the last step accepted the pass */
    MPE_CALIB_REJECTED = 32        /* the last step rejected it       */
};
#define MPE_CALIB_SUMS 28
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t joint_mask;           /* bit j: joint j is observed                                     */
    float threshold;               /* 0.5, as for mpe_reproject_batch                                */
    int32_t reserved;
    double huber_px;               /* pixels, >= 0; 0: plain least squares                           */
    const int32_t *d_persons;      /* [n_frames][pcap][V]                                            */
    const int32_t *d_n_persons;    /* [n_frames]                                                     */
    const void *d_poses;
    const uint8_t *d_flags;
} mpe_calib_args;
typedef struct {
    double rot_tol, trans_tol;     /* radians, metres                                                */
    int64_t min_obs;               /* >= 6                                                           */
    uint32_t hold_mask;            /* bit c: camera c is held                                        */
    int32_t reserved;
} mpe_calib_step_args;
typedef struct {
    int32_t status, passes;        /* MPE_CALIB_* bits; passes this camera's state has seen          */
    int64_t n_obs, n_skipped;      /* of the pass just read                                          */
    double cost_start, cost;       /* C_a after the first pass and now                               */
    double lambda;
    double last_rot, last_trans;   /* |w| and |tau| of the last trial built                          */
    double delta[6];               /* that trial's perturbation (w, tau)                             */
} mpe_calib_cam_report;
typedef struct {
    int32_t n_cameras, all_done;
    mpe_calib_cam_report cam[MPE_MAX_CAMERAS];
} mpe_calib_report;
int mpe_calib_create(mpe_ctx *ctx, mpe_calib_state **out);
int mpe_calib_destroy(mpe_ctx *ctx, mpe_calib_state *st);
int mpe_calib_reset(mpe_ctx *ctx, void *stream, mpe_calib_state *st);
int mpe_calib_set_extrinsics(mpe_ctx *ctx, void *stream, mpe_calib_state *st, const double *E);
int mpe_calib_get_extrinsics(mpe_ctx *ctx, const mpe_calib_state *st, double *accepted, double *trial);
int mpe_calib_batch(mpe_ctx *ctx, void *stream, mpe_calib_state *st, const mpe_batch *b, const mpe_calib_args *a);
int mpe_calib_read(mpe_ctx *ctx, void *stream, mpe_calib_state *st, double *sums, int64_t *n_obs, int64_t *n_skipped);
int mpe_calib_step(mpe_ctx *ctx, void *stream, mpe_calib_state *st, const mpe_calib_step_args *a, mpe_calib_report *report);
int mpe_calib_launches(mpe_ctx *ctx, const mpe_calib_state *st, int64_t *n);

/* Camera fit: the intrinsics and the radial lens terms of every camera fitted together with its extrinsics from a
 * recording's own poses -- mpe_calib_* with seven more unknowns per camera.  The 3D joints are held fixed; a pass
 * (mpe_camfit_batch over every batch of the recording) reduces all observations into one 13 x 13 system per camera on the
 * device, mpe_camfit_step solves the systems on the host.  The context's own calibration is never modified.  All binary64,
 * every operation named below rounded on its own (nothing fused); harness/camfit.py states the same in numpy: the sums
 * agree bit for bit, and so does the step.
 * Unknowns, per camera, in this order: 0-2 w, 3-5 tau (the rigid perturbation pc + w x pc + tau, exactly mpe_calib_batch's),
 *   6 fx, 7 fy, 8 cx, 9 cy, 10 kd0, 11 kd1, 12 kd2.  The model is that of mpe_refine_batch as it is: the tangential terms
 *   dist[2], dist[3] are not read, are carried through untouched and are not unknowns.  K has the form
 *   [[fx,0,cx],[0,fy,cy],[0,0,1]]; a context whose K has another form is refused by mpe_camfit_create (MPE_ERR_INVALID).
 * Trial set, per camera: extrinsics [12] f64, (fx, fy, cx, cy) held as FLOAT32, dist[5] f64.  K is float32 because the
 *   context, every kernel and every caller carry it that way: the step rounds (double)fx + delta to float before the next
 *   pass, so the cost a pass reports is the cost at exactly the numbers a new context will evaluate.
 * One pass, per observation.  Every observation mpe_calib_batch would count is counted: the selection, the finite test,
 *   pc_2 > 0 before any quotient, the skip rule, the weight w and rho(e) are the same, taken at the trial set (T = the trial
 *   extrinsics, kd = the trial dist[0], dist[1], dist[4], K = the trial numbers widened).  Jx_0..5, Jy_0..5 are
 *   mpe_calib_batch's lines with the trial K and dist in them.  With d0 = h0*f, d1 = h1*f:
 *     Jx_6 = d0 ; Jy_6 = 0       Jx_7 = 0 ; Jy_7 = d1       Jx_8 = 1 ; Jy_8 = 0       Jx_9 = 0 ; Jy_9 = 1
 *     Jx_{10+i} = (fx*h0)*r^(i+1) ; Jy_{10+i} = (fy*h1)*r^(i+1),  i = 0..2, the powers taken as r, r*r, (r*r)*r
 *   Every summed observation adds MPE_CAMFIT_SUMS = 105 numbers to its camera, every one of the one form
 *   w*(a_k*a_l + b_k*b_l) -- the structural zeros are computed like everything else:
 *     A_kl += w*(Jx_k*Jx_l + Jy_k*Jy_l)   k <= l, row by row: (0,0) (0,1) .. (0,12) (1,1) .. (12,12)    q = 0..90
 *     g_k  += w*(Jx_k*rx + Jy_k*ry)                                                                  q = 91..103
 *     C    += rho(e)                                                                                 q = 104
 *   and 1 to n_obs[c]; a skipped one adds 1 to n_skipped[c].
 * Order: mpe_calib_batch's.  Per frame the left fold from 0.0 over p, then j; then the frames of a call in increasing f,
 *   every frame whether its partial is zero or not; then calls in the order made.  Any cut of a recording into batches
 *   gives the same bits.
 * mpe_camfit_batch: two launches whatever the frame count, ordered on `stream`; neither synchronises nor allocates;
 *   n_frames == 0 does nothing.  It takes mpe_calib_args and refuses what mpe_calib_batch refuses.
 * mpe_camfit_step: mpe_calib_step's rule per camera (csrc/camfit_solve.h writes out every sum), with these additions.
 *   free_mask names the groups that are unknowns: MPE_CAMFIT_POSE (0-5), _FOCAL (6, 7), _CENTRE (8, 9), _K1 (10), _K2 (11),
 *     _K3 (12); zero or a bit outside these: MPE_ERR_INVALID.  The row and column of a held unknown are left out of the
 *     solve and its delta is 0.  The solve is the unpivoted LDL^T of mpe_calib_step over the free unknowns in ascending
 *     index, M = A + lambda*diag(A); with only MPE_CAMFIT_POSE free it performs the same operations in the same order.
 *   Compose: the extrinsics as in mpe_calib_step from delta_0..5 when MPE_CAMFIT_POSE is free (else copied); for a free
 *     intrinsic fx_t = (float)((double)fx_a + delta_6), fy, cx, cy likewise; for a free lens term kd_t = kd_a + delta.
 *     A trial whose fx or fy is not finite or is <= 0 counts as a failed solve (lambda * 10, at most 8 retries, then
 *     MPE_CALIB_STALLED).
 *   Accepted iff the cost fell (strict; the first pass is accepted).  MPE_CALIB_CONVERGED when the accepted step had
 *     |w| < rot_tol, max |tau_k| < trans_tol, max |delta_6..9| < pix_tol (pixels) and max |delta_10..12| < lens_tol -- or
 *     when the trial just built equals the accepted set bit for bit in every free unknown: the float rounding left
 *     nothing to move.
 *   min_obs >= max(6, the number of free unknowns), else MPE_ERR_INVALID; hold_mask, MPE_CALIB_FEW_OBS, the n_obs check
 *     ("the passes did not see the same data") and the status bits (MPE_CALIB_*) are mpe_calib_step's.
 * mpe_camfit_set_cameras: host E [V][12], k [V][4] float (fx, fy, cx, cy), dist [V][5]; accepted = trial = these, the
 *   Levenberg-Marquardt state and the sums start afresh; a value that is not finite, or fx or fy <= 0: MPE_ERR_INVALID.
 *   mpe_camfit_reset: the same with the context's own.  mpe_camfit_get_cameras: host copies of the accepted and the trial
 *   set (any pointer may be NULL).  mpe_camfit_read: synchronises and returns the sums of the pass so far, [V][105], and the
 *   counts [V] (any may be NULL).  One state serves one thread and one stream of work at a time. */
typedef struct mpe_camfit_state mpe_camfit_state;
enum {
    MPE_CAMFIT_POSE = 1,
    MPE_CAMFIT_FOCAL = 2,
    MPE_CAMFIT_CENTRE = 4,
    MPE_CAMFIT_K1 = 8,
    MPE_CAMFIT_K2 = 16,
    MPE_CAMFIT_K3 = 32
};
#define MPE_CAMFIT_UNKNOWNS 13
#define MPE_CAMFIT_SUMS 105
typedef struct {
    double rot_tol, trans_tol;     /* radians, metres                                                */
    double pix_tol, lens_tol;      /* pixels (fx, fy, cx, cy); the three kd                          */
    int64_t min_obs;               /* >= max(6, free unknowns)                                       */
    uint32_t hold_mask;            /* bit c: camera c is held                                        */
    uint32_t free_mask;            /* MPE_CAMFIT_* bits: the groups that are unknowns                */
} mpe_camfit_step_args;
typedef struct {
    int32_t status, passes;        /* MPE_CALIB_* bits; passes this camera's state has seen          */
    int64_t n_obs, n_skipped;      /* of the pass just read                                          */
    double cost_start, cost;       /* C_a after the first pass and now                               */
    double lambda;
    double last_rot, last_trans;   /* |w| and |tau| of the last trial built                          */
    double last_pix, last_lens;    /* max |delta_6..9| and max |delta_10..12| of that trial          */
    double delta[13];              /* that trial's step, in the order of the unknowns                */
} mpe_camfit_cam_report;
typedef struct {
    int32_t n_cameras, all_done;
    mpe_camfit_cam_report cam[MPE_MAX_CAMERAS];
} mpe_camfit_report;
int mpe_camfit_create(mpe_ctx *ctx, mpe_camfit_state **out);
int mpe_camfit_destroy(mpe_ctx *ctx, mpe_camfit_state *st);
int mpe_camfit_reset(mpe_ctx *ctx, void *stream, mpe_camfit_state *st);
int mpe_camfit_set_cameras(mpe_ctx *ctx, void *stream, mpe_camfit_state *st, const double *E, const float *k, const double *dist);
int mpe_camfit_get_cameras(mpe_ctx *ctx, const mpe_camfit_state *st, double *E_accepted, float *k_accepted, double *dist_accepted,
                           double *E_trial, float *k_trial, double *dist_trial);
int mpe_camfit_batch(mpe_ctx *ctx, void *stream, mpe_camfit_state *st, const mpe_batch *b, const mpe_calib_args *a);
int mpe_camfit_read(mpe_ctx *ctx, void *stream, mpe_camfit_state *st, double *sums, int64_t *n_obs, int64_t *n_skipped);
int mpe_camfit_step(mpe_ctx *ctx, void *stream, mpe_camfit_state *st, const mpe_camfit_step_args *a, mpe_camfit_report *report);
int mpe_camfit_launches(mpe_ctx *ctx, const mpe_camfit_state *st, int64_t *n);

/* Time lags: how many frames each camera runs ahead of or behind the poses of a recording, estimated from the recording
 * itself -- the time half of the rig adjustment of which mpe_calib_* is the space half.  The 3D poses of the whole
 * sequence, with track ids, are a table; every detection of a camera is compared with the projection of its track's pose
 * at the table frames f + lag for a grid of lags, linearly interpolated between frames, and the reprojection cost of every
 * grid entry is summed per camera.  The entry of least mean cost, refined by a parabola through its neighbours, is the
 * camera's lag relative to the poses' own time (the common shift of all cameras cannot be seen from poses the cameras made
 * themselves).  All binary64, every operation named below rounded on its own (nothing fused), quotients and roots
 * correctly rounded; harness/lag.py states the same in numpy: the sums agree bit for bit, and so does the estimate.
 * Configuration, fixed at create: pcap, n_joints (the context's), window W in 0 .. MPE_LAG_MAX_WINDOW, sub in 1 ..
 *   MPE_LAG_MAX_SUB, pose_f64, joint_flags, max_frames (frames per call, at most: the workspace of the per-frame partials).
 *   The grid has K = 2*W*sub + 1 entries, i = 0 .. K-1:
 *   k = i - W*sub ; s = floor(k / sub) (towards -inf) ; r = k - s*sub ; alpha = (double)r / (double)sub
 *   and the lag of entry i is (double)k / (double)sub frames.  Sign: a camera with lag > 0 shows, in its picture of frame f,
 *   the world at time f + lag.
 * The table, given at every call (no frame is carried from call to call, which is what makes the sums independent of the
 *   chunking): d_poses [n_table][pcap][J][3], d_flags, d_n_persons [n_table], d_tid [n_table][pcap], rows as every sequence
 *   stage reads them.  A call takes a batch -- the detections of the table frames frame_start .. frame_start + n_frames - 1
 *   --, d_persons [n_frames][pcap][V] for those frames, joint_mask, threshold and huber_px.
 * Row of a track.  For t >= 0 and a table frame g, the row of (g, t) is the lowest p below the rows of frame g (n_persons
 *   held within 0 .. pcap) with tid[g][p] == t and, with per-row flags, the flag set; there is none when g is outside
 *   0 .. n_table - 1.
 * Observation (f, p, c, j), f a table frame of the call: where mpe_reproject_batch would count d_res[f][p][c][j] given the
 *   batch, these persons, the table's n_persons and flags of frame f and the same mask and threshold.  It is supported when
 *   t = tid[f][p] >= 0 and for every g in f-W .. f+W the row of (g, t) exists, joint j of it is flagged and its three
 *   coordinates are finite (f-W .. f+W is exactly what the grid touches: its last entry has r = 0).  Supported observations
 *   count in n_support[c], the others in n_unsupported[c]; the support is the same for every k, so the K costs of a camera
 *   are sums over the same observations.
 * Term, per supported observation and k:
 *   X_a = joint j of the row of (f+s, t), widened to f64
 *   r = 0: X = X_a.  Otherwise X_b = joint j of the row of (f+s+1, t) and X_i = X_a,i + alpha*(X_b,i - X_a,i)
 *   X projected with camera c of the context (cfg.P, kd, K and the projection lines of mpe_refine_batch)
 *   if pc_2 > 0 does not hold, or px or py is not finite: n_skipped[c][k] += 1, nothing is summed
 *   otherwise rx = px - x ; ry = py - y ; e = sqrt(rx*rx + ry*ry) ; the term is rho(e) as for mpe_refine_batch (Huber;
 *   huber_px = 0: the plain square) and n_obs[c][k] += 1.
 * Order.  Per frame, S_f[c][k] is the left fold from 0.0 of the terms over p increasing, then j increasing.  A call takes
 *   cost[c][k] = cost[c][k] + S_f[c][k] for its frames in increasing f -- every frame, whether its partial is zero or not --
 *   and calls count in the order made: with the same table the sums do not depend on how a recording is cut into batches,
 *   bit for bit.
 * mpe_lag_batch: two launches whatever the frame count, ordered on `stream`; neither synchronises nor allocates; n_frames
 *   == 0 does nothing.  MPE_ERR_INVALID: n_frames other than the batch's, n_joints other than the context's, pcap, pose_f64
 *   or joint_flags other than the state's, frame_start < 0, frame_start + n_frames > n_table, n_frames > max_frames, a
 *   negative (or NaN) huber_px, a NULL array.  mpe_lag_create: MPE_ERR_INVALID for a window or sub out of range, pcap < 1,
 *   max_frames < 1, n_joints other than the context's; MPE_ERR_CAPACITY for pcap > MPE_TRACK_MAX_PERSONS.
 * mpe_lag_reset zeroes the sums and the counts (stream-ordered memsets).  mpe_lag_read synchronises `stream` and returns
 *   cost [V][K], n_obs [V][K], n_skipped [V][K], n_support [V], n_unsupported [V] (any may be NULL).
 * mpe_lag_estimate does the same read, then per camera (csrc/lag_pick.h):
 *   entry i is valid when n_obs[c][i] >= min_obs (min_obs >= 1, else MPE_ERR_INVALID) ; m_i = cost / (double)n_obs
 *   no valid entry: MPE_LAG_FEW_OBS, k_best = 0, both lags 0, both costs NaN
 *   i* = the lowest index of the least m_i among the valid entries (a NaN is never least; with nothing but NaN the lowest
 *   valid index)
 *   i* = 0, i* = K-1 or an invalid neighbour: MPE_LAG_EDGE, refined = grid
 *   otherwise den = (m_{i*-1} - m_{i*}) + (m_{i*+1} - m_{i*}) ; den > 0: off = (0.5*(m_{i*-1} - m_{i*+1})) / den, held within
 *   -0.5 .. 0.5 ; else, or when off is a NaN, off = 0 and MPE_LAG_FLAT
 *   k* = i* - W*sub ; lag_grid = (double)k* / (double)sub ; lag_refined = ((double)k* + off) / (double)sub
 *   cost_best = m_{i*} ; cost_zero = m at k = 0, NaN when that entry is invalid ; n_obs = that of i*.
 * One state serves one thread and one stream of work at a time. */
typedef struct mpe_lag_state mpe_lag_state;
enum {
    MPE_LAG_FEW_OBS = 1,
    MPE_LAG_EDGE = 2,
    MPE_LAG_FLAT = 4
};
#define MPE_LAG_MAX_WINDOW 8
#define MPE_LAG_MAX_SUB 8
#define MPE_LAG_MAX_GRID (2 * MPE_LAG_MAX_WINDOW * MPE_LAG_MAX_SUB + 1)
typedef struct {
    int32_t pcap, n_joints;
    int32_t window, sub;           /* W and the grid entries per frame                               */
    int32_t pose_f64;              /* 0: table poses f32; 1: f64                                     */
    int32_t joint_flags;           /* 0: table flags [n_table][pcap] u8; 1: [n_table][pcap][J]       */
    int32_t max_frames;            /* frames per mpe_lag_batch, at most                              */
    int32_t reserved;
} mpe_lag_config;
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64, joint_flags; /* as the state was made                                          */
    int32_t frame_start, n_table;  /* the call's frames are frame_start .. + n_frames - 1 of n_table */
    uint32_t joint_mask;           /* bit j: joint j is observed                                     */
    float threshold;               /* 0.5, as for mpe_reproject_batch                                */
    int32_t reserved;
    double huber_px;               /* pixels, >= 0; 0: the plain square                              */
    const int32_t *d_persons;      /* [n_frames][pcap][V], of the call's frames                      */
    const void *d_poses;           /* [n_table][pcap][J][3]                                          */
    const uint8_t *d_flags;        /* [n_table][pcap] or [n_table][pcap][J]                          */
    const int32_t *d_n_persons;    /* [n_table]                                                      */
    const int32_t *d_tid;          /* [n_table][pcap]                                                */
} mpe_lag_args;
typedef struct {
    int32_t status, k_best;        /* MPE_LAG_* bits; k* (signed, in grid steps)                     */
    double lag_grid, lag_refined;  /* frames                                                         */
    double cost_best, cost_zero;   /* mean cost per observation, px^2 (Huber: its units)             */
    int64_t n_obs;                 /* of entry i*                                                    */
    int64_t n_support, n_unsupported;
} mpe_lag_cam_report;
typedef struct {
    int32_t n_cameras, n_grid;
    mpe_lag_cam_report cam[MPE_MAX_CAMERAS];
} mpe_lag_report;
int mpe_lag_create(mpe_ctx *ctx, const mpe_lag_config *cfg, mpe_lag_state **out);
int mpe_lag_reset(mpe_ctx *ctx, void *stream, mpe_lag_state *st);
int mpe_lag_destroy(mpe_ctx *ctx, mpe_lag_state *st);
int mpe_lag_batch(mpe_ctx *ctx, void *stream, mpe_lag_state *st, const mpe_batch *b, const mpe_lag_args *a);
int mpe_lag_launches(mpe_ctx *ctx, const mpe_lag_state *st, int64_t *n);
int mpe_lag_read(mpe_ctx *ctx, void *stream, mpe_lag_state *st, double *cost, int64_t *n_obs, int64_t *n_skipped, int64_t *n_support,
                 int64_t *n_unsupported);
int mpe_lag_estimate(mpe_ctx *ctx, void *stream, mpe_lag_state *st, int32_t min_obs, mpe_lag_report *report);

/* Time-aware refinement: mpe_refine_batch with every camera looking at the joint where the joint's track says it was at that
 * camera's time -- what corrects the sub-frame lags mpe_lag_estimate reports.  A camera that lags by L frames saw, in its
 * picture of frame f, the world at f + L; the track of the joint in the table gives how far the joint moved between f and
 * f + L, and camera c projects the unknown point displaced by that much.  The displacements are taken from the table once
 * and are constants of the call: the problem keeps its three unknowns per joint.  Stateless.  All binary64, every operation
 * named below rounded on its own (nothing fused); harness/refine_timed.py states the same in numpy, and the two agree bit
 * for bit.
 * Inputs: everything mpe_refine_batch takes; the table of mpe_lag_batch, given at every call (d_poses [n_table][pcap][J][3],
 *   d_flags, d_n_persons [n_table], d_tid [n_table][pcap], frame_start, n_table: the batch holds the detections of the table
 *   frames frame_start .. frame_start + n_frames - 1 and d_persons [n_frames][pcap][V] their rows); and lag[c], frames,
 *   c < V, with the sign the lag report has: lag > 0 means camera c's picture of frame f shows the world at f + lag.
 * Per camera c, with L = lag[c]: s = floor(L) ; alpha = L - (double)s (one subtraction; exact for L >= 0 and for every
 *   multiple of 2^-k frames within the window; 0 <= alpha <= 1).
 * Start.  The start point of joint (f, p, j) is joint j of row p of table frame F = frame_start + f.  The observing cameras
 *   are those of mpe_refine_batch given the batch, d_persons, and the table's n_persons and flags of frame F.
 * Timed cameras.  With t = tid[F][p] and the row of a track as mpe_lag_batch has it (the lowest row of that id below the
 *   frame's rows, with per-row flags the flag set; none outside 0 .. n_table - 1), an observing camera with L != 0 is timed
 *   for joint j when t >= 0 and the rows of (F, t), (F+s, t) and -- when alpha != 0 -- (F+s+1, t) exist and joint j of each
 *   is flagged (per-joint flags; a per-row flag stands for every joint) and has three finite coordinates.  Then, with X_f,
 *   X_a, X_b joint j of those rows widened to f64:
 *   alpha == 0: X_l = X_a.  Otherwise X_l,i = X_a,i + alpha*(X_b,i - X_a,i)                         i = 0..2
 *   d_c,i = X_l,i - X_f,i
 *   A camera with L == 0, or one that is not timed (at a track's or the table's ends, say: nothing is extrapolated), has no
 *   offset.  d_n_timed = the number of observing cameras that are timed, whether the joint is solved or not.
 * Solve.  Cost, Jacobian, LM step, acceptance, statuses and outputs are those of mpe_refine_batch, except that wherever
 *   camera c projects a point X (the start, the iterate, the trial) a timed camera projects (X0 + d_c,0, X1 + d_c,1,
 *   X2 + d_c,2): pc_2 > 0 is tested there and the Jacobian is taken there (the offset is a constant, so it is the
 *   Jacobian by X).  A camera without offset projects X itself, with no addition: with every lag 0 the seven shared
 *   outputs are the bits of mpe_refine_batch given the call's frames of the table.
 * The offsets come from the input table, never from d_poses_out, so the result does not depend on how a recording is cut
 *   into calls.  d_poses_out is [n_frames][pcap][J][3] and must not overlap the table (other frames' workgroups read their
 *   neighbours from it).
 * One launch, ordered on `stream`; neither synchronises nor allocates; n_frames == 0 does nothing.  MPE_ERR_INVALID for
 *   what mpe_refine_batch and mpe_lag_batch refuse on the arguments they share (max_iters, step_tol, huber_px, n_frames
 *   other than the batch's, n_joints other than the context's, frame_start < 0, frame_start + n_frames > n_table, a NULL
 *   array), for a lag[c], c < V, that is not finite or exceeds MPE_LAG_MAX_WINDOW in magnitude, and for a d_poses_out whose
 *   bytes overlap the table's poses; MPE_ERR_CAPACITY for more than 2^23 frames.
 * Not done here: the DLT and the MLP stay untimed, as do mpe_calib_* and mpe_body_refine_batch; velocity is not an unknown;
 *   no offset is extrapolated beyond a track's ends; wire timestamps are not read. */
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64, joint_flags; /* of the table: 0 / 1 as for mpe_lag_batch                       */
    int32_t frame_start, n_table;  /* the call's frames are frame_start .. + n_frames - 1 of n_table */
    uint32_t joint_mask;           /* bit j: joint j is refined                                      */
    float threshold;               /* 0.5, as for mpe_reproject_batch                                */
    int32_t max_iters;             /* 1 .. MPE_REFINE_MAX_ITERS                                      */
    double step_tol;               /* metres, >= 0                                                   */
    double huber_px;               /* pixels, >= 0; 0: plain least squares                           */
    double lag[MPE_MAX_CAMERAS];   /* frames, by camera slot; |lag| <= MPE_LAG_MAX_WINDOW            */
    const int32_t *d_persons;      /* [n_frames][pcap][V], of the call's frames                      */
    const void *d_poses;           /* [n_table][pcap][J][3]                                          */
    const uint8_t *d_flags;        /* [n_table][pcap] or [n_table][pcap][J]                          */
    const int32_t *d_n_persons;    /* [n_table]                                                      */
    const int32_t *d_tid;          /* [n_table][pcap]                                                */
    void *d_poses_out;             /* [n_frames][pcap][J][3], the type of d_poses                    */
    uint8_t *d_status;             /* [n_frames][pcap][J]                                            */
    double *d_cost0, *d_cost1;     /* [n_frames][pcap][J]                                            */
    uint8_t *d_iters, *d_n_views;  /* [n_frames][pcap][J]                                            */
    uint8_t *d_n_timed;            /* [n_frames][pcap][J]                                            */
} mpe_refine_timed_args;
int mpe_refine_timed_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_refine_timed_args *a);

/* Geometric cross-view matching: a score per edge-node (h1,h2) that needs the calibration only -- how closely the
 * back-projected rays of the two 2D skeletons meet in space (the standard multi-view baseline; no GAT, no MLP weights).
 * All binary64, every operation named below rounded on its own (nothing fused), quotients and roots correctly rounded;
 * only the score is rounded to float.  harness/geometric.py states the same in numpy, and the two agree bit for bit.
 * The edge-nodes are the batch's: the implicit list or mpe_batch::d_en_pair (checked and copied as for every other stage).
 * Rays.  Head h of camera c, joint j, pixel (u, v) = d_xy[h][j]; (x, y) = the five-iteration undistortion of
 *   mpe_triangulate_batch (csrc/dlt_common.h: undistort_point, with fx, fy, cx, cy = (double) cfg.K[c] and k1, k2, p1, p2,
 *   k3 = cfg.dist[c]), which leaves up to 1.5e-2 px at the image border, followed by two Newton steps on the same lens
 *   model (a ray then passes within 1e-6 px of its pixel).  With xt = (u - cx) * (1 / fx), yt = (v - cy) * (1 / fy), twice:
 *   r = x*x + y*y ; f = 1 + ((k3*r + k2)*r + k1)*r ; fd = ((3*k3)*r + 2*k2)*r + k1 ; tx = 2*x ; ty = 2*y
 *   ex = ((x*f + p1*(tx*y)) + p2*(r + tx*x)) - xt ; ey = ((y*f + p1*(r + ty*y)) + p2*(tx*y)) - yt
 *   a = ((f + (tx*x)*fd) + p1*ty) + (3*p2)*tx ; b = ((tx*y)*fd + p1*tx) + p2*ty ; d = ((f + (ty*y)*fd) + (3*p1)*ty) + p2*tx
 *   det = a*d - b*b ; x, y = x - (d*ex - b*ey) / det, y - (a*ey - b*ex) / det          (both from the old x, y)
 *   With T = cfg.P[c] as stored (root -> camera; R = T[:, 0:3], t = T[:, 3]):
 *   q_k = (T[0][k]*x + T[1][k]*y) + T[2][k]                                 k = 0..2
 *   n   = sqrt((q_0*q_0 + q_1*q_1) + q_2*q_2) ; r_k = q_k / n              (unit direction, world frame)
 *   o_k = -((T[0][k]*T[0][3] + T[1][k]*T[1][3]) + T[2][k]*T[2][3])         (camera centre, world frame)
 * Votes.  Joint j of edge-node (h1,h2) votes when the two heads are in different cameras, bit j is set in both
 *   d_joint_mask words and in joint_mask (0 = every joint), and d_vp[h][j][0] >= min_conf for both heads.
 * Distance of a voting joint, (o1, r1) the ray of h1 and (o2, r2) that of h2:
 *   w_k = o1_k - o2_k ; b = (r1_0*r2_0 + r1_1*r2_1) + r1_2*r2_2 ; d and e likewise from (r1, w) and (r2, w)
 *   den = 1 - b*b ; den < 1e-12 (parallel rays): t1 = 0, t2 = e ; otherwise t1 = (b*e - d) / den, t2 = (e - b*d) / den
 *   a t1 or t2 that is < 0 is replaced by 0 (rays that meet behind a camera are penalised, not rewarded)
 *   g_k = (o1_k + t1*r1_k) - (o2_k + t2*r2_k) ; dist = sqrt((g_0*g_0 + g_1*g_1) + g_2*g_2)
 *   with clip_m > 0, a dist > clip_m is replaced by clip_m.
 * Score.  n = the number of voting joints, mean = (the left-fold sum of dist over the voting joints in increasing j,
 *   from 0.0) / n, score = (float)(sigma_m / (sigma_m + mean)); 0.0f when n < min_joints (and so whenever the heads share
 *   a camera).  With the clustering threshold 0.5, two skeletons link when their rays pass within sigma_m on average.
 * Outputs per edge-node: d_scores; optionally d_n_votes = n and d_mean = mean (-1 where n == 0).  A frame beyond
 *   max_heads_per_frame (or, with d_en_pair, beyond the per-frame edge-node limit) gets zeros (d_mean -1) and the sticky
 *   status bit mpe_sync_status reports, as everywhere.
 * mpe_geom_scores_batch: the topology launch mpe_cluster_batch also makes, then one launch (one workgroup per frame: the
 *   unit rays of every head once, in LDS, or in a table of the context when max_heads_per_frame * (3 n_joints + 1) doubles
 *   exceed 48 KiB -- same bits either way).  mpe_geom_match_batch: the same, then the clustering of mpe_cluster_batch on the
 *   scores (d_scores may be NULL: the scores then stay in context scratch).  Both are ordered on `stream`, neither
 *   synchronises nor allocates, n_frames == 0 does nothing, both work on a context without weights, and neither reads or
 *   writes anything mpe_match_batch leaves behind for mpe_mlp3d_batch.  MPE_ERR_INVALID for sigma_m <= 0, clip_m < 0
 *   (or NaN), min_joints outside 1..n_joints, a negative or NaN min_conf, or a NULL output. */
typedef struct {
    double sigma_m;                /* metres, > 0                                                    */
    double clip_m;                 /* metres, >= 0; 0: no clip                                       */
    int32_t min_joints;            /* 1 .. n_joints                                                  */
    uint32_t joint_mask;           /* bit j: joint j may vote; 0: every joint                        */
    float min_conf;                /* votes need values[3] >= this in both heads; 0: all             */
    float *d_scores;               /* [n_edge_nodes]                                                 */
    uint8_t *d_n_votes;            /* [n_edge_nodes] or NULL                                         */
    double *d_mean;                /* [n_edge_nodes] or NULL: mean distance, -1 where n_votes == 0   */
} mpe_geom_args;
int mpe_geom_scores_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_geom_args *a);
int mpe_geom_match_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_geom_args *a,
                         int32_t *d_persons, int32_t *d_n_persons);

/* Regrouping: the person proposals repaired by reprojection consistency -- the verification pass of multi-view association,
 * between the matching stage and the refinement.  Once a row has a 3D pose, projecting the pose into a camera says which
 * skeleton of that camera belongs to it: the stage computes the cost of EVERY head of a frame against EVERY person of the
 * frame, releases the heads a row should not hold (a wrong person's skeleton, two persons exchanged in a camera) and
 * attaches free heads to rows that lack their camera (a skeleton the clustering left out).  All arithmetic is binary64,
 * every operation named below rounded on its own (nothing fused), quotients and roots correctly rounded; harness/regroup.py
 * states the same in numpy, and the two agree bit for bit.
 * Inputs.  The batch; d_persons / d_n_persons / d_poses / d_flags / pose_f64 / joint_flags / joint_mask / threshold exactly as
 *   mpe_refine_batch takes them; gate_px > 0, clip_px >= 0, min_joints in 1..n_joints, flags (MPE_REGROUP_RELEASE |
 *   MPE_REGROUP_ATTACH, at least one).  The rows of a frame are its persons p < min(d_n_persons[f], pcap); entries < 0 are
 *   open.  Person p has a pose when joint_flags == 1 or d_flags[f][p] != 0.
 * Cost of head h (camera c = d_head_cam[h]) against person p of the same frame, for every p that has a pose and every head of
 *   the frame.  Joint j counts when bit j is set in joint_mask and in d_joint_mask[h]; d_vp[h][j][0] > threshold (strict);
 *   with joint_flags == 1, d_flags[f][p][j] != 0; the pose's joint j, widened to f64, is finite; pc_2 > 0 for it in camera c;
 *   and e is finite, where e is the pixel distance of mpe_refine_batch's projection lines (T, kd and K as stored there)
 *   from the detection (x, y) = d_xy[h][j].  With clip_px > 0, an e > clip_px is replaced by clip_px.
 *   cost = (the left-fold sum of e over the counting joints in increasing j, from 0.0) / n, n = their number.  With
 *   n < min_joints (or a head whose camera index is outside 0..V-1, or a cost that is not finite) the pair is UNSCORED: -1.
 *   A scored cost is finite and >= 0.  The table does not depend on d_persons.
 * Bad rows.  An entry e >= 0 in column c of a row is bad when e >= the frame's head count, when head e is not of camera c, or
 *   when another entry of the frame's rows names e too.  Any bad entry makes the frame MPE_REGROUP_BAD_ROWS.  A frame with
 *   more heads than max_heads_per_frame is MPE_REGROUP_OVER_CAP (its rows are not looked at) and sets the sticky status bit
 *   mpe_sync_status reports, as everywhere.  Either frame is COPIED THROUGH: its rows unchanged, d_change 0, d_n_views
 *   counted from the rows as they are, d_counts 0; its cost table is still written.
 * Release (MPE_REGROUP_RELEASE).  For every person with a pose and every camera c whose entry h is >= 0: if (p, h) is scored
 *   and cost < gate_px does not hold, the entry becomes -1 and h is free.  Unscored pairs are kept (nothing can be said
 *   about them); persons without a pose are left alone, and their heads are not free.
 * Attach (MPE_REGROUP_ATTACH), after the release, per camera c, independently of the other cameras.  Heads: those of camera
 *   c that no row of the frame names now (released ones included).  Persons: those with a pose whose entry for c is open
 *   now.  A pair is linkable when it is scored and cost < gate_px.  The linkable pair of least cost -- ties to the lowest
 *   head id, then the lowest p -- is written into the row and both leave; repeated until no linkable pair is left (the
 *   greedy rule of mpe_track_batch).  A released head cannot return to the row that released it.
 * d_n_persons is not changed and rows are not compacted: row p of the output still belongs to row p of d_poses.  A row may
 *   end with fewer heads than min_views, or with none: the 3D stages decide from a row's heads whether it yields a pose.
 * Outputs.  d_persons_out [n_frames][pcap][V] (may be d_persons itself); d_change [n_frames][pcap][V]: 0 kept, 1 released,
 *   2 attached, 3 released and another head attached; d_n_views [n_frames][pcap]: entries >= 0 of the row afterwards, 0 for
 *   p >= n_persons; d_cost [n_heads][pcap] f64: -1 for unscored pairs, for p >= n_persons and for persons without a pose
 *   (required: the context holds no table of this size; it may be NULL only when the batch has no heads, where the table
 *   is empty and nothing is written to it); d_counts [n_frames][4]: entries released, entries attached, heads
 *   named by no row afterwards, persons with a pose and fewer than cfg.min_views heads afterwards; d_status [n_frames].
 * Limits.  The stage does not merge two rows that hold the same body and does not found persons from the heads left free
 *   (mpe_consolidate_batch, below, does both), and
 *   does not update the pose: the caller alternates 3D stage, regroup, 3D stage again on the new rows.  joint_mask must
 *   name only joints whose pose is filled in: mpe_triangulate_batch without flags bit 0 flags the joints outside
 *   used_joints as emitted and leaves them at the origin, so after it the mask is cfg.used_joint_mask.
 * One launch (one workgroup per frame), ordered on `stream`; keeps no state, neither synchronises nor allocates; n_frames == 0
 *   does nothing; works on a context without weights and neither reads nor writes anything mpe_match_batch leaves behind
 *   for mpe_mlp3d_batch.  MPE_ERR_INVALID for a gate_px that is not > 0 (or NaN), a negative (or NaN) clip_px, min_joints
 *   outside 1..n_joints, flags 0 or with unknown bits, a NULL output, n_frames other than the batch's, n_joints other
 *   than the context's, pcap < 1 or a pose_f64 / joint_flags other than 0 or 1; MPE_ERR_CAPACITY for
 *   pcap > MPE_REGROUP_MAX_PERSONS. */
enum {
    MPE_REGROUP_BAD_ROWS = 1,
    MPE_REGROUP_OVER_CAP = 2
};
enum {
    MPE_REGROUP_RELEASE = 1,
    MPE_REGROUP_ATTACH = 2
};
#define MPE_REGROUP_MAX_PERSONS 128
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t joint_mask;           /* bit j: joint j may count                                       */
    float threshold;               /* 0.5, as for mpe_reproject_batch                                */
    int32_t min_joints;            /* 1 .. n_joints: counting joints a scored pair needs             */
    double gate_px;                /* pixels, > 0: a pair fits when its cost is below                */
    double clip_px;                /* pixels, >= 0; 0: no clip                                       */
    uint32_t flags;                /* MPE_REGROUP_RELEASE | MPE_REGROUP_ATTACH                       */
    int32_t reserved;
    const int32_t *d_persons;      /* [n_frames][pcap][V]                                            */
    const int32_t *d_n_persons;    /* [n_frames]                                                     */
    const void *d_poses;
    const uint8_t *d_flags;
    int32_t *d_persons_out;        /* [n_frames][pcap][V]                                            */
    uint8_t *d_change;             /* [n_frames][pcap][V]                                            */
    int32_t *d_n_views;            /* [n_frames][pcap]                                               */
    double *d_cost;                /* [n_heads][pcap]; NULL allowed when the batch has no heads      */
    int32_t *d_counts;             /* [n_frames][4]                                                  */
    int32_t *d_status;             /* [n_frames]                                                     */
} mpe_regroup_args;
int mpe_regroup_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_regroup_args *a);

/* Consolidation: the two repairs the regrouping leaves open, between mpe_regroup_batch and the second 3D stage.  MERGE: two
 * rows that hold the same body -- the greedy clustering gave each two or more views, so both got a pose, a few centimetres
 * apart -- become one.  FOUND: the skeletons no row names (the clustering missed them, or the release freed them from a
 * mixed row) found new rows where their back-projected rays meet.  All arithmetic is binary64, every operation named
 * below rounded on its own (nothing fused), quotients and roots correctly rounded; harness/consolidate.py states the same
 * in numpy, and the two agree bit for bit on every output.
 * Inputs.  The batch; d_persons / d_n_persons / d_poses / d_flags / pose_f64 / joint_flags / joint_mask / threshold / pcap
 *   exactly as mpe_regroup_batch takes them; merge_m > 0 and found_m > 0 (metres), clip_m >= 0, min_joints in 1..n_joints,
 *   found_min_views >= 2, fcap in 1..MPE_CONSOLIDATE_MAX_FREE with fcap * (3 n_joints + 1) <= MPE_CONSOLIDATE_RAY_DOUBLES,
 *   flags (MPE_CONSOLIDATE_MERGE | MPE_CONSOLIDATE_FOUND, at least one).  Rows, n = min(max(d_n_persons[f], 0), pcap), "has
 *   a pose", the bad-row check and the head cap are mpe_regroup_batch's, word for word.  A frame that is
 *   MPE_CONSOLIDATE_BAD_ROWS or MPE_CONSOLIDATE_OVER_CAP (the sticky status bit, as everywhere) is COPIED THROUGH: its rows and
 *   d_n_persons_out[f] = d_n_persons[f] unchanged, d_change 0, d_counts 0, d_dist, d_pair and d_free filled with -1,
 *   d_n_views counted from the rows as they are.
 * Merge distances.  Joint j of row p is present when the row has a pose, bit j is set in joint_mask, with joint_flags == 1
 *   d_flags[f][p][j] != 0, and its three coordinates, widened to f64, are finite.  The distance of rows p < q is the cost of
 *   mpe_track_batch with p in the role of a, over the joints both have in increasing j: dx, dy, dz = a - b; s = dx*dx;
 *   s = s + dy*dy; s = s + dz*dz; d = sqrt(s); the left-fold sum of d from 0.0, divided by the count n.  With
 *   n < min_joints, or a result that is not finite, the pair is UNSCORED: -1.  d_dist [n_frames][pcap][pcap] holds the
 *   distance at [p][q] for p < q < n and -1 everywhere else; it does not depend on d_persons and is written whatever flags.
 * Merge (MPE_CONSOLIDATE_MERGE), first.  A pair (p, q), p < q < n, is mergeable NOW when neither row has been merged away,
 *   it is scored and dist < merge_m (strict), and no camera holds an entry >= 0 in both rows as they are now.  The
 *   mergeable pair of least (dist, p, q) merges: q's entries move into p's open columns, q becomes all -1 and is merged
 *   away; repeated until no pair is mergeable.  Distances are not recomputed: p keeps its own pose's distances and tests
 *   disjointness with its union.  Rows are not renumbered and the row count does not fall.  Rows that share a camera are
 *   never merged: one of the two heads there is wrong, and which is for mpe_regroup_batch's release to decide.
 * Free heads.  The heads of the frame that no row p < n names (merging does not change them), in increasing head id; K their
 *   number.  d_free [n_frames][fcap]: the frame-local head id of ranks 0 .. min(K, fcap) - 1, -1 beyond.  With K > fcap the
 *   frame gets MPE_CONSOLIDATE_FREE_OVER_CAP: the merge stands, nothing is founded and d_pair is -1.
 * Pair costs.  Free heads a < b of different cameras (a in the role of h1): the mean ray distance of mpe_geom_scores_batch,
 *   by its ray lines (five-iteration undistortion, two Newton steps, rotation, norm) and its closest-point lines (the
 *   den < 1e-12 branch, both parameters clamped at 0, clip_m), folded as there: the sum over the voting joints in
 *   increasing j from 0.0, divided by their number n.  Joint j votes when bit j is set in joint_mask and in both heads'
 *   d_joint_mask and d_vp[h][j][0] > threshold (strict, mpe_regroup_batch's rule) for both.  With n < min_joints, two heads
 *   of one camera, a head whose camera index is outside 0..V-1, or a cost that is not finite the pair is UNSCORED: -1.
 *   d_pair [n_frames][fcap][fcap], indexed by rank, holds the cost at [a][b] for a < b < K and -1 everywhere else; written
 *   whatever flags.
 * Found (MPE_CONSOLIDATE_FOUND), after the merge.  A cursor (cost, a, b) starts below every pair.  Repeat: among the pairs with
 *   both heads free now, scored, cost < found_m and strictly greater than the cursor in (cost, a, b) order, take the least;
 *   with none, stop.  If the frame holds pcap rows already, set MPE_CONSOLIDATE_ROWS_FULL and stop.  The cursor becomes that
 *   pair.  The tentative row holds a and b and grows: a candidate is a free head whose camera the tentative row lacks and
 *   whose cost to EVERY member is scored and < found_m (complete linkage: no summation order); its key is (the largest of
 *   those costs, head id); the candidate of least key joins; repeated until there is no candidate.  With found_min_views
 *   heads or more the row is written at index n (every other column -1), n rises by one and the members stop being free;
 *   otherwise the row is dissolved: its heads stay free, and the cursor keeps the seed from seeding again (every pair seeds
 *   at most once, in increasing order).  Rows without a pose that exist already are left alone, and their heads are not
 *   free.  A founded row has no pose yet: the caller runs the 3D stage again on d_persons_out AND d_n_persons_out.
 * Outputs.  d_persons_out [n_frames][pcap][V] (may be d_persons itself); d_n_persons_out [n_frames] (may be d_n_persons):
 *   n plus the rows founded; d_change [n_frames][pcap][V], mpe_regroup_batch's coding: bit 0, the entry held a head and
 *   holds another or none now; bit 1, it holds a head it did not hold before; d_n_views [n_frames][pcap]: entries >= 0 of the
 *   rows below the new count, 0 beyond; d_dist, d_pair, d_free as above (d_dist f64, d_pair f64, d_free i32);
 *   d_counts [n_frames][4]: rows merged away, rows founded, heads placed by founding, heads named by no row afterwards;
 *   d_status [n_frames].
 * One launch (one workgroup per frame), ordered on `stream`; keeps no state, neither synchronises nor allocates; n_frames == 0
 *   does nothing; works on a context without weights.  MPE_ERR_INVALID for a merge_m or found_m that is not > 0 (or NaN), a
 *   negative (or NaN) clip_m, min_joints outside 1..n_joints, found_min_views < 2, fcap outside
 *   1..MPE_CONSOLIDATE_MAX_FREE, flags 0 or with unknown bits, a NULL output, n_frames other than the batch's, n_joints
 *   other than the context's, pcap < 1 or a pose_f64 / joint_flags other than 0 or 1; MPE_ERR_CAPACITY for
 *   pcap > MPE_REGROUP_MAX_PERSONS or fcap * (3 n_joints + 1) > MPE_CONSOLIDATE_RAY_DOUBLES. */
enum {
    MPE_CONSOLIDATE_BAD_ROWS = 1,
    MPE_CONSOLIDATE_OVER_CAP = 2,
    MPE_CONSOLIDATE_FREE_OVER_CAP = 4,
    MPE_CONSOLIDATE_ROWS_FULL = 8
};
enum {
    MPE_CONSOLIDATE_MERGE = 1,
    MPE_CONSOLIDATE_FOUND = 2
};
#define MPE_CONSOLIDATE_MAX_FREE 64
#define MPE_CONSOLIDATE_RAY_DOUBLES 3520   /* 64 free heads of 18 joints: 3 doubles a ray, one word a head */
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t joint_mask;           /* bit j: joint j may count                                       */
    float threshold;               /* 0.5, as for mpe_regroup_batch                                  */
    int32_t min_joints;            /* 1 .. n_joints: joints a scored pair (of rows, of heads) needs  */
    double merge_m;                /* metres, > 0: rows merge when their poses are closer            */
    double found_m;                /* metres, > 0: heads link when their rays pass closer            */
    double clip_m;                 /* metres, >= 0; 0: no clip                                       */
    int32_t found_min_views;       /* >= 2: heads a founded row needs                                */
    int32_t fcap;                  /* 1 .. MPE_CONSOLIDATE_MAX_FREE: free heads per frame taken      */
    uint32_t flags;                /* MPE_CONSOLIDATE_MERGE | MPE_CONSOLIDATE_FOUND                  */
    int32_t reserved;
    const int32_t *d_persons;      /* [n_frames][pcap][V]                                            */
    const int32_t *d_n_persons;    /* [n_frames]                                                     */
    const void *d_poses;
    const uint8_t *d_flags;
    int32_t *d_persons_out;        /* [n_frames][pcap][V]                                            */
    int32_t *d_n_persons_out;      /* [n_frames]                                                     */
    uint8_t *d_change;             /* [n_frames][pcap][V]                                            */
    int32_t *d_n_views;            /* [n_frames][pcap]                                               */
    double *d_dist;                /* [n_frames][pcap][pcap]                                         */
    double *d_pair;                /* [n_frames][fcap][fcap]                                         */
    int32_t *d_free;               /* [n_frames][fcap]                                               */
    int32_t *d_counts;             /* [n_frames][4]                                                  */
    int32_t *d_status;             /* [n_frames]                                                     */
} mpe_consolidate_args;
int mpe_consolidate_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_consolidate_args *a);

/* Clustering quality of the matching stage (test/sm_metrics.py:125-229, test/sm_metrics_without_gt.py:131-170): labels
 * from proposals, the ground-truth grouping of a frame's bodies_3D, and the four scores of two labelings.
 * harness/partition.py states all three on the host; host and device agree bit for bit.  Per-frame status words: */
enum {
    MPE_PART_SKIPPED = 1,          /* nothing computed for the frame (skip flag, no sample, unequal counts) */
    MPE_PART_OVER_CAP = 2          /* the frame exceeds a compiled cap: the caller finishes it on the host */
};
#define MPE_PART_MAX_SAMPLES 256    /* labels per frame mpe_partition_scores takes           */
#define MPE_PART_MAX_SKELETONS 1024 /* skeletons per frame mpe_group_bodies takes            */
#define MPE_PART_MAX_KEYS 32        /* distinct joint keys of a batch: one presence bit each */

/* One label per head of every frame: the index of the first proposal p < d_n_persons[f] whose row d_persons[f][p][:]
 * holds the frame-local head id, else d_n_persons[f] (sm_metrics.py:211-218).  d_labels[f][h] for h < H (the frame's head
 * count, from the batch), -1 beyond; d_count[f] = H; a frame with H > hcap gets MPE_PART_OVER_CAP and its first hcap labels. */
typedef struct {
    int32_t n_frames, pcap, hcap;
    const int32_t *d_persons;      /* [n_frames][pcap][V], as mpe_match_batch / mpe_cluster_batch write them */
    const int32_t *d_n_persons;    /* [n_frames]        */
    int32_t *d_labels;             /* [n_frames][hcap]  */
    int32_t *d_count;              /* [n_frames]        */
    int32_t *d_status;             /* [n_frames]        */
} mpe_partition_labels_args;
int mpe_partition_labels(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_partition_labels_args *a);

/* Ground-truth persons by greedy 3D proximity (sm_metrics.py:125-157).  The bodies of frame f, d_n[f] of them in (used
 * camera, list) order, are packed per joint KEY: the distinct keys of the batch are numbered 0..kcap-1; skeleton s has
 * d_xyz[f][s][k] for the keys of d_mask[f][s] (bit k), d_nkeys[f][s] keys in all, d_order[f][s][0..nkeys) their numbers in
 * the order of the body's dict, d_m1[f][s] = '-1' in body.  Skeleton by skeleton: against every person founded so far the
 * distance is the left-to-right f64 sum over the FOUNDING skeleton's keys in its d_order, of sqrt(fma(dz, dz, fma(dy, dy,
 * dx*dx))) for the keys skeleton s has too; the least distance wins (strict <, from 1e9; the first person of equals);
 * without a shared key or with distance / keys > 1. the skeleton founds person number d_n_groups.  d_labels[f][s] = the
 * person, -1 for s >= d_n[f]; d_skip[f] = 1 for a frame without persons, with a body lacking '-1', or with d_skip_in[f]
 * != 0 (d_skip_in may be NULL; such a frame is not grouped and gets MPE_PART_SKIPPED).  A frame with more than
 * MPE_PART_MAX_SKELETONS skeletons gets MPE_PART_OVER_CAP, d_skip = 1 and no labels.  MPE_ERR_CAPACITY for kcap >
 * MPE_PART_MAX_KEYS. */
typedef struct {
    int32_t n_frames, scap, kcap;
    const double *d_xyz;           /* [n_frames][scap][kcap][3] */
    const uint32_t *d_mask;        /* [n_frames][scap]          */
    const int32_t *d_nkeys;        /* [n_frames][scap]          */
    const uint8_t *d_order;        /* [n_frames][scap][kcap]    */
    const uint8_t *d_m1;           /* [n_frames][scap]          */
    const int32_t *d_n;            /* [n_frames]                */
    const uint8_t *d_skip_in;      /* [n_frames] or NULL        */
    int32_t *d_labels;             /* [n_frames][scap]          */
    int32_t *d_n_groups;           /* [n_frames]                */
    uint8_t *d_skip;               /* [n_frames]                */
    int32_t *d_status;             /* [n_frames]                */
} mpe_group_bodies_args;
int mpe_group_bodies(mpe_ctx *ctx, void *stream, const mpe_group_bodies_args *a);

/* The table of logarithms mpe_partition_scores reads: table[k - 1] = log k for k = 1..n, host memory, copied as it is (the
 * host statement reads the same numbers, so no logarithm is ever taken twice).  Once per context, before the first call. */
int mpe_set_log_table(mpe_ctx *ctx, const double *table, int32_t n);

/* d_scores[f] = adjusted Rand index, homogeneity, completeness, V-measure of the labelings d_labels_true[f][0..n) and
 * d_labels_pred[f][0..n), n = d_count[f] (sklearn's adjusted_rand_score and homogeneity_completeness_v_measure, sums in
 * the order harness/partition.py writes them: classes by ascending label, cells by ascending (true, predicted); integer
 * pair counts exact; nothing fused).  Four NaN and MPE_PART_SKIPPED for a frame with n <= 0, with d_skip[f] != 0 (may be
 * NULL) or with d_count_true[f] != n (may be NULL); four NaN and MPE_PART_OVER_CAP for n > ld_true, n > ld_pred
 * (the row lengths of the two label arrays), n > MPE_PART_MAX_SAMPLES or n * n beyond the table.  MPE_ERR_STATE without a table. */
typedef struct {
    int32_t n_frames, ld_true, ld_pred;
    const int32_t *d_labels_true;  /* [n_frames][ld_true] */
    const int32_t *d_labels_pred;  /* [n_frames][ld_pred] */
    const int32_t *d_count;        /* [n_frames]       */
    const int32_t *d_count_true;   /* [n_frames] or NULL */
    const uint8_t *d_skip;         /* [n_frames] or NULL */
    double *d_scores;              /* [n_frames][4]    */
    int32_t *d_status;             /* [n_frames]       */
} mpe_partition_scores_args;
int mpe_partition_scores(mpe_ctx *ctx, void *stream, const mpe_partition_scores_args *a);

/* ---- stage-level entry points (parity tests, Python mirrors of single reference symbols) */
/* C[M][N] = act(A[M][K] * W[N][K]^T + bias): nn.Linear (+ LeakyReLU when slope_on != 0).
 * Row strides in elements; A and C device pointers, W/bias device pointers prepared by
 * mpe_upload_linear (zero padded).  d_m, if not NULL, overrides M with a device-side count.
 * flags: bit 0 = apply LeakyReLU(slope), bit 1 = f64 running sums (see mpe_set_precision), bit 2 = the split-bf16 form
 * (csrc/gemm_sb16.hip; the planes are made for the call), with bit 3 = without its f64 sums and bit 4 = an f64 flush per K stage;
 * bit 5 = the f64 matrix-pipe form (csrc/gemm_f64.hip).
 * What is read and written (every form; tests/test_gpu_linear_contract.py):
 *   rows   M = min(m, *d_m) when d_m is given (m is then the capacity: kernel and grid are chosen from it, the bits of a row do
 *          not depend on it); M <= 0 launches or writes nothing.  Rows >= M of A are never read into a result (they may hold
 *          anything, NaN included) and rows >= M of C are never written.
 *   A      read over ldw columns of rows [0, M): columns [k, ldw) meet the zero padding of W and must be FINITE (0 * NaN is NaN);
 *          columns >= ldw are never read.
 *   C      written in [0, M) x [0, n) only: columns [n, ldc) and everything outside those rows keep their bytes.
 * MPE_ERR_INVALID, before anything is launched, unless ldw % 32 == 0, k <= ldw <= lda <= 2^21 (the split form's tile kernel
 * addresses 255 rows of lda floats by a 32-bit byte offset), lda % 4 == 0, ldc % 4 == 0, ldc >= n, and d_a, d_w, d_c are
 * 16-byte aligned (operands are moved in 16-byte pieces). */
int mpe_upload_linear(mpe_ctx *ctx, const float *w, const float *b, int32_t out_dim, int32_t in_dim,
                      float **d_w, float **d_b, int32_t *ldw);
int mpe_free_device(mpe_ctx *ctx, void *d_ptr);
int mpe_linear(mpe_ctx *ctx, void *stream, const float *d_a, int32_t lda, const float *d_w, int32_t ldw,
               const float *d_bias, float *d_c, int32_t ldc, int32_t m, const int32_t *d_m,
               int32_t n, int32_t k, int32_t flags, float slope);

/* HumanGraphFromView.initializeWithAlternative3 (graph_generator.py:444-508): the J*10
 * non-zero block of every head row: d_feat [n_heads][J][10]. */
int mpe_head_features(mpe_ctx *ctx, void *stream, const mpe_batch *b, float *d_feat);
/* graph.ndata['h'] of ONE frame's graph as the reference builds it (graph_generator.py:444-508, 629-631): the dense
 * [n_heads + n_edge_nodes][ld >= 2 + V*J*10] rows in node order -- head rows (column 0 = 1, the camera's J*10 block),
 * then the edge-node rows (one-hot at column 1); pad columns are zeroed.  For callers that ask for the matrix itself. */
int mpe_dense_rows(mpe_ctx *ctx, void *stream, const mpe_batch *b, float *d_rows, int32_t ld);

/* GAT2.forward over the batch (gat2.py:137-149).  d_feats == NULL: node rows are featurised
 * on the device from the packed skeletons (the production path; edge-node rows are constant
 * and de-duplicated).  d_feats != NULL: caller-provided dense [n_nodes][ld_feats] rows in
 * node order (frame by frame: heads, then edge-nodes), as GAT2.forward(inputs, g) receives.
 * d_scores_en [n_edge_nodes]; optional d_scores_heads [n_heads] (the reference also evaluates
 * the last layer at head nodes; unused downstream). */
/* Non-finite input (d_feats == NULL).  As at mpe_match_batch: values under a cleared mask bit are never read; a non-finite value
 * under a set bit affects the scores (edge-nodes and heads) of its own frame only; MPE_OK, no status bit; nothing survives into
 * later calls on the context.  Caller-provided rows: a row of d_feats affects the frame it belongs to. */
int mpe_gat_forward(mpe_ctx *ctx, void *stream, const mpe_batch *b, const float *d_feats, int32_t ld_feats,
                    float *d_scores_en, float *d_scores_heads);
/* Activation of the last GAT layer: 1 = sigmoid (final_activation = nn.Sigmoid(), the deployed
 * model, train_skeleton_matching.py:34), 2 = identity (final_activation = None, gat2.py:146-148). */
int mpe_set_gat_output(mpe_ctx *ctx, int32_t mode);

/* One GraphAttention2 layer (gat2.py:50-76) plus the activation GAT2.forward applies to its
 * flattened output (:141-147).  d_in [n_nodes][ld_in] holds the layer's input rows in node order
 * (frame by frame: heads, then edge-nodes; in_dim columns used), d_out [n_nodes][ld_out] receives
 * heads*out_dim columns.  activation: 0 = LeakyReLU(hidden slope), 1 = sigmoid, 2 = none.
 * Layer 0 takes dense F-wide rows (no de-duplication of the constant edge-node rows); with d_in == NULL (ld_in ignored) it
 * featurises the rows on the device as mpe_gat_forward(d_feats == NULL) does (implicit topology only) -- the production route of
 * layer 0; rows of frames without a graph then read 0 or the head's own transformed row, depending on the attention kernel.
 * Non-finite input.  As at mpe_match_batch: with d_in == NULL values under a cleared mask bit are never read and a non-finite value
 * under a set bit affects the rows of its own frame only; a non-finite row of d_in affects the rows of the frame it belongs to.
 * MPE_OK, no status bit.  Nothing survives into later calls, and nothing an earlier call left in the workspaces reaches this one:
 * the rows are laid over cleared workspace rows, pad columns of the layer's own fc1 output included. */
int mpe_gat_layer(mpe_ctx *ctx, void *stream, const mpe_batch *b, int32_t layer, const float *d_in, int32_t ld_in,
                  float *d_out, int32_t ld_out, int32_t activation);

/* The graph half of a layer only -- what the reference delegates to DGL (gat2.py:57-66, 78-88):
 * a1/a2 = <ft2, attn_l/r> (the two torch.bmm), apply_edges(LeakyReLU(a1[src] + a2[dst])),
 * edge_softmax over the in-edges of every destination, update_all(u_mul_e, sum).
 * d_ft2 [n_nodes][ld_ft2] = fc2 output (heads*out_dim columns) -> d_out [n_nodes][ld_out], no
 * activation.  Uses attn_l / attn_r of `layer`. */
int mpe_edge_softmax_aggregate(mpe_ctx *ctx, void *stream, const mpe_batch *b, int32_t layer, const float *d_ft2,
                               int32_t ld_ft2, float *d_out, int32_t ld_out);

/* Per-frame capacity.  The host side of this ABI sees batch totals only; a frame that holds
 * more than mpe_config.max_heads_per_frame skeletons (and therefore possibly more edge-nodes
 * than the per-frame LDS / scratch budget) is detected on the device: its scores come back as
 * zeros, it yields n_persons = 0, and a sticky status bit is raised.  mpe_sync_status
 * synchronises `stream`, returns MPE_ERR_CAPACITY if any batch since the last call contained
 * such a frame (MPE_ERR_INVALID if an explicit edge-node list held a bad pair; MPE_OK otherwise) and clears the bits.  Limits that mpe_create enforces:
 * max_heads_per_frame < 32768, n_cameras <= 32, n_joints <= 32, attention heads <= 16. */
int mpe_sync_status(mpe_ctx *ctx, void *stream);
/* The same in two halves: mpe_status_queue orders the read-back (into page-locked memory) and the reset of the word behind everything
 * queued on `stream` so far and returns at once; mpe_status_wait synchronises `stream` and reports what the read-back saw (it queues
 * one itself if none is pending).  Bits raised by work queued after mpe_status_queue are reported by the next call.
 * The context remembers the stream a pending read-back was ordered on: mpe_status_wait on another stream synchronises that stream
 * as well before it reads the word, and a second mpe_status_queue (on any stream) waits for the pending one and carries its bits
 * into the next report -- no bit is lost and none is read early, whichever streams the two halves are given.  (A stream with a
 * read-back pending on it must stay alive until that read-back has been waited for.) */
int mpe_status_queue(mpe_ctx *ctx, void *stream);
int mpe_status_wait(mpe_ctx *ctx, void *stream);

/* CLASSIFICATION_THRESHOLD of get_person_proposal_from_network_output (default from mpe_config).  It takes no stream: the
 * device-side configuration is rewritten with a blocking copy that is ordered against nothing a non-blocking stream holds.  Call
 * it only with nothing pending on the context (after mpe_sync_status / a synchronisation of every stream the context was given
 * work on); clustering that is still queued may otherwise run with either threshold. */
int mpe_set_threshold(mpe_ctx *ctx, float threshold);

/* get_person_proposal_from_network_output on caller-provided scores. */
int mpe_cluster_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const float *d_scores,
                      int32_t *d_persons, int32_t *d_n_persons);

/* MLP input rows only: d_rows [n_frames*Pcap][ld_rows] f32 (row r = frame*Pcap + p).
 * Non-finite input.  As at mpe_mlp3d_batch: values under a cleared mask bit are never read; a non-finite value under a set bit
 * reaches the rows of the persons that hold its head and no other row; d_valid of such a row is the reference's sum(|row|) > 1 on
 * it (a NaN in the row: 0; infinities only: 1).  MPE_OK, no status bit; the call keeps nothing on the context. */
int mpe_mlp_input_rows(mpe_ctx *ctx, void *stream, const mpe_batch *b, const int32_t *d_persons,
                       const int32_t *d_n_persons, float *d_rows, int32_t ld_rows, uint8_t *d_valid);
/* PoseEstimatorMLP.forward on d_x [m][ld_x] -> d_y [m][ld_y] (out_dim columns written, the rest of a row kept; no x10).
 * d_x is read as mpe_linear reads A: over round_up(in_dim, 128) columns, those beyond in_dim zero (finite at least); columns
 * beyond that are never read.  MPE_ERR_INVALID, before anything is launched, unless round_up(in_dim, 128) <= ld_x <= 2^21,
 * ld_x % 4 == 0, d_x is 16-byte aligned and ld_y >= out_dim. */
int mpe_mlp_forward(mpe_ctx *ctx, void *stream, const float *d_x, int32_t ld_x, int32_t m,
                    float *d_y, int32_t ld_y);

/* cv2.undistortPoints + cv2.triangulatePoints for explicit pairs (pose_estimator_utils.py:63-67):
 * d_pts [n][2][2] pixel points, d_cams [n][2] camera indices -> d_out [n][3] f64. */
int mpe_dlt_pairs(mpe_ctx *ctx, void *stream, const double *d_pts, const int32_t *d_cams,
                  int32_t n, double *d_out);

/* ---- host-side packer (no GPU involved) ---------------------------------------------------
 * Frame JSON in the reference's wire format (list of frames; frame = {camera: ["<JSON text of
 * the skeleton list>", timestamp, 'no_image', bodies_3D]}; skeleton = {joint id: [id, x, y,
 * valid, prob], optional "ID"}; panoptic_conversor/get_joints_from_panoptic_model_multi.py:
 * 231-236,281,287) -> the host arrays of an mpe_batch, in the reference's head order
 * (graph_generator.py:573-605).  Replaces json.load + json.loads per camera + the Python
 * loops of load_people_view_graph.  Frames frame_start, frame_start+frame_step, ... (at most
 * max_frames, 0 = all) are parsed by n_threads threads (0 = all cores). */
typedef struct mpe_packed mpe_packed;
typedef struct {
    int32_t n_frames, n_heads, n_edge_nodes, n_cameras, n_joints;
    const int32_t *frame_head_off, *frame_en_off, *slot_cam, *slot_n, *head_cam, *skeleton_index;
    const uint32_t *joint_mask, *tri_mask;
    const double *xy;
    const float *vp;
} mpe_packed_arrays;
int mpe_pack_json(const char *json, size_t len, const char *const *camera_names, int32_t n_cameras,
                  int32_t n_joints, int32_t frame_start, int32_t frame_step, int32_t max_frames,
                  int32_t n_threads, mpe_packed **out);
int mpe_packed_view(const mpe_packed *pk, mpe_packed_arrays *view);
/* The same parse straight into caller-provided arrays -- e.g. views of ONE page-locked buffer
 * that then travels to the device in a single copy (no intermediate host copies).  Capacities
 * max_frames / max_heads are the caller's array sizes: frame_head_off / frame_en_off hold
 * max_frames + 1 entries, slot_cam / slot_n max_frames * n_cameras, the per-head arrays max_heads
 * (xy / vp max_heads * n_joints * 2).  At most min(max_frames argument, dst->max_frames) frames are
 * parsed; MPE_ERR_CAPACITY if their skeletons exceed dst->max_heads. */
typedef struct {
    int32_t max_frames, max_heads;
    int32_t *frame_head_off, *frame_en_off, *slot_cam, *slot_n, *head_cam, *skeleton_index;
    uint32_t *joint_mask, *tri_mask;
    double *xy;
    float *vp;
} mpe_pack_dst;
int mpe_pack_json_into(const char *json, size_t len, const char *const *camera_names, int32_t n_cameras,
                       int32_t n_joints, int32_t frame_start, int32_t frame_step, int32_t max_frames,
                       int32_t n_threads, const mpe_pack_dst *dst, int32_t *n_frames, int32_t *n_heads,
                       int32_t *n_edge_nodes);
/* ONE frame as the reference's per-frame callers hold it after json.load (test/metrics_from_model.py:182-199; what
 * MergedMultipleHumansDataset(mode='test') receives, graph_generator.py:813-876): per configured camera the TEXT of its skeleton list
 * (frame[cam][0]), in the frame dict's order; cams[i] = that camera's index in the configured list.  Same grammar, head order and numbers
 * as mpe_pack_json_into gives for the document [frame]; dst as there with max_frames >= 1.  extents (NULL or dst->max_heads * 2 entries)
 * receives per head the byte offsets [begin, end) of its skeleton object inside its camera text (the per-frame callers hand single
 * skeletons on as text, metrics_from_model.py:250-252).  MPE_ERR_INVALID with mpe_pack_last_error for text the packer declines,
 * MPE_ERR_CAPACITY beyond dst->max_heads. */
int mpe_pack_views_into(const char *const *texts, const size_t *lens, const int32_t *cams, int32_t n_views, int32_t n_cameras,
                        int32_t n_joints, const mpe_pack_dst *dst, int32_t *n_heads, int32_t *n_edge_nodes, int32_t *extents);
/* A document that is consumed in windows (frame_start, max_frames): the index scans the document for
 * its frame extents ONCE, in a background thread it starts at creation, ahead of the windows; a window
 * is parsed as its frames are published (n_threads = 0: as many workers as the process may use: the
 * smaller of the hardware threads, the affinity mask and the cgroup CPU quota; MPE_PACK_THREADS
 * overrides).  A malformed document fails the first window that reaches the damage.  `json` must stay
 * valid and unchanged while the index lives; mpe_json_index_free joins the scan thread.  One index may
 * be used from one caller thread at a time. */
typedef struct mpe_json_index mpe_json_index;
int mpe_json_index_create(const char *json, size_t len, mpe_json_index **out);
void mpe_json_index_free(mpe_json_index *ix);
int mpe_pack_indexed_into(mpe_json_index *ix, const char *const *camera_names, int32_t n_cameras, int32_t n_joints,
                          int32_t frame_start, int32_t frame_step, int32_t max_frames, int32_t n_threads,
                          const mpe_pack_dst *dst, int32_t *n_frames, int32_t *n_heads, int32_t *n_edge_nodes);
void mpe_packed_free(mpe_packed *pk);
const char *mpe_pack_last_error(void);

/* ---- device-side second-level parse (csrc/jsonparse.hip) -----------------------------
 * The host keeps the first level of the wire format only: mpe_json_stage_window walks the frames of a window
 * (extents from the index) down to the camera entries, records for every configured camera the extent of the
 * STRING that holds its skeleton list (frame dict key order: graph_generator.py:583-601) and copies those
 * strings, 16-byte aligned, into `text_dst` -- one page-locked buffer that travels to the device in one copy.
 * mpe_json_parse_device parses the strings there into the arrays of `out` (device pointers; capacities as for
 * mpe_pack_dst) and `d_skeleton_index`, replacing json.loads per camera + load_people_view_graph
 * (graph_generator.py:573-605) like the host packer, whose arrays it reproduces bit for bit.
 *   skeletons_per_string_cap  rows of the staging arena per string (a string with more skeleton objects goes to the host)
 *   d_scratch  mpe_json_scratch_bytes(n_entries, skeletons_per_string_cap, n_joints) bytes of device memory
 *   d_totals   [4]: n_heads, n_edge_nodes, status (0 ok, bit 0: a string needs the host parser, bit 1: more
 *              heads than head_cap), largest number of heads in a frame
 * MPE_ERR_UNSUPPORTED from the staging call and a non-zero status both mean: pack this window with
 * mpe_pack_indexed_into (the host parser defines the accepted language and the error messages). */
typedef struct {
    int32_t frame, cam;            /* frame of the window, camera index (position in camera_names) */
    uint32_t begin, end;           /* the string's body in the staged text                         */
} mpe_json_entry;
int mpe_json_stage_window(mpe_json_index *ix, const char *const *camera_names, int32_t n_cameras, int32_t frame_start,
                          int32_t frame_step, int32_t max_frames, int32_t n_threads, char *text_dst, size_t text_cap,
                          mpe_json_entry *entries, int32_t entry_cap, int32_t *frame_entry_off, int32_t *n_frames,
                          int32_t *n_entries, size_t *text_bytes);
size_t mpe_json_scratch_bytes(int32_t n_entries_cap, int32_t skeletons_per_string_cap, int32_t n_joints);
int mpe_json_parse_device(mpe_ctx *ctx, void *stream, const char *d_text, const mpe_json_entry *d_entries,
                          const int32_t *d_frame_entry_off, int32_t n_entries, int32_t n_frames, int32_t head_cap,
                          int32_t skeletons_per_string_cap, void *d_scratch, size_t scratch_bytes, const mpe_batch *out,
                          int32_t *d_skeleton_index, int32_t *d_totals);

/* ---- ground-truth bodies of the frame JSON on the device (csrc/jsonparse.hip, csrc/gt.hip) -----------------
 * The fourth element of every camera entry is bodies_3D: a JSON list (not a string) of dicts {"<joint>": [x, y, z],
 * ..., "-1": [x, y, z]}, centimetres.  mpe_json_stage_gt_window is mpe_json_stage_window for that element: for every
 * frame of the window and EVERY camera key of the frame, in the frame's key order, one mpe_json_entry with the extent
 * of element [3] (cam = the position in camera_names, -1 for a key that is not configured: test/metrics_from_model.py:
 * 126-138 looks at all keys), the extents copied 16-byte aligned into text_dst.  The host walks the first level only;
 * it neither counts nor parses bodies.  MPE_ERR_UNSUPPORTED for a camera entry that is not a list of exactly four
 * elements or whose element [3] is not a list: the caller then takes the host path (json.load), which keeps the
 * reference's "There is no ground truth" behaviour. */
int mpe_json_stage_gt_window(mpe_json_index *ix, const char *const *camera_names, int32_t n_cameras, int32_t frame_start,
                             int32_t frame_step, int32_t max_frames, int32_t n_threads, char *text_dst, size_t text_cap,
                             mpe_json_entry *entries, int32_t entry_cap, int32_t *frame_entry_off, int32_t *n_frames,
                             int32_t *n_entries, size_t *text_bytes);

/* The staged lists parsed on the device into the arrays mpe_group_bodies takes (kcap = MPE_GT_KEY_SLOTS; they can be
 * passed to it as they are).  Row [f][s]: the bodies of frame f's CONFIGURED cameras in (entry order, list order) --
 * d_n[f] of them, what harness/partition.py:pack_bodies packs -- and behind them the bodies of the entries with cam ==
 * -1 in the same order (mpe_gt_from_bodies may select such a camera).  Key slots are fixed: joint key "j", j in
 * 0..30, is slot j and "-1" is slot 31 (mpe_group_bodies sums over the founding skeleton's keys in d_order and does
 * not depend on the numbering).  The numbers are the correctly rounded binary64 of the decimal text (Python's float()),
 * untouched.  Accepted language per body: {"<key>": [n, n, n], ...} with blanks between tokens; any other key (a
 * leading zero, "-0", 31 and up, text), a value that is not a list of exactly three numbers, null / NaN / Infinity,
 * a number of more than 19 significant digits or outside the exact conversion's range, a duplicate key in a body and
 * any nesting set bit 0 of *d_status ("host parser, please"); a frame with more than scap bodies sets bit 1 -- the two
 * bits and the contract of mpe_json_parse_device's status word.  With a non-zero status the arrays are not to be used.
 *   d_scratch  mpe_json_bodies_scratch_bytes(n_entries, scap) bytes of device memory */
#define MPE_GT_KEY_SLOTS 32
#define MPE_GT_M1_SLOT 31
typedef struct {
    int32_t n_frames, n_entries, scap;
    const char *d_text;                   /* staged text                                            */
    const mpe_json_entry *d_entries;      /* [n_entries]                                            */
    const int32_t *d_frame_entry_off;     /* [n_frames+1]                                           */
    double *d_xyz;                        /* [n_frames][scap][32][3], 0 where the key is absent     */
    uint32_t *d_mask;                     /* [n_frames][scap] bit per key slot                      */
    int32_t *d_nkeys;                     /* [n_frames][scap]                                       */
    uint8_t *d_order;                     /* [n_frames][scap][32] key slots in the body's dict order*/
    uint8_t *d_m1;                        /* [n_frames][scap] '-1' in body                          */
    int32_t *d_n;                         /* [n_frames] bodies of configured cameras                */
    int32_t *d_entry_count;               /* [n_entries] bodies of every entry, configured or not   */
    int32_t *d_body_cam;                  /* [n_frames][scap] camera index of the row's entry; -1 for a non-configured camera and for unused rows */
    int32_t *d_status;                    /* [1]                                                    */
    void *d_scratch;
    size_t scratch_bytes;
} mpe_json_bodies_args;
size_t mpe_json_bodies_scratch_bytes(int32_t n_entries_cap, int32_t scap);
int mpe_json_parse_bodies_device(mpe_ctx *ctx, void *stream, const mpe_json_bodies_args *a);

/* Ground truth of the metrics scripts from the parsed bodies (test/metrics_from_model.py:126-174), one workgroup per
 * frame, written as mpe_eval_batch reads it.  Camera: the frame's first entry, replaced by a later entry only when its
 * d_entry_count is STRICTLY greater (all keys of the frame, configured or not).  d_n_gt_in[f] = that entry's bodies
 * (0: the frame the callers skip); body b of it, joint j < n_joints:
 *   d_gt_joint[f][b][j] = key "j" present;  d_gt_valid[f][b] = '-1' present;  d_gt_xyz[f][b][j] = 0 when absent, else
 *   g_k = (float)(v_k / 100.0)             an IEEE f64 division, then one rounding to f32;  x = (g_0, g_1, g_2, 1)
 *   y = T_d[file_of_frame[f]] x ; w = T_i1 y   (the first three rows of w), every row of both products
 *   acc = T[i][0] * x_0 ; acc = fmaf(T[i][k], x_k, acc) for k = 1, 2, 3    fp32, nothing else contracted
 * which gives the bits of torch's fp32 matmul on the CPU (harness/groundtruth.py states it in numpy, exactly).
 * T_i1 is HOST memory (16 floats, copied into the launch); d_T_d [n_files][4][4] f32 and d_file_of_frame [n_frames] are
 * device arrays.  MPE_ERR_CAPACITY for gcap < scap or n_joints > 31. */
typedef struct {
    int32_t n_frames, scap, gcap, n_joints, n_files;
    const mpe_json_entry *d_entries;
    const int32_t *d_frame_entry_off;     /* [n_frames+1]                  */
    const int32_t *d_entry_count;         /* [n_entries]                   */
    const double *d_xyz;                  /* [n_frames][scap][32][3]       */
    const uint32_t *d_mask;               /* [n_frames][scap]              */
    const uint8_t *d_m1;                  /* [n_frames][scap]              */
    const float *d_T_d;                   /* [n_files][16]                 */
    const int32_t *d_file_of_frame;       /* [n_frames]                    */
    const float *T_i1;                    /* HOST [16]                     */
    float *d_gt_xyz;                      /* [n_frames][gcap][n_joints][3] */
    uint8_t *d_gt_joint;                  /* [n_frames][gcap][n_joints]    */
    uint8_t *d_gt_valid;                  /* [n_frames][gcap]              */
    int32_t *d_n_gt_in;                   /* [n_frames]                    */
} mpe_gt_args;
int mpe_gt_from_bodies(mpe_ctx *ctx, void *stream, const mpe_gt_args *a);

/* Tracking: one identity per person over the frames of a recording.  Row p of one frame's poses has nothing to do with
 * row p of the next (person order is the clustering's; the reference's viewers colour by that row,
 * test/show_results_from_model.py:276,321,329); mpe_track_batch gives every detection a track id that follows the person.
 * The rule (harness/tracking.py states it in numpy, frame by frame, and the two agree exactly):
 *   Detections of frame f: as in mpe_eval_batch.  joint_flags == 0: persons p < d_n_persons[f] with d_flags[f][p] != 0,
 *   all joints present; joint_flags == 1: every p < d_n_persons[f], joint j present when d_flags[f][p][j] != 0.  Only
 *   joints of used_joint_mask count; a person with no present used joint is not a detection.
 *   Cost of a newer detection a against an older one b: over the used joints both have, in increasing j, the stored
 *   coordinates widened to f64: dx, dy, dz = a - b; s = dx*dx; s = s + dy*dy; s = s + dz*dz (every product and sum
 *   rounded on its own); d = sqrt(s), correctly rounded; the left-fold sum of d divided by the count.  No common joint:
 *   +inf.  A pair is linkable when cost < gate (strict; a NaN never links).
 *   Cascade, g = 1 .. max_gap + 1 (the tracks seen last choose first): for every frame t, rows = its detections without
 *   a parent, columns = the detections of frame t - g without a child; take the linkable pair of least cost (ties: the
 *   lowest row, then the lowest column, in detection order), link it, remove both, until none is left.  Within one g
 *   the frames are independent; the result is that of the frame-by-frame online cascade.
 *   Ids: a detection without a parent starts a track; ids are consecutive in birth order (frame, then detection order)
 *   from the state's count; every other detection takes its parent's id.
 * Outputs per row [n_frames][pcap]: d_track_id (-1: not a detection); d_link_cost f64 (-1.0 for a birth and for rows
 * that are no detection); d_link_gap (g of the link, 0 for a birth, -1 no detection); *d_issued = ids issued so far.
 * The state holds the detections of the last max_gap + 1 frames with their ids and has-child marks and the count, so a
 * sequence may arrive in any chunking (one frame per call included) and gets the same ids; joint_flags, used_joint_mask
 * and gate are per call.  mpe_track_create allocates all device memory the calls need (MPE_ERR_CAPACITY for pcap >
 * MPE_TRACK_MAX_PERSONS or max_gap > MPE_TRACK_MAX_GAP); mpe_track_reset starts a new sequence, ordered on `stream`;
 * mpe_track_batch is ordered on `stream` like the other batch entry points and neither synchronises nor allocates: max_gap + 7
 * kernels whatever n_frames is (mpe_track_launches: the launches of a state that the runtime accepted, counted on the host).  n_frames == 0 does
 * nothing.  Sizes or a pose type other than the state's: MPE_ERR_INVALID (the code this header has for a bad argument),
 * with the three values in mpe_last_error; n_frames > 2^23: MPE_ERR_CAPACITY.  Calls on one state belong on one stream,
 * in sequence order. */
#define MPE_TRACK_MAX_PERSONS 128
#define MPE_TRACK_MAX_GAP 15
typedef struct mpe_track_state mpe_track_state;
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t used_joint_mask;
    double gate;                   /* metres, > 0 */
    const void *d_poses;
    const uint8_t *d_flags;
    const int32_t *d_n_persons;    /* [n_frames] */
    int32_t *d_track_id;           /* [n_frames][pcap] */
    double *d_link_cost;           /* [n_frames][pcap] */
    int32_t *d_link_gap;           /* [n_frames][pcap] */
    int32_t *d_issued;             /* [1] */
} mpe_track_args;
int mpe_track_create(mpe_ctx *ctx, int32_t pcap, int32_t n_joints, int32_t max_gap, int32_t pose_f64, mpe_track_state **out);
int mpe_track_reset(mpe_ctx *ctx, void *stream, mpe_track_state *state);
int mpe_track_destroy(mpe_ctx *ctx, mpe_track_state *state);
int mpe_track_batch(mpe_ctx *ctx, void *stream, mpe_track_state *state, const mpe_track_args *a);
int mpe_track_launches(mpe_ctx *ctx, const mpe_track_state *state, int64_t *n);

/* Smoothing: tracked poses filtered over time.  A causal, windowed, weighted line fit per (track, joint, axis) over the
 * RAW poses of the current frame and the `window` (W) frames before it: no feedback, so every output is a function of
 * W + 1 frames of input and all (frame, person, joint) outputs of a call are independent.  It follows d_track_id, not
 * person rows.  The rule (harness/smoothing.py states it in numpy, and the two agree bit for bit):
 *   Detections and joint presence as in mpe_track_batch.  Row p of frame f is a detection when p < d_n_persons[f],
 *   d_track_id[f][p] >= 0 and, with joint_flags == 0, d_flags[f][p] != 0; joint_flags == 0: all joints of a detection
 *   are present; joint_flags == 1: joint j is present when d_flags[f][p][j] != 0.  Only joints of joint_mask are
 *   processed.
 *   Samples of joint j of a detection with id t: for age a = 0 .. W the sample of age a exists when frame f - a exists
 *   in the sequence (frames count over the whole sequence; the state supplies those before the call), that frame has a
 *   detection with id t (the lowest such row; for a = 0 row p itself, which it is when ids are unique within a frame,
 *   as the tracker's are), joint j is present in that row by the INPUT flags and its three stored coordinates are
 *   finite.  Value: the stored input coordinate widened to f64.  Weight: w_0 = 1, w_a = w_(a-1) * lambda, every
 *   product rounded on its own.
 *   Sums: n = the number of samples, r = the youngest one.  Per axis, y_a = x_a - x_r, u_a = (double)a, c_a = w_a * u_a;
 *   left-fold sums from 0.0 over the samples in increasing a, nothing contracted:
 *   S0 += w_a; S1 += c_a; S2 += c_a * u_a; T0 += w_a * y_a; T1 += c_a * y_a.
 *   Fit (IEEE f64 divisions): D = S0*S2 - S1*S1; alpha = x_r + (S2*T0 - S1*T1) / D; beta = (S0*T1 - S1*T0) / D.  A fit
 *   exists when n >= 2, D > 0 and alpha and beta are finite on all three axes.
 *   Joint present now (the sample of age 0 exists): with a fit d_poses_out = alpha, rounded once to the pose type, and
 *   d_vel = -beta (metres per frame); without one the input bits are copied and d_vel = 0.  A joint that is present
 *   but not finite now is copied likewise.  d_flags_out is 1 for a present joint with joint_flags == 1; with
 *   joint_flags == 0 it is the input flag.
 *   Joint missing now (joint_flags == 1 only): with fill != 0 and a fit, d_poses_out = alpha, d_vel = -beta and
 *   d_flags_out = MPE_SMOOTH_FILLED; otherwise the input bits, d_flags_out = 0, d_vel = 0.
 *   d_n_samples = n for every processed joint.  Rows that are no detection and joints outside joint_mask are copied
 *   through bit for bit with d_vel = 0, d_n_samples = 0 and the input flag.  window == 0 copies everything.
 * A person who has no row at all in a frame gets none here either.  The state holds, for the last W frames, the
 * coordinates widened to f64, the presence masks and the ids: a sequence cut into any chunks, one frame per call
 * included, gives the same bits.  window is fixed at create time; lambda, fill, joint_flags and joint_mask are per call.
 * mpe_smooth_create allocates all device memory the calls need (MPE_ERR_CAPACITY for pcap > MPE_TRACK_MAX_PERSONS,
 * MPE_ERR_INVALID for a window outside 0 .. MPE_SMOOTH_MAX_WINDOW); mpe_smooth_reset starts a new sequence, ordered on
 * `stream`; mpe_smooth_batch is ordered on `stream` and neither synchronises nor allocates: two kernels whatever n_frames
 * is, the filter and the carry of the last W frames into the other half of the state (one when window == 0;
 * mpe_smooth_launches counts them as mpe_track_launches does).  n_frames == 0 does nothing.  MPE_ERR_INVALID, with the
 * values in mpe_last_error: sizes or a pose type other than the state's, lambda outside [0.25, 1], joint_flags outside
 * {0, 1}, d_poses_out == d_poses; n_frames > 2^23: MPE_ERR_CAPACITY.  Calls on one state belong on one stream, in
 * sequence order. */
#define MPE_SMOOTH_MAX_WINDOW 15
#define MPE_SMOOTH_FILLED 2
typedef struct mpe_smooth_state mpe_smooth_state;
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    int32_t fill;
    uint32_t joint_mask;
    double lambda;                 /* weight ratio of consecutive ages, within [0.25, 1] */
    const void *d_poses;
    const uint8_t *d_flags;
    const int32_t *d_n_persons;    /* [n_frames] */
    const int32_t *d_track_id;     /* [n_frames][pcap], mpe_track_batch's */
    void *d_poses_out;             /* the type and shape of d_poses, another buffer */
    uint8_t *d_flags_out;          /* the shape of d_flags */
    double *d_vel;                 /* [n_frames][pcap][J][3] */
    uint8_t *d_n_samples;          /* [n_frames][pcap][J] */
} mpe_smooth_args;
int mpe_smooth_create(mpe_ctx *ctx, int32_t pcap, int32_t n_joints, int32_t window, int32_t pose_f64, mpe_smooth_state **out);
int mpe_smooth_reset(mpe_ctx *ctx, void *stream, mpe_smooth_state *state);
int mpe_smooth_destroy(mpe_ctx *ctx, mpe_smooth_state *state);
int mpe_smooth_batch(mpe_ctx *ctx, void *stream, mpe_smooth_state *state, const mpe_smooth_args *a);
int mpe_smooth_launches(mpe_ctx *ctx, const mpe_smooth_state *state, int64_t *n);

/* Track scoring: how well the track ids follow the ground-truth identities over a recording -- CLEAR-MOT (MOTA, MOTP, ID
 * switches, fragmentations, MT / PT / ML; Bernardin & Stiefelhagen 2008) and the identity measures IDF1 / IDP / IDR
 * (Ristani et al. 2016).  The inputs are what mpe_eval_batch and mpe_track_batch left on the device plus one identity
 * per GT row; every output is an exact integer or one f64 left fold, so there is nothing to tolerate.  The rule
 * (harness/track_score.py states it in numpy, and the two agree exactly):
 *   Frames arrive in sequence order, in any chunking.  A frame with d_skip[f] != 0 (d_skip may be NULL) changes neither
 *   the state nor the frame count; its d_frame_counts are 0 and its d_match_tid are -2.
 *   Prediction side of frame f: detections and their order are mpe_eval_batch's.  joint_flags == 0: detection r is the
 *   r-th row p < d_n_persons[f] with d_flags[f][p] != 0; joint_flags == 1: r = p < d_n_persons[f].  Those with
 *   r < d_n_res[f] exist.  Detection r carries g = d_assign[f][r], e = d_err[f][r] (metres), d_invalid[f][r] (NULL
 *   pointer: 0) and the track id h = d_track_id[f][p(r)] (row order, as mpe_track_batch writes it).
 *   GT side: row g < d_n_gt[f] carries o = d_gt_id[f][g] and d_gt_valid[f][g]; it is COUNTED when valid and o >= 0,
 *   every other row is an IGNORE row.
 *   Classes: a detection with 0 <= g < d_n_gt[f] whose row is an ignore row is IGNORED and counts nowhere.  A detection
 *   is a CANDIDATE when g names a counted row, e * 1000. < threshold_mm (f64, strict), it is not invalid and h >= 0; the
 *   candidate of lowest r of a row is its MATCH (mpe_eval_batch's assignment is one-to-one, so there is one at most).
 *   Every other detection that is not ignored is a FALSE POSITIVE; a counted row without a match is a MISS.
 *   Per frame: d_frame_counts[f] = {tp, fp, fn, idsw}; d_match_tid[f][g] = h of the match, -1 for a miss, -2 for a row
 *   that is not counted (g >= d_n_gt[f] included).
 *   Identity pass: the RECORD of a counted row is (o, h) or (o, miss).  For every identity o, over the frames with a
 *   record of o in sequence order: present[o] += 1; with a match: matched[o] += 1, table[o][h] += 1, an ID switch when
 *   last[o] >= 0 and last[o] != h (it counts in the frame's idsw), then last[o] = h, and a fragmentation when o was
 *   matched in an earlier frame and its previous record was a miss; last[o] survives misses and absences.
 *   pred_count[h] += 1 for every detection with h >= 0 that is not ignored.
 *   Left out, each adding 1 to over_ids and setting the sticky MPE_TRACK_SCORE_OVER_IDS: a record with o >= gid_cap,
 *   with a matched h >= tid_cap, or whose o a lower counted row of the frame already carries (the identity pass sees
 *   nothing of it); a pred_count increment with h >= tid_cap.  tp / fp / fn count them all the same.
 *   Totals (int64, in the state): frames, n_gt (counted rows), n_pred (detections not ignored), tp, fp, fn, idsw, frag,
 *   ignored, over_ids.  err_sum: the f64 left fold of e over the matches in (frame, detection) order, every addition
 *   rounded on its own, continued from call to call.
 * mpe_track_score_create allocates all device memory the calls need: the state, table[gid_cap][tid_cap] and a scratch of
 * max_frames frames (MPE_ERR_CAPACITY for pcap or gcap > MPE_TRACK_MAX_PERSONS or gid_cap * tid_cap > 2^22).
 * mpe_track_score_reset starts a new recording, ordered on `stream`.  mpe_track_score_batch is ordered on `stream` and
 * neither synchronises nor allocates: three kernels whatever n_frames is (mpe_track_score_launches counts them as
 * mpe_track_launches does); n_frames == 0 does nothing.  MPE_ERR_INVALID: pcap / gcap other than the state's,
 * joint_flags outside {0, 1}, threshold_mm <= 0; MPE_ERR_CAPACITY: n_frames > max_frames.  *d_status receives the sticky
 * bits.  Calls on one state belong on one stream, in sequence order.
 * mpe_track_score_result is the only call that synchronises (`stream`): it reads the state back and finishes on the
 * host.  MOTA = 1 - (fn + fp + idsw) / n_gt; MOTP_mm = err_sum * 1000 / tp; IDTP = the largest sum of table over
 * one-to-one pairings of identities and tracks (an exact integer; once per recording, on the host: csrc/assign_int.h);
 * IDP = IDTP / n_pred, IDR = IDTP / n_gt, IDF1 = 2 IDTP / (n_gt + n_pred); an identity with present > 0 is mostly
 * tracked when 5 * matched >= 4 * present, mostly lost when 5 * matched < present, partially tracked otherwise;
 * n_ids = identities with present > 0, n_tracks = tracks with pred_count > 0.  A ratio with a zero denominator is NaN. */
#define MPE_TRACK_SCORE_OVER_IDS 1
#define MPE_TRACK_SCORE_MAX_TABLE (1 << 22)
typedef struct mpe_track_score_state mpe_track_score_state;
typedef struct {
    int32_t n_frames, pcap, gcap;
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8 (f32 poses' person flags); 1: not read, r = p */
    double threshold_mm;           /* > 0 */
    const uint8_t *d_flags;        /* joint_flags == 0 only */
    const int32_t *d_n_persons;    /* [n_frames] */
    const int32_t *d_track_id;     /* [n_frames][pcap], mpe_track_batch's */
    const int32_t *d_assign;       /* [n_frames][pcap], mpe_eval_batch's (detection order), as d_err and d_invalid */
    const double *d_err;           /* [n_frames][pcap] */
    const uint8_t *d_invalid;      /* [n_frames][pcap] or NULL */
    const int32_t *d_n_res;        /* [n_frames] */
    const int32_t *d_n_gt;         /* [n_frames] */
    const int32_t *d_gt_id;        /* [n_frames][gcap] */
    const uint8_t *d_gt_valid;     /* [n_frames][gcap] */
    const uint8_t *d_skip;         /* [n_frames] or NULL */
    int32_t *d_frame_counts;       /* [n_frames][4] */
    int32_t *d_match_tid;          /* [n_frames][gcap] */
    int32_t *d_status;             /* [1] */
} mpe_track_score_args;
typedef struct {
    int64_t frames, n_gt, n_pred, tp, fp, fn, idsw, frag, ignored, over_ids;
    int64_t idtp, n_ids, n_tracks, mt, pt, ml;
    double err_sum, mota, motp_mm, idp, idr, idf1;
    int32_t status, reserved;
} mpe_track_score_totals;
int mpe_track_score_create(mpe_ctx *ctx, int32_t pcap, int32_t gcap, int32_t gid_cap, int32_t tid_cap, int32_t max_frames,
                           mpe_track_score_state **out);
int mpe_track_score_reset(mpe_ctx *ctx, void *stream, mpe_track_score_state *state);
int mpe_track_score_destroy(mpe_ctx *ctx, mpe_track_score_state *state);
int mpe_track_score_batch(mpe_ctx *ctx, void *stream, mpe_track_score_state *state, const mpe_track_score_args *a);
int mpe_track_score_launches(mpe_ctx *ctx, const mpe_track_score_state *state, int64_t *n);
int mpe_track_score_result(mpe_ctx *ctx, void *stream, mpe_track_score_state *state, mpe_track_score_totals *out);
/* The per-identity and per-track state as it stands, to host arrays (any may be NULL); synchronises `stream`.
 * h_ident [4][gid_cap]: last, present, matched, bits (1: matched in some frame, 2: the previous record was a miss);
 * h_pred_count [tid_cap]; h_table [gid_cap][tid_cap]. */
int mpe_track_score_read(mpe_ctx *ctx, void *stream, mpe_track_score_state *state, int32_t *h_ident, int32_t *h_pred_count,
                         int32_t *h_table);

/* Skeleton: bone lengths held constant along a track.  The tracker says which rows are one body over time; the lengths of
 * that body's bones are learned from its own frames (a histogram per (track, bone), its lower median) and every pose of
 * the track is then moved, within its own frame, towards those lengths.  The rule (harness/skeleton.py states it in
 * numpy, and the two agree bit for bit):
 *   State, fixed at create time (mpe_skel_config): pcap, n_joints, pose_f64, tid_cap, the bone list int32 [n_bones][2] = (parent, child)
 *   with 0 <= parent != child < n_joints, 1 <= n_bones <= MPE_SKEL_MAX_BONES, and bin_width (f64 metres, finite, > 0).
 *   It holds hist u32 [tid_cap][n_bones][MPE_SKEL_BINS], len f64 and count i32 [tid_cap][n_bones], the int64 counters
 *   out_of_range and over_ids, and the sticky status word.
 *   Detections and joint presence as in mpe_smooth_batch.  Row p of frame f is a detection when p < d_n_persons[f],
 *   d_track_id[f][p] >= 0 and, with joint_flags == 0, d_flags[f][p] != 0; joint_flags == 0: all joints of a detection
 *   are present; joint_flags == 1: joint j is present when d_flags[f][p][j] != 0.  A joint is ACTIVE when it is present,
 *   inside joint_mask and its three stored coordinates are finite; a bone is LIVE in a row when both its joints are
 *   active.  Coordinates are widened to f64; nothing is contracted; sqrt and / are IEEE.
 *   Length of a bone from coordinates x: d = x_child - x_parent; s = (dx*dx + dy*dy) + dz*dz; l = sqrt(s).
 *   mpe_skel_observe_batch: for every detection with id t < tid_cap and every live bone b, l from the stored
 *   coordinates and q = l / bin_width; when l > 0 and q < MPE_SKEL_BINS, hist[t][b][(int)q] += 1, otherwise
 *   out_of_range += 1.  A detection with t >= tid_cap adds 1 to over_ids (once per row, whatever its bones) and sets
 *   MPE_SKEL_OVER_IDS; it reaches neither hist nor out_of_range.  Only integer additions reach memory: the state after
 *   a sequence is the same bits for any chunking and any frame order.
 *   mpe_skel_update(min_samples): for every (t, b), n = the sum of hist[t][b][..] and count = n (INT32_MAX at most).
 *   n < max(min_samples, 1): len = 0.0, no length.  Otherwise k* = the smallest k with 2 * (hist[..0] + .. + hist[..k])
 *   >= n (the lower median) and len = ((double)k* + 0.5) * bin_width.
 *   mpe_skel_set_lengths copies a table [tid_cap][n_bones] f64 in DEVICE memory over len, ordered on `stream`, as it is;
 *   an entry has a length when it is > 0 and finite.  count keeps what the last update left.
 *   mpe_skel_fit_batch(iters): every (frame, row) on its own.  A bone is CONSTRAINED in a row when it is live and
 *   len[t][b] has a length; a row is PROCESSED when it is a detection with t < tid_cap and a constrained bone.  The
 *   working copy x holds the active joints in f64.  For sweep = 1 .. iters, for each constrained bone in LIST ORDER with
 *   L = len[t][b]: l from x; unless l > 0 the bone is skipped; e = (l - L) / l; h = 0.5 * e; per axis a, with d taken
 *   before any update of this bone: m = h * d_a; x_parent[a] = x_parent[a] + m; x_child[a] = x_child[a] - m.
 *   d_poses_out: a joint that is an end of a constrained bone of a processed row gets its working value rounded once to
 *   the pose type; every other joint and every other row is copied through bit for bit (absent joints and NaNs as well).
 *   d_err[f][p] = {e0, e1}: the left fold from 0.0 over the constrained bones in list order of `if (v > m) m = v` with
 *   v = |l - L|, l from the stored input coordinates (e0) and from the final working values before rounding (e1); both
 *   -1.0 for a row that is not processed.  d_n_bones[f][p] = the constrained bones, 0 for a row that is not processed.
 *   The fit changes nothing in the state and counts nothing.
 * mpe_skel_create allocates all device memory the calls need (MPE_ERR_CAPACITY when tid_cap * n_bones * MPE_SKEL_BINS * 4
 * bytes exceed MPE_SKEL_MAX_HIST_BYTES or pcap > MPE_TRACK_MAX_PERSONS; MPE_ERR_INVALID, with the values in
 * mpe_last_error, for anything else that is wrong); no later call allocates.  mpe_skel_reset zeroes hist, len, count,
 * the counters and the status, ordered on `stream`.  observe, update and fit are one kernel each whatever n_frames is
 * (mpe_skel_launches counts them as mpe_track_launches does), ordered on `stream`, and neither synchronise nor allocate;
 * n_frames == 0 does nothing.  MPE_ERR_INVALID, with the values in mpe_last_error: sizes or a pose type other than the
 * state's, joint_flags outside {0, 1}, iters outside 1 .. MPE_SKEL_MAX_ITERS, d_poses_out == d_poses; n_frames > 2^23:
 * MPE_ERR_CAPACITY.  mpe_skel_get_lengths is the only call that synchronises (`stream`): len, count, {out_of_range,
 * over_ids} and the status to host arrays (any may be NULL).  Calls on one state belong on one stream. */
#define MPE_SKEL_BINS 512
#define MPE_SKEL_MAX_BONES 32
#define MPE_SKEL_MAX_ITERS 64
#define MPE_SKEL_OVER_IDS 1
#define MPE_SKEL_MAX_HIST_BYTES (256u << 20)
typedef struct mpe_skel_state mpe_skel_state;
typedef struct {
    int32_t pcap, n_joints;
    int32_t pose_f64;              /* 0: f32 poses; 1: f64 */
    int32_t tid_cap;               /* track ids 0 .. tid_cap - 1 have a row in the tables */
    int32_t n_bones, reserved;
    double bin_width;              /* metres, finite, > 0 */
    const int32_t *bones;          /* host, [n_bones][2] (parent, child); copied */
} mpe_skel_config;
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    int32_t iters;                 /* mpe_skel_fit_batch: sweeps, 1 .. MPE_SKEL_MAX_ITERS; observe does not read it */
    uint32_t joint_mask;
    int32_t reserved;
    const void *d_poses;
    const uint8_t *d_flags;
    const int32_t *d_n_persons;    /* [n_frames] */
    const int32_t *d_track_id;     /* [n_frames][pcap], mpe_track_batch's */
    void *d_poses_out;             /* fit: the type and shape of d_poses, another buffer */
    double *d_err;                 /* fit: [n_frames][pcap][2] */
    uint8_t *d_n_bones;            /* fit: [n_frames][pcap] */
} mpe_skel_args;
int mpe_skel_create(mpe_ctx *ctx, const mpe_skel_config *cfg, mpe_skel_state **out);
int mpe_skel_reset(mpe_ctx *ctx, void *stream, mpe_skel_state *state);
int mpe_skel_destroy(mpe_ctx *ctx, mpe_skel_state *state);
int mpe_skel_observe_batch(mpe_ctx *ctx, void *stream, mpe_skel_state *state, const mpe_skel_args *a);
int mpe_skel_update(mpe_ctx *ctx, void *stream, mpe_skel_state *state, int32_t min_samples);
/* d_len: DEVICE memory, [tid_cap][n_bones] f64; a host pointer is not detected and faults.  Copied on `stream`, no synchronisation. */
int mpe_skel_set_lengths(mpe_ctx *ctx, void *stream, mpe_skel_state *state, const double *d_len);
int mpe_skel_get_lengths(mpe_ctx *ctx, void *stream, mpe_skel_state *state, double *h_len, int32_t *h_count, int64_t *h_counters,
                         int32_t *h_status);
int mpe_skel_fit_batch(mpe_ctx *ctx, void *stream, mpe_skel_state *state, const mpe_skel_args *a);
int mpe_skel_launches(mpe_ctx *ctx, const mpe_skel_state *state, int64_t *n);

/* The body-level fit: one cost per tracked row -- the reprojection error of every joint over the cameras that saw it plus
 * the deviation of every bone from the length of its track -- minimised joint by joint, the neighbours held, by
 * Levenberg-Marquardt steps of three unknowns.  mpe_refine_batch sees the pixels and not the body, mpe_skel_fit_batch the
 * body and not the pixels; this call stands in for the pair, and it moves the joint one camera saw, which the refinement
 * declines.  All binary64, every operation named below rounded on its own (nothing fused), quotients and roots correctly
 * rounded.  harness/skeleton_refine.py states the same in numpy, and the two agree bit for bit.
 *   Rows.  The pose rows of n_frames frames as mpe_skel_fit_batch takes them; detections, ACTIVE joints, LIVE and
 *   CONSTRAINED bones and PROCESSED rows exactly as there.  Every row that is not processed is copied through bit for bit.
 *   Frame map.  d_frame[f] is the frame of batch b whose heads pose-frame f is observed in; NULL: f itself, and n_frames
 *   is then the batch's.  An entry outside 0 .. b->n_frames - 1: the frame's rows are copied through and every d_status
 *   of the frame is MPE_BODY_REFINE_BAD_FRAME.
 *   Observations.  Camera c observes active joint j of a processed row when mpe_reproject_batch, given d_persons /
 *   d_n_persons / d_flags / joint_flags / joint_mask / threshold, would count (f, p, c, j) on the heads of frame
 *   d_frame[f]; x, y = that detection.  A flag of any non-zero value is a flag: a joint mpe_smooth_batch filled in
 *   (MPE_SMOOTH_FILLED) is present and observable.  n_views = the number of observing cameras.  An active joint whose
 *   start has pc_2 <= 0 (or NaN) in an observing camera is BAD_START: it is held at its input and still anchors its
 *   bones.  A joint is FREE when it is active, not BAD_START and has an observing camera or is an end of a constrained bone.
 *   Colours, fixed at create time.  Over j increasing, colour[j] = the least colour no lower-numbered joint that shares a
 *   bone with j holds.
 *   Local cost C_j(Y) of joint j at Y, the neighbours at their working values: the left fold from 0.0 over the observing
 *   cameras in increasing c of rho(e_c) -- projection, e, rho and the weight w_c are those of mpe_refine_batch -- then,
 *   when kappa = bone_weight (pixels per metre) is > 0, over the constrained bones incident to j in list order, N the
 *   other end and L the bone's length: d_a = Y_a - N_a ; s = (d_0*d_0 + d_1*d_1) + d_2*d_2 ; l = sqrt(s) ;
 *   q = kappa*(l - L) ; C = C + q*q.  bone_weight == 0 adds no bone term anywhere.
 *   One update of a free joint at Y.  A_kl and g_k from the observing cameras exactly as in mpe_refine_batch; then per
 *   incident constrained bone in list order with l > 0: n_a = d_a / l ; m_a = kappa*n_a ; A_kl = A_kl + m_k*m_l ;
 *   g_k = g_k + m_k*q (a bone whose l is not > 0 adds nothing here and still counts in the cost).  M = A +
 *   lambda_j*diag(A), solved by the LDL^T lines of mpe_refine_batch; a pivot that is not > 0 or a delta that is not finite
 *   rejects the update.  The trial Y + delta is accepted only if pc_2 > 0 there in every observing camera and
 *   C_j(trial) < C_j(Y) (strict; a NaN rejects).  lambda_j starts at 1e-3 and lives across sweeps: accepted
 *   max(lambda_j / 10, 1e-12), rejected lambda_j * 10.
 *   Order.  For sweep = 1 .. sweeps, for colour = 0 .. n_colours - 1, every free joint of that colour takes one update,
 *   reading its neighbours as they stood before the colour step; two joints of one colour share no bone, so the result is
 *   that of the joints walked one by one in (sweep, colour, j) order.  The sweep count is fixed: no early exit.
 *   d_poses_out: a joint that accepted at least one update gets its working value rounded once to the pose type;
 *   everything else keeps the input bits.  d_status (bits below; _ONE_VIEW: n_views == 1) and d_n_views are 0 in a row
 *   that is not processed (_BAD_FRAME apart).  d_cost[f][p] = {the pixel part and the bone part of the row's cost at the
 *   start, then at the end}, -1.0 for a row that is not processed: the pixel part is the fold from 0.0 over the active
 *   joints in increasing j of the joint's camera fold, the bone part the fold from 0.0 over the constrained bones in list
 *   order of q*q (0.0 with bone_weight == 0); held joints count.  d_err and d_n_bones as mpe_skel_fit_batch defines them.
 * One launch whatever n_frames is, counted by mpe_skel_launches, ordered on `stream`; it neither synchronises nor
 * allocates, changes nothing in the state and needs no weights in the context.  n_frames == 0 does nothing.
 * MPE_ERR_INVALID, with the values in mpe_last_error: sizes or a pose type other than the state's, n_joints other than the
 * context's, joint_flags outside {0, 1}, sweeps outside 1 .. MPE_SKEL_MAX_ITERS, a negative (or NaN) bone_weight, huber_px
 * or threshold, d_poses_out == d_poses, a NULL required pointer, d_frame == NULL with n_frames other than the batch's;
 * n_frames > 2^23: MPE_ERR_CAPACITY. */
enum {
    MPE_BODY_REFINE_FREE = 1,
    MPE_BODY_REFINE_MOVED = 2,
    MPE_BODY_REFINE_BAD_START = 4,
    MPE_BODY_REFINE_ONE_VIEW = 8,
    MPE_BODY_REFINE_BAD_FRAME = 16
};
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    int32_t sweeps;                /* 1 .. MPE_SKEL_MAX_ITERS                                        */
    uint32_t joint_mask;
    float threshold;               /* 0.5, as for mpe_reproject_batch                                */
    double bone_weight;            /* pixels per metre, >= 0; 0: no bone term                        */
    double huber_px;               /* pixels, >= 0; 0: plain least squares                           */
    const void *d_poses;
    const uint8_t *d_flags;
    const int32_t *d_n_persons;    /* [n_frames] */
    const int32_t *d_track_id;     /* [n_frames][pcap], mpe_track_batch's */
    const int32_t *d_persons;      /* [n_frames][pcap][V], head ids within frame d_frame[f] of the batch */
    const int32_t *d_frame;        /* [n_frames] or NULL */
    void *d_poses_out;             /* the type and shape of d_poses, another buffer */
    uint8_t *d_status, *d_n_views; /* [n_frames][pcap][J] */
    double *d_cost;                /* [n_frames][pcap][4] */
    double *d_err;                 /* [n_frames][pcap][2] */
    uint8_t *d_n_bones;            /* [n_frames][pcap] */
} mpe_body_refine_args;
int mpe_body_refine_batch(mpe_ctx *ctx, void *stream, mpe_skel_state *state, const mpe_batch *b, const mpe_body_refine_args *a);

/* Relink: a person who returns after a long gap gets the identity they had.  mpe_track_batch links a detection only a few
 * frames back and only within its gate; whoever walks behind a pillar or leaves the volume comes back under a new id.  This
 * stage sits between the tracker and everything that reads its ids: a newborn track takes the id of a lost track with the
 * same bone lengths and, optionally, a plausible position.  It is causal (an id handed out is never revised), needs no
 * weights, and a sequence fed in any chunking gets the same result.  The rule (harness/relink.py states it in numpy, and
 * the two agree bit for bit):
 *   State, fixed at create time (mpe_relink_config): the sizes, the bone list as mpe_skel_create takes it, and the options.
 *   It holds frame (the frames seen), canon i32 [tid_cap] (-1 until the id has been seen) and one record per canonical id:
 *   last_frame (-1: none), last_pose f64 [J][3] with its active-joint mask, sum f64 and cnt i32 [n_bones]; the int64
 *   counters births, linked and over_ids and the sticky status word.
 *   Detections, presence, ACTIVE joints, LIVE bones and the length of a bone exactly as mpe_skel_observe_batch defines them
 *   (joint_mask cuts the joints that count at all).  A length is ACCEPTED when the bone is live, l > 0 and l <= max_bone_m.
 *   Per frame, in order; f counts over the whole sequence and an empty frame counts too:
 *   1. a detection with t >= tid_cap keeps its id, adds 1 to over_ids and sets MPE_RELINK_OVER_IDS; it takes no further part.
 *   2. a detection with canon[t] >= 0 is KNOWN and its record canon[t] is PRESENT in this frame; every other detection is a
 *      BIRTH.  A later row that repeats an id gets the same output id and touches nothing.
 *   3. rows = the births in row order; columns = the records c in increasing c with last_frame >= 0, not present, and
 *      min_gap <= g <= max_gap for g = f - last_frame.
 *   4. cost of (row, column) over the bones in list order: a bone counts when the birth has an accepted length l of it and
 *      the record cnt >= min_samples; m = sum / (double)cnt ; v = |l - m| ; cost = (the left fold of v from 0.0) /
 *      (double)(the count of such bones), +inf with fewer than min_bones of them.
 *   5. position gate, when reach_m > 0: d = the pair cost of mpe_track_batch between the birth's pose and last_pose over
 *      the joints active in both and inside used_joint_mask; the pair is kept only when d < reach_m + reach_per_frame_m *
 *      (double)g, product and sum rounded on their own; a pair with no common joint is not kept.
 *   6. a pair is linkable when cost < gate_m (strict; a NaN never links).
 *   7. greedy, as in mpe_track_batch: the linkable pair of least cost, ties to the lowest row, then the lowest column, is
 *      linked and both are removed, until none is left.
 *   8. a linked birth t -> c: canon[t] = c, d_link_cost and d_link_gap = g for that row, linked += 1.
 *   9. an unlinked birth: canon[t] = t, births += 1.
 *   10. every detection with t < tid_cap, taking the first row of each canonical id, updates its record: per accepted bone
 *      sum = sum + l and cnt += 1; last_pose and its mask = this row's active joints; last_frame = f.
 *   d_ids[f][p] = canon[t]; -1 where the input has no detection; t itself for t >= tid_cap.  d_link_cost[f][p] = -1.0
 *   unless the row is a linked birth.  d_link_gap[f][p] = the gap of a linked birth, 0 for any other detection, -1 for none.
 *   A canonical id is a tracker id and never larger than the id it replaces.  Nothing is contracted; sqrt and / are IEEE.
 * mpe_relink_create allocates all device memory the calls need, scratch for max_frames frames per call included
 * (MPE_ERR_CAPACITY for pcap > MPE_TRACK_MAX_PERSONS, tid_cap > MPE_RELINK_MAX_TID_CAP or max_frames > 2^23;
 * MPE_ERR_INVALID, with the values in mpe_last_error, for a bone list mpe_skel_create would decline, an option that is
 * not finite, gate_m or max_bone_m not > 0, a negative reach, min_gap < 1, max_gap < min_gap or > MPE_RELINK_MAX_GAP,
 * min_samples < 1, min_bones outside 1 .. n_bones); no later call allocates.  mpe_relink_reset starts a new sequence,
 * ordered on `stream`.  mpe_relink_batch is TWO kernels whatever n_frames is and whatever the frames hold
 * (mpe_relink_launches counts them as mpe_track_launches does), ordered on `stream`; it neither synchronises nor
 * allocates; n_frames == 0 does nothing.  MPE_ERR_INVALID: sizes or a pose type other than the state's, joint_flags
 * outside {0, 1}, a NULL pointer; MPE_ERR_CAPACITY: n_frames > max_frames, or a sequence of 2^31 frames or more.
 * mpe_relink_read is the only call that synchronises (`stream`): {births, linked, over_ids} and the status to host memory
 * (either may be NULL).  Calls on one state belong on one stream. */
#define MPE_RELINK_MAX_TID_CAP 4096
#define MPE_RELINK_MAX_GAP (1 << 30)
#define MPE_RELINK_OVER_IDS 1
typedef struct mpe_relink_state mpe_relink_state;
typedef struct {
    int32_t pcap, n_joints;
    int32_t pose_f64;              /* 0: f32 poses; 1: f64 */
    int32_t tid_cap;               /* track ids 0 .. tid_cap - 1 have a record, 1 .. MPE_RELINK_MAX_TID_CAP */
    int32_t n_bones;
    int32_t max_frames;            /* frames per mpe_relink_batch, at most */
    int32_t min_gap, max_gap;      /* frames since the lost track was last seen, both ends included */
    int32_t min_samples;           /* a record's bone counts only with this many lengths */
    int32_t min_bones;             /* fewest bones a birth and a record must have in common */
    uint32_t used_joint_mask;      /* joints the position gate looks at */
    uint32_t joint_mask;           /* joints that count at all */
    double gate_m;                 /* a link needs a bone-length cost strictly below this, metres */
    double max_bone_m;             /* longest length that is accepted */
    double reach_m;                /* 0: no position gate */
    double reach_per_frame_m;      /* growth of the position gate per frame of gap */
    const int32_t *bones;          /* host, [n_bones][2] (parent, child); copied */
} mpe_relink_config;
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    int32_t reserved;
    const void *d_poses;
    const uint8_t *d_flags;
    const int32_t *d_n_persons;    /* [n_frames] */
    const int32_t *d_track_id;     /* [n_frames][pcap], mpe_track_batch's */
    int32_t *d_ids;                /* [n_frames][pcap] */
    double *d_link_cost;           /* [n_frames][pcap] */
    int32_t *d_link_gap;           /* [n_frames][pcap] */
} mpe_relink_args;
int mpe_relink_create(mpe_ctx *ctx, const mpe_relink_config *cfg, mpe_relink_state **out);
int mpe_relink_reset(mpe_ctx *ctx, void *stream, mpe_relink_state *state);
int mpe_relink_destroy(mpe_ctx *ctx, mpe_relink_state *state);
int mpe_relink_batch(mpe_ctx *ctx, void *stream, mpe_relink_state *state, const mpe_relink_args *a);
int mpe_relink_launches(mpe_ctx *ctx, const mpe_relink_state *state, int64_t *n);
/* h_counters [3] = births, linked, over_ids; synchronises `stream`. */
int mpe_relink_read(mpe_ctx *ctx, void *stream, mpe_relink_state *state, int64_t *h_counters, int32_t *h_status);

/* ---- the poses written as JSON on the device (csrc/jsonwrite.hip, csrc/fmt_double.h) -----------------------
 * One line per frame, in frame order, each exactly what Python's json.dumps(obj) + "\n" writes (default separators) for
 *   obj  = {"frame": frame_start + f, "ids": [d_track_id of each written row], "bodies": [body, ...]}
 *   body = {"<j>": [x, y, z], ...}      j ascending
 * (harness/write_poses.py: write_lines states it with numpy and json.dumps, and the two agree byte for byte).
 *   Row p of frame f is looked at when p < min(max(d_n_persons[f], 0), pcap).  Its flagged joints are all J with
 *   joint_flags == 0 and d_flags[f][p] != 0, and with joint_flags == 1 the j with d_flags[f][p][j] != 0.  Every
 *   coordinate is written as (double)x * scale, one IEEE multiply (1.0: metres; 100.0: the centimetres of bodies_3D);
 *   f32 poses are widened exactly first.  The written joints of a row are its flagged joints within joint_mask whose
 *   three scaled coordinates are all finite; a flagged joint of the mask that is dropped because one is not sets
 *   MPE_WRITE_NONFINITE in d_status[f].  A row without a written joint appears neither in "ids" nor in "bodies".
 *   "ids" is there exactly when d_track_id is not NULL; ids are written as plain integers, -1 included.
 *   A number is the shortest decimal that reads back to the same double, the closest to it among those, in the layout of
 *   Python's repr (positional for 1e-4 <= |x| < 1e16 with ".0" behind an integer, otherwise d[.ddd]e+XX; "-0.0"), at
 *   most 24 bytes; the device always produces it.
 * A line is a function of its own frame alone: the outputs of any chunking of a recording, joined, are the output of the
 * whole recording.  The body grammar is the one mpe_json_parse_bodies_device reads, so with n_joints <= 31 and scale 100
 * the extents of d_bodies_extent can go back in as mpe_json_entry.
 * Outputs: d_text (line f is d_text[d_frame_off[f] .. d_frame_off[f + 1])), d_frame_off [n_frames + 1], d_bodies_extent
 * [n_frames][2] (begin and end of the "bodies" list with its brackets, offsets into d_text), d_rows_written [n_frames],
 * d_status [n_frames], d_total [2]: the bytes needed and the OR of every d_status.  When the bytes needed exceed text_cap
 * MPE_WRITE_CAPACITY is set in d_total[1], d_total[0] and d_frame_off still hold the need, and nothing is stored at or
 * behind d_text + text_cap; the text below it is then not to be used.  mpe_json_write_bound is a size that is always
 * enough.  d_scratch: mpe_json_write_scratch_bytes(n_frames, pcap, n_joints) bytes of device memory, 16-byte aligned.
 * Ordered on `stream`; neither synchronises nor allocates.  Five kernels whatever the frames hold (one for n_frames ==
 * 0, which writes d_frame_off[0] = 0 and d_total): mpe_json_write_launches counts the launches this context queued for
 * mpe_json_write_poses, on the host.  A line of up to MPE_JSON_WRITE_STAGE_BYTES is put together on chip and stored in
 * 16-byte pieces, a longer one is written to d_text directly; the bytes are the same.
 * MPE_ERR_INVALID: a NULL pointer (d_track_id may be), n_joints other than the context's, n_frames or frame_start
 * negative (frame_start at most 2^62), pcap < 1, pose_f64 / joint_flags other than 0 or 1, a scale that is NaN or
 * infinite, text_cap of 2^32 or more, scratch_bytes below the need.  MPE_ERR_CAPACITY: pcap >
 * MPE_JSON_WRITE_MAX_PERSONS, n_frames > 2^23, or 2^31 coordinates or more in one call.
 * mpe_format_f64 runs the same conversion on a plain array: d_slots [n][MPE_JSON_WRITE_SLOT_BYTES] receives the tokens
 * (the bytes behind a token are left as they were), d_len [n] their lengths, 0 for an infinity or a NaN. */
#define MPE_WRITE_NONFINITE 1
#define MPE_WRITE_CAPACITY 2
#define MPE_JSON_WRITE_SLOT_BYTES 32
#define MPE_JSON_WRITE_STAGE_BYTES 16384
#define MPE_JSON_WRITE_MAX_PERSONS 1024
typedef struct {
    int32_t n_frames, pcap, n_joints;
    int32_t pose_f64;              /* 0: d_poses f32 [n_frames][pcap][J][3]; 1: f64                  */
    int32_t joint_flags;           /* 0: d_flags [n_frames][pcap] u8; 1: d_flags [n_frames][pcap][J] */
    uint32_t joint_mask;
    int64_t frame_start;           /* "frame" of the first line */
    double scale;
    const void *d_poses;
    const uint8_t *d_flags;
    const int32_t *d_n_persons;    /* [n_frames] */
    const int32_t *d_track_id;     /* [n_frames][pcap]; NULL: no "ids" */
    char *d_text;                  /* [text_cap] */
    uint64_t text_cap;
    int64_t *d_frame_off;          /* [n_frames + 1] */
    uint32_t *d_bodies_extent;     /* [n_frames][2] */
    int32_t *d_rows_written;       /* [n_frames] */
    int32_t *d_status;             /* [n_frames] */
    int64_t *d_total;              /* [2] */
    void *d_scratch;
    size_t scratch_bytes;
} mpe_json_write_args;
int mpe_json_write_poses(mpe_ctx *ctx, void *stream, const mpe_json_write_args *a);
/* 0 for a negative argument */
size_t mpe_json_write_bound(int32_t n_frames, int32_t pcap, int32_t n_joints, int32_t with_ids);
size_t mpe_json_write_scratch_bytes(int32_t n_frames, int32_t pcap, int32_t n_joints);
int mpe_json_write_launches(mpe_ctx *ctx, int64_t *n);
int mpe_format_f64(mpe_ctx *ctx, void *stream, const double *d_values, int64_t n, char *d_slots, uint8_t *d_len);


/* Timing probe for bench.py: average duration (ms) of the dominant GEMM launches measured
 * with HIP events on the launch stream during the last mpe_match_batch / mpe_mlp3d_batch
 * when profiling is enabled; see bench.py. */
int mpe_profile_enable(mpe_ctx *ctx, int32_t on);      /* 1 = on, records cleared; 2 = on, records kept (resume); 0 = off (records kept until read) */
int mpe_profile_read(mpe_ctx *ctx, double *gemm_ms, double *gemm_flop, int64_t *gemm_launches,
                     double *total_ms);
/* mpe_profile_read reports the launches on the fp32 MFMA (the dominant kernel, k_linear_dma); the split-bf16 launches of the
 * same records (MLP mode 3: k_linear_sb*, fp32-equivalent FLOPs = 2 M N K, executed on the bf16 MFMA as six products) are kept
 * apart and read here, after mpe_profile_read. */
int mpe_profile_read_split(mpe_ctx *ctx, double *ms, double *flop, int64_t *launches);
/* ... and the plain bf16 launches of the reduced-precision modes (configs[4]): one bf16 product per product, priced against the bf16 peak */
int mpe_profile_read_bf16(mpe_ctx *ctx, double *ms, double *flop, int64_t *launches);
/* How often this context has queued the whole-row layer-0 attention launch (k_l0_attention: layer 0 on device-featurised fp32
 * rows, implicit topology, 40-wide heads, none of MPE_NO_FUSED_ATTENTION / MPE_NO_COEF_EPILOGUE / MPE_FUSED_NO_OVERLAP /
 * MPE_NO_HEAD_SRC_TABLE set) since it was created; counted on the host.  Every other layer-0 call takes the coefficient kernel
 * and the attention kernels of the other layers. */
int mpe_l0_attention_launches(mpe_ctx *ctx, int64_t *n);

#ifdef __cplusplus
}
#endif
#endif /* MPE_H */
