// ahv_launch.h -- the host-side interface between the .hip files: the scorer's launch descriptors and ONE prototype of every
// launcher and size function that one file defines and another calls (the C ABI in ahv_abi.hip calls all of them; the
// developer benchmarks include the kernel sources, tools/kbench.cpp).  Every defining file includes this header.  C++ takes a
// definition that drifted from its prototype for an overload, not an error: the library's link line refuses undefined
// symbols (Makefile), which is what turns the drift into a failed build.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ahv.h"  // the encoder's weight structs

namespace ahv {

struct ScoreLaunch {
    const float* vol_src;   // [B][16][8][8][8]
    const float* tgt;       // target features [B][32][64], or the target volume [B][16][8][8][8] if tgt_is_volume
    bool tgt_is_volume;     // ahv_verify_pair_f32: forward_3d2d(vol_tgt) is computed inside the launch
    const float* R;
    int64_t r_batch_stride, n_offset;
    const float *W1, *W2, *b2;
    int B;
    int64_t N;
    float* scores;          // [B][N] or NULL
    int64_t* best_key;      // [B] or NULL
    float* feat_tgt_out;    // [B][32][64] or NULL (tgt_is_volume only): the target features the launch computed
    int num_cu, spare_cu;   // compute units of the device; how many of them to leave without a workgroup
    bool split_f16;         // AHV_SCORE_SPLIT_F16
    bool no_teams;          // AHV_SCORE_NO_TEAMS
    uint64_t* clock_stamps; // diagnostic entry point, else NULL
};

struct ScorePlan {
    int gx, gy;       // grid: x strides the hypotheses, y the batch
    int64_t n_main;   // hypotheses [0, n_main) by single waves, [n_main, N) by teams of four
};

// ---- ahv_score.hip ----
ScorePlan plan_score_launch(int B, int64_t N, int num_cu, int spare_cu, bool teams);
hipError_t launch_score_hypotheses(const ScoreLaunch& a, hipStream_t stream);
// the training forward: scores [B][N] and, in u_out, 8 KB of pre-activations per hypothesis for the backward
hipError_t launch_score_hypotheses_train(const ScoreLaunch& a, float* u_out, hipStream_t stream);

// ahv_coarse_to_fine_f32: the verify step on the coarse set (a.coarse, tgt = the target volume, n_offset 0) and, in the
// same launch, on the refinement set R* D[n] of its winner (coarse_to_fine_kernel, ahv_score.hip)
struct CoarseToFineLaunch {
    ScoreLaunch coarse;
    const float* D;            // [N2][3][3]
    int64_t N2;
    float* scores2;            // [B][N2] or NULL
    int64_t* best_key2;        // [B], EMPTY on entry and exit
    uint32_t* sync;            // [2 B + 1], zero on entry and exit (last word: error flag, sticky)
    float* R_pred;             // [B][3][3]
    float *fine_score, *coarse_score;
    int64_t *fine_idx, *coarse_idx;
};
hipError_t launch_coarse_to_fine(const CoarseToFineLaunch& a, hipStream_t stream);
hipError_t launch_unpack_best(const int64_t* best_key, int B, float* best_score, int64_t* best_idx, hipStream_t stream);

// ---- ahv_ops.hip ----
hipError_t launch_forward_3d2d(const float* vol, const float* W1, const float* W2, const float* b2, int64_t M, float* out,
                               int num_cu, hipStream_t stream);
hipError_t launch_score_features(const float* f_src, const float* f_tgt, int B, int64_t N, float* scores, int num_cu,
                                 hipStream_t stream);
hipError_t launch_random_rotations(uint64_t seed, uint64_t offset, int64_t N, float* out, hipStream_t stream);
hipError_t launch_so3_grid(int64_t n_total, int64_t offset, int64_t N, float* out, hipStream_t stream);
hipError_t launch_zero_fill(void* const* ptrs, const size_t* bytes, int count, hipStream_t stream);
// rows of `elems` floats, `stride` floats apart (stride >= elems): only the rows are written
hipError_t launch_zero_fill_strided(float* p, int64_t elems, int64_t stride, int64_t rows, hipStream_t stream);

// ---- ahv_rotate.hip ----
hipError_t launch_rotate_volume(const float* vol, int64_t vol_batch_stride, const float* R, int64_t N, int C, int D, int H, int W,
                                float* out, int num_cu, hipStream_t stream);
hipError_t launch_rotate_volume_backward(const float* grad_out, int64_t vol_batch_stride, const float* R, int64_t N, int C, int D,
                                         int H, int W, float* grad_vol, int num_cu, hipStream_t stream);

// ---- ahv_select.hip ----
hipError_t launch_argmax(const float* scores, int B, int64_t N, int64_t n_offset, int64_t* best_key, int num_cu,
                         hipStream_t stream);
hipError_t launch_fill_keys(int64_t* best_key, int B, hipStream_t stream);
// partial lists per sample of a top-K launch over N scores: a pure function of N (the workspace is sized by it)
int topk_parts(int64_t N);
hipError_t launch_topk(const float* scores, int B, int64_t N, int64_t n_offset, int K, int64_t* keys, int64_t* workspace,
                       bool carry, hipStream_t stream);
hipError_t launch_topk_merge(const int64_t* lists, int P, int B, int K, int64_t* keys, bool carry, hipStream_t stream);
hipError_t launch_select_topk(int64_t* keys, int K, const float* R, int64_t r_batch_stride, int64_t n_offset, int64_t N, int B,
                              float* R_out, float* scores_out, int64_t* idx_out, bool reset, hipStream_t stream);
hipError_t launch_compose_rotations_topk(const int64_t* keys, int K, const float* R, int64_t r_batch_stride, int64_t n_offset,
                                         int64_t N, const float* D, int64_t N2, int B, float* out, hipStream_t stream);
hipError_t launch_compose_rotations_indexed(const int64_t* idx, const float* R, int64_t r_batch_stride, int64_t N, const float* D,
                                            int64_t M, int B, float* out, hipStream_t stream);
// hypotheses per sample of the alive state of ahv_topk_modes_f32: N rounded up to a lane's four
int64_t topk_modes_state_stride(int64_t N);
// K + 1 launches: the list filled EMPTY, round 0, rounds 1 .. K - 1 (each reads the entry the one before reduced)
hipError_t launch_topk_modes(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset, int K,
                             float tau, int64_t* keys, int64_t* state, hipStream_t stream);
// launch_topk_modes with the rounds j >= 1 taken modulo the group (axis == nullptr: the finite part alone)
hipError_t launch_topk_modes_sym(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset,
                                 int K, float tau, const float* S, int64_t s_batch_stride, int G, const float* axis,
                                 int64_t axis_batch_stride, int64_t* keys, int64_t* state, hipStream_t stream);
hipError_t launch_sym_fold(const float* R, int64_t r_batch_stride, int B, int64_t N, const float* S, int64_t s_batch_stride, int G,
                           const float* axis, int64_t axis_batch_stride, const float* anchors, int K, float tau, int64_t keep,
                           const float* V, float* R_out, float* V_out, int32_t* which, int32_t* elem, float* trace,
                           hipStream_t stream);
hipError_t launch_so3_ascent_candidates(const float* R_cur, const float* grad_R, const float* theta, const float* ladder, int L,
                                        int B, int K, float* R_cand, hipStream_t stream);
hipError_t launch_so3_ascent_select(const float* R_cand, const float* cand_scores, const float* ladder, int L, int B, int K,
                                    float* R_cur, float* score_cur, float* theta, hipStream_t stream);

// ---- ahv_views.hip ----
hipError_t launch_view_rotations(const float* Q, int64_t q_batch_stride, const float* A, int B, int V, int64_t N, float* out,
                                 hipStream_t stream);
// weights: V floats on the HOST (or nullptr: 1 each), copied into the kernel arguments (the launch itself reads no host memory)
hipError_t launch_fuse_views(const float* scores, const float* Q, int64_t q_batch_stride, const float* A, const float* weights,
                             int B, int V, int64_t N, int64_t n_offset, float tau, bool limit, float* fused, int64_t* best_key,
                             hipStream_t stream);
hipError_t launch_nearest_views(const float* anchor, const float* A, int B, int V, int K, int32_t* view_idx, float* A_sel,
                                hipStream_t stream);
// L4: the row length in 16-byte units; grid (B K rows, up to 64 chunks of a row)
hipError_t launch_gather_views(const void* src, const int32_t* view_idx, int B, int V, int K, int64_t L4, void* dst, bool broadcast,
                               hipStream_t stream);
int64_t view_compact_tiles(int64_t N);
// two launches: the per-tile counts into the workspace, then -- across the kernel boundary -- the slot map, the composed
// matrices, counts and the identity padding.  out == slot == nullptr: counts only (one summing workgroup per sample).
// weights: on the HOST, as for launch_fuse_views.
hipError_t launch_view_rotations_compact(const float* Q, int64_t q_batch_stride, const float* A, const float* weights, int B, int V,
                                         int64_t N, float tau, int64_t capacity, float* out, int32_t* slot, int64_t* counts,
                                         void* workspace, hipStream_t stream);
hipError_t launch_fuse_views_compact(const float* scores, const int32_t* slot, const float* weights, int B, int V, int64_t N,
                                     int64_t capacity, int64_t n_offset, float* fused, int64_t* best_key, hipStream_t stream);

// ---- ahv_posterior.hip ----
size_t posterior_state_stride(int K);
int posterior_parts(int64_t N);
// two launches: one partial state per workgroup into the workspace, then their merge into (or over) the caller's state
hipError_t launch_posterior(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, const float* anchors,
                            int K, float tau, float beta, void* state, void* workspace, bool carry, hipStream_t stream);
hipError_t launch_posterior_merge(const void* states, int P, int B, int K, float beta, void* state, bool carry, hipStream_t stream);
hipError_t launch_posterior_finish(const void* state, int B, int K, float beta, float* log_z, float* entropy, float* mean_score,
                                   int64_t* n_excluded, float* mode_prob, float* rest_prob, float* mode_R_mean, float* R_mean,
                                   float* mode_spread_deg, float* spread_deg, hipStream_t stream);
size_t resample_stride(int64_t N);
// three launches: a record per tile, the scan of the records, the draws (u: [B] on the device, or nullptr)
hipError_t launch_resample(const float* scores, int B, int64_t N, float beta, int64_t M, const float* u, int64_t* idx,
                           void* workspace, hipStream_t stream);

// ---- ahv_track.hip ----
hipError_t launch_diffuse_rotations(const int64_t* idx, const float* R, int64_t r_batch_stride, int64_t N, const int64_t* best_key,
                                    int64_t M, int64_t n_fresh, int B, uint64_t seed, const int64_t* step, float sigma,
                                    float max_angle, float* out, float* omega, hipStream_t stream);
hipError_t launch_predict_rotations(const int64_t* idx, const float* R, int64_t r_batch_stride, const float* V,
                                    int64_t v_batch_stride, int64_t N, const int64_t* best_key, int64_t M, int64_t n_fresh, int B,
                                    uint64_t seed, const int64_t* step, float sigma, float sigma_vel, float damping,
                                    float max_angle, float max_speed, int coast, float* out, float* vel_out, float* omega,
                                    hipStream_t stream);
hipError_t launch_predict_rotations_ctl(const int64_t* idx, const float* R, int64_t r_batch_stride, const float* V,
                                        int64_t v_batch_stride, int64_t N, const int64_t* best_key, int64_t M, const uint32_t* control,
                                        int B, uint64_t seed, const int64_t* step, float damping, float max_angle, float max_speed,
                                        int coast, float* out, float* vel_out, float* omega, hipStream_t stream);
hipError_t launch_track_control(const float* R_cur, const float* V_cur, const int64_t* idx, const float* score, int B, int64_t M,
                                int first, float sigma0, float sigma_vel0, int n_fresh0, float sigma_min, float sigma_max, float gain,
                                float rate, float score_floor, int n_fresh_lost, uint32_t* control, uint8_t* reacquired,
                                hipStream_t stream);
hipError_t launch_track_advance(uint64_t seed, int64_t* step, int B, float* u, hipStream_t stream);
hipError_t launch_smooth_step(const float* R_cur, const float* scores, const float* V_cur, const int64_t* step, int64_t first_step,
                              int B, int64_t M, int64_t H, float beta, float inv4s2, float jump, float damping, float* hist_R,
                              float* hist_P, float* hist_delta, int32_t* hist_back, hipStream_t stream);
hipError_t launch_smooth_backtrace(const float* hist_R, const float* hist_delta, const int32_t* hist_back, const int64_t* step,
                                   int64_t first_step, int B, int64_t M, int64_t H, int64_t F, int64_t* path_idx, float* path_R,
                                   hipStream_t stream);
hipError_t launch_marginal_step(const float* R_cur, const float* scores, const int64_t* step, int64_t first_step, int B, int64_t M,
                                int64_t H, float beta, float inv4s2, float jump, const float* hist_R, const float* hist_P,
                                float* hist_alpha, float* hist_emit, hipStream_t stream);
// F - 1 backward launches (frames t - 1, t - 2, ...: each reads the beta the launch before wrote) and the finish, in stream
// order: a linear chain under capture.
hipError_t launch_marginal_smooth(const float* hist_R, const float* hist_P, const float* hist_alpha, const float* hist_emit,
                                  const int64_t* step, int64_t first_step, int B, int64_t M, int64_t H, int64_t F, float inv4s2,
                                  float jump, float* logw, int64_t* idx, float* R, hipStream_t stream);

// ---- ahv_graph.hip ----
hipError_t launch_pose_graph_init(const float* pair_R, const float* pair_score, const int32_t* edges, int B, int V, int E, int root,
                                  float* A, int32_t* parent_edge, int32_t* reached, hipStream_t stream);
hipError_t launch_pose_graph_propose(const float* A, const float* pair_R, const float* pair_score, const int32_t* edges,
                                     const int32_t* incident, int B, int V, int E, int k, int D, int64_t N, int64_t n_fresh,
                                     uint64_t seed, const int64_t* counter, int sweep, float sigma, float* Q, float* Rrel,
                                     hipStream_t stream);
hipError_t launch_pose_graph_commit(const int64_t* key, const float* Q, int B, int V, int k, int64_t N, float* A, float* node_score,
                                    hipStream_t stream);

// ---- the scorer's backward: its grid rule and its workspace, plain host code (the launchers below, ahv_abi.hip and
// tools/kbench_bwd.cpp all take them from here) ----
// Persistent grid: y strides the batch, x the hypotheses -- one workgroup per CU, but no more along x than a list of N
// has turns of `per_workgroup` hypotheses (a short list is spread over more workgroups), and at least one.  B, N >= 1.
constexpr int kBwdHeadPerWg = 4, kBwdHeadSavedPerWg = 8, kBwdW1PerWg = 4, kBwdVolumePerWg = 2;
constexpr int kBwdHeadDuPerWg = 1;   // the head pass of the rotation gradient: a short list goes one hypothesis per workgroup
inline dim3 backward_grid(int num_cu, int B, int64_t N, int per_workgroup)
{
    const int gy = B < num_cu ? B : num_cu;
    int gx = num_cu / gy;
    const int64_t need = (N + per_workgroup - 1) / per_workgroup;
    if (gx > need) gx = (int)need;
    if (gx < 1) gx = 1;
    return dim3(gx, gy);
}

// The workspace of a backward, in floats: du (2 048 per hypothesis; u on entry of the saved-u backward), one reserved word
// per sample (rounded up to 16 bytes; unused since the dV kernel stopped needing max |du|, kept so the size stays ABI 2.3's),
// then one partial dW1 (32 x 384) per workgroup of kernel 2a.  Kernel 2a runs on backward_grid(num_cu, B, N, kBwdW1PerWg),
// where gx * gy <= (num_cu / gy) * gy <= num_cu: one partial per CU always suffices.  num_cu <= 0 (the device query
// failed: the size is then reported without a device) counts as 1 024, which covers any device.
struct BackwardWs {
    size_t du_floats, pad_floats, partials;
    BackwardWs(int B, int64_t N, int num_cu)
        : du_floats(2048 * (size_t)B * (size_t)N), pad_floats(((size_t)B + 3) & ~(size_t)3),
          partials(num_cu > 0 ? (size_t)num_cu : 1024) {}
    size_t partials_offset() const { return du_floats + pad_floats; }
    size_t floats() const { return partials_offset() + partials * 32 * 384; }
};

// ---- ahv_backward.hip ----
hipError_t launch_score_backward(const float* vol_src, const float* feat_tgt, const float* R, int64_t r_batch_stride,
                                 const float* W1, const float* W2, const float* b2, int B, int64_t N, const float* grad_scores,
                                 float* du_ws, float* dw1_partials, float* grad_vol, float* grad_feat_tgt, float* grad_W1,
                                 float* grad_W2, float* grad_b2, int num_cu, hipStream_t stream, bool saved_u);
// the head pass that leaves du of every hypothesis in du_ws and nothing else (score_backward_head_kernel<false>: no sums
// across hypotheses, no atomics); grad_scores may be null (= all ones)
hipError_t launch_score_backward_head_du(const float* vol_src, const float* feat_tgt, const float* R, int64_t r_batch_stride,
                                         const float* W1, const float* W2, const float* b2, int B, int64_t N,
                                         const float* grad_scores, float* du_ws, int num_cu, hipStream_t stream);

// ---- ahv_bwd_volume.hip ----
hipError_t launch_score_backward_volume(const float* R, int64_t r_batch_stride, const float* W1, int B, int64_t N,
                                        const float* du_ws, float* grad_vol, int num_cu, hipStream_t stream);

// ---- ahv_rotgrad.hip ----
hipError_t launch_score_rotation_grad(const float* vol_src, const float* feat_tgt, const float* R, int64_t r_batch_stride,
                                      const float* W1, const float* W2, const float* b2, int B, int64_t N,
                                      const float* grad_scores, float* du_ws, float* grad_R, int num_cu, hipStream_t stream);
hipError_t launch_rotate_volume_rotation_grad(const float* grad_out, const float* vol, int64_t vol_batch_stride, const float* R,
                                              int64_t N, int C, int D, int H, int W, float* grad_R, int num_cu,
                                              hipStream_t stream);

// ---- ahv_encoder.hip: host side; kernels in ahv_enc_linear.h / ahv_enc_rows.h, shape decisions in ahv_enc_plan.h
// (int: 0, or the hipError_t of the launch that *what then names) ----
size_t transformer_workspace_floats(int B);
int transformer_blocks(const ahv_block_weights* blocks, int depth, float* x_src, float* x_tgt, int B, float* ws, hipStream_t s,
                       const char** what);
size_t forward_2d3d_workspace_floats(int B);
int forward_2d3d(const ahv_aligner_weights* w, const float* l4_src, const float* l4_tgt, int B, float* ws, float* vol_src,
                 float* vol_tgt, hipStream_t s, const char** what);

}  // namespace ahv
